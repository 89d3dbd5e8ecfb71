// triangulate_host_check.cpp -- cs_triangulate.h WITHOUT a GPU: the routines the kernel runs with one match per lane, run here by a serial
// worker (cs::triangulate_pair_serial: one pair, match after match) over a dumped batch.  tests/test_triangulate_ref.py builds it with g++
// (once plain, once under the address and undefined-behaviour sanitizers), writes the dump, and compares what is printed with the numpy
// statement.
//
//   triangulate_host_check run DUMP            per match "m i status route X[3] normal[3] min max cosRays cosS1 cosS2", per pair "pair f ran n_accepted"
//   triangulate_host_check time REPEATS DUMP   run, REPEATS times, and the time of one pass over the batch in ms (one core)
//   triangulate_host_check hvec A B C D        triangulate_dehomogenize on a hand-made homogeneous vector: "hvec ok X[3]"
//   triangulate_host_check scale DUMP X Y Z    steps 5 and 6 alone at the point X Y Z, with pair 0 and the octave scales of match 0 of the
//                                              dump: "scale status normal[3] min max"
//
// DUMP (text, every double in %.17g): n_pairs n_matches / the six parameters in cs_triangulate_params' order / per pair: Tcw1 (7) Tcw2 (7)
// cam1 (6) cam2 (6) median_depth2 first_match end_match / per match: the 12 doubles of a packed record (cs_triangulate.h).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cube_slam_wu_amd/csrc/cs_triangulate.h"

int main(int argc, char** argv) {
  const bool run = argc == 3 && !std::strcmp(argv[1], "run");
  const bool timed = argc == 4 && !std::strcmp(argv[1], "time");
  const bool hvec = argc == 6 && !std::strcmp(argv[1], "hvec");
  const bool scale = argc == 6 && !std::strcmp(argv[1], "scale");
  if (!run && !timed && !hvec && !scale) { std::fprintf(stderr, "usage: %s run DUMP | time REPEATS DUMP | hvec A B C D | scale DUMP X Y Z\n", argv[0]); return 2; }
  if (hvec) {
    const double h4[4] = {std::atof(argv[2]), std::atof(argv[3]), std::atof(argv[4]), std::atof(argv[5])};
    double X[3];
    const bool ok = cs::triangulate_dehomogenize(h4, X);
    std::printf("hvec %d %.17g %.17g %.17g\ntriangulate_host_check: ok\n", ok ? 1 : 0, X[0], X[1], X[2]);
    return 0;
  }
  const int repeats = timed ? std::atoi(argv[2]) : 1;
  if (repeats < 1 || repeats > 1000000) { std::fprintf(stderr, "bad count\n"); return 2; }
  const char* path = argv[timed ? 3 : 2];
  FILE* f = std::fopen(path, "r");
  if (!f) { std::perror(path); return 2; }
  int n_pairs = 0, n_matches = 0;
  cs::TriParams prm;
  bool ok = std::fscanf(f, "%d %d", &n_pairs, &n_matches) == 2 && n_pairs >= 0 && n_matches >= 0;
  ok = ok && std::fscanf(f, "%lf %lf %lf %lf %lf %lf", &prm.min_baseline_ratio, &prm.max_cos_parallax, &prm.chi2_mono, &prm.chi2_stereo, &prm.ratio_factor, &prm.scale_range) == 6;
  if (!ok) { std::fprintf(stderr, "bad header\n"); return 2; }
  std::vector<double> pose(14 * (size_t)n_pairs), cam(12 * (size_t)n_pairs), median(n_pairs), rec((size_t)cs::TRI_MATCH_DOUBLES * n_matches);
  std::vector<int> first(n_pairs), end(n_pairs);
  for (int i = 0; i < n_pairs && ok; i++) {
    for (int k = 0; k < 14 && ok; k++) ok = std::fscanf(f, "%lf", &pose[14 * (size_t)i + k]) == 1;
    for (int k = 0; k < 12 && ok; k++) ok = std::fscanf(f, "%lf", &cam[12 * (size_t)i + k]) == 1;
    ok = ok && std::fscanf(f, "%lf %d %d", &median[i], &first[i], &end[i]) == 3 && 0 <= first[i] && first[i] <= end[i] && end[i] <= n_matches;
  }
  for (size_t k = 0; k < rec.size() && ok; k++) ok = std::fscanf(f, "%lf", &rec[k]) == 1;
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "bad dump\n"); return 2; }

  std::vector<cs::TriPair> pair(n_pairs);
  for (int i = 0; i < n_pairs; i++)
    cs::triangulate_pair_record(&pose[14 * (size_t)i], &pose[14 * (size_t)i + 7], &cam[12 * (size_t)i], &cam[12 * (size_t)i + 6], median[i], prm.min_baseline_ratio, pair[i]);

  if (scale) {
    if (n_pairs < 1 || end[0] - first[0] < 1) { std::fprintf(stderr, "scale needs a match in pair 0\n"); return 2; }
    cs::TriMatchOut o;
    std::memset(&o, 0, sizeof(o));
    for (int k = 0; k < 3; k++) o.X[k] = std::atof(argv[3 + k]);
    const double* m = &rec[(size_t)first[0] * cs::TRI_MATCH_DOUBLES];
    const int status = cs::triangulate_scale_stage(pair[0], prm, m[5], m[11], o);
    std::printf("scale %d %.17g %.17g %.17g %.17g %.17g\ntriangulate_host_check: ok\n", status, o.normal[0], o.normal[1], o.normal[2], o.min_distance, o.max_distance);
    return 0;
  }

  std::vector<double> out8((size_t)cs::TRI_OUT_DOUBLES * n_matches), cos3(3 * (size_t)n_matches);
  std::vector<unsigned char> status(n_matches), route(n_matches);
  std::vector<int> accepted(n_pairs);
  auto pass = [&] {
    for (int i = 0; i < n_pairs; i++)
      accepted[i] = cs::triangulate_pair_serial(pair[i], prm, rec.data() + (size_t)first[i] * cs::TRI_MATCH_DOUBLES, end[i] - first[i], out8.data() + (size_t)first[i] * cs::TRI_OUT_DOUBLES,
                                                status.data() + first[i], route.data() + first[i], cos3.data() + 3 * (size_t)first[i]);
  };
  const auto t0 = std::chrono::steady_clock::now();
  for (int r = 0; r < repeats; r++) pass();
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / repeats;
  if (run) {
    for (int i = 0; i < n_pairs; i++) {
      for (int m = first[i]; m < end[i]; m++) {
        std::printf("m %d %d %d", m, (int)status[m], (int)route[m]);
        for (int k = 0; k < cs::TRI_OUT_DOUBLES; k++) std::printf(" %.17g", out8[(size_t)m * cs::TRI_OUT_DOUBLES + k]);
        std::printf(" %.17g %.17g %.17g\n", cos3[3 * (size_t)m], cos3[3 * (size_t)m + 1], cos3[3 * (size_t)m + 2]);
      }
      std::printf("pair %d %d %d\n", i, pair[i].ran != 0.0 ? 1 : 0, accepted[i]);
    }
  } else {
    long total = 0;
    for (int i = 0; i < n_pairs; i++) total += accepted[i];
    std::printf("host, one core: %.4f ms per pass over %d pairs, %d matches (%ld accepted)\n", ms, n_pairs, n_matches, total);
  }
  std::printf("triangulate_host_check: ok\n");
  return 0;
}
