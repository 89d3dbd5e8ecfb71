// sim3_ransac_host_check.cpp -- cs_sim3_ransac.h WITHOUT a GPU: the routines the kernel runs with one hypothesis per lane, run here by a
// serial worker (cs::sim3_ransac_pair_serial: one hypothesis after the other, the selection as it is stated) over a dumped batch, pair
// after pair.  tests/test_sim3_ransac_ref.py builds it with g++ (once plain, once under the address and undefined-behaviour sanitizers),
// writes the dump, and compares what is printed with the numpy statement.
//
//   sim3_ransac_host_check run DUMP            per pair "pair f found hyp iterations n_inliers S12[8]" and "inl f <flags>"
//   sim3_ransac_host_check hyp N_HYP DUMP      per pair and hypothesis "hyp f h count S12[8]" (a refused one: -1 and the identity)
//   sim3_ransac_host_check time REPEATS DUMP   run, REPEATS times, and the time of one pass over the batch in ms (one core)
//
// DUMP (text, every double in %.17g): n_pairs n_matches / probability min_inliers max_iterations / per pair: intr (8) fix_scale seed
// first_match end_match / per match: the 8 doubles of a packed record (cs_sim3_ransac.h).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cube_slam_wu_amd/csrc/cs_sim3_ransac.h"

int main(int argc, char** argv) {
  const bool run = argc == 3 && !std::strcmp(argv[1], "run");
  const bool hyp = argc == 4 && !std::strcmp(argv[1], "hyp");
  const bool timed = argc == 4 && !std::strcmp(argv[1], "time");
  if (!run && !hyp && !timed) { std::fprintf(stderr, "usage: %s run DUMP | hyp N_HYP DUMP | time REPEATS DUMP\n", argv[0]); return 2; }
  const int count_arg = run ? 0 : std::atoi(argv[2]);
  if (!run && (count_arg < 1 || count_arg > (hyp ? (int)cs::SIM3_RANSAC_MAX_ITERATIONS : 1000000))) { std::fprintf(stderr, "bad count\n"); return 2; }
  const char* path = argv[run ? 2 : 3];
  FILE* f = std::fopen(path, "r");
  if (!f) { std::perror(path); return 2; }
  int n_pairs = 0, n_matches = 0, min_inliers = 0, max_iterations = 0;
  double probability = 0;
  bool ok = std::fscanf(f, "%d %d", &n_pairs, &n_matches) == 2 && n_pairs >= 0 && n_matches >= 0;
  ok = ok && std::fscanf(f, "%lf %d %d", &probability, &min_inliers, &max_iterations) == 3 && probability > 0 && probability < 1 && min_inliers >= 0 &&
       max_iterations >= 1 && max_iterations <= cs::SIM3_RANSAC_MAX_ITERATIONS;
  if (!ok) { std::fprintf(stderr, "bad header\n"); return 2; }
  std::vector<double> intr(8 * (size_t)n_pairs), rec((size_t)cs::SIM3_RANSAC_MATCH_DOUBLES * n_matches);
  std::vector<int> fix(n_pairs), first(n_pairs), end(n_pairs);
  std::vector<unsigned long long> seed(n_pairs);
  for (int i = 0; i < n_pairs && ok; i++) {
    for (int k = 0; k < 8 && ok; k++) ok = std::fscanf(f, "%lf", &intr[8 * (size_t)i + k]) == 1;
    ok = ok && std::fscanf(f, "%d %llu %d %d", &fix[i], &seed[i], &first[i], &end[i]) == 4 && 0 <= first[i] && first[i] <= end[i] && end[i] <= n_matches;
  }
  for (size_t k = 0; k < rec.size() && ok; k++) ok = std::fscanf(f, "%lf", &rec[k]) == 1;
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "bad dump\n"); return 2; }

  std::vector<unsigned char> flags(n_matches);
  std::vector<cs::Sim3RansacResult> res(n_pairs);
  auto pass = [&] {
    for (int i = 0; i < n_pairs; i++) {
      const int n = end[i] - first[i];
      const int max_its = cs::sim3_ransac_budget(n, probability, min_inliers, max_iterations);
      res[i] = cs::sim3_ransac_pair_serial(rec.data() + (size_t)first[i] * cs::SIM3_RANSAC_MATCH_DOUBLES, n, &intr[8 * (size_t)i], fix[i] != 0, seed[i], min_inliers, max_its,
                                           flags.data() + first[i]);
    }
  };
  if (hyp) {
    for (int i = 0; i < n_pairs; i++) {
      const int n = end[i] - first[i];
      for (int h = 0; h < count_arg; h++) {
        cs::Sim3RansacHyp H;
        cs::Sim3RansacResult none;
        cs::sim3_ransac_result_init(none, 0);
        int count = -1;
        const bool valid = n >= 3 && cs::sim3_ransac_evaluate(rec.data() + (size_t)first[i] * cs::SIM3_RANSAC_MATCH_DOUBLES, n, &intr[8 * (size_t)i], fix[i] != 0, seed[i], h, H, count);
        if (valid) cs::sim3_ransac_store(H, none.S12);
        std::printf("hyp %d %d %d", i, h, valid ? count : -1);
        for (int k = 0; k < 8; k++) std::printf(" %.17g", none.S12[k]);
        std::printf("\n");
      }
    }
  } else {
    const int repeats = timed ? count_arg : 1;
    const auto t0 = std::chrono::steady_clock::now();
    for (int r = 0; r < repeats; r++) pass();
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count() / repeats;
    for (int i = 0; i < n_pairs && run; i++) {
      std::printf("pair %d %d %d %d %d", i, res[i].found, res[i].hyp, res[i].iterations, res[i].n_inliers);
      for (int k = 0; k < 8; k++) std::printf(" %.17g", res[i].S12[k]);
      std::printf("\ninl %d ", i);
      for (int m = first[i]; m < end[i]; m++) std::putchar(flags[m] ? '1' : '0');
      std::printf("\n");
    }
    if (timed) {
      long found = 0, its = 0;
      for (int i = 0; i < n_pairs; i++) { found += res[i].found; its += res[i].iterations; }
      std::printf("host, one core: %.3f ms per pass over %d pairs (%ld found, %ld hypotheses up to the winners)\n", ms, n_pairs, found, its);
    }
  }
  std::printf("sim3_ransac_host_check: ok\n");
  return 0;
}
