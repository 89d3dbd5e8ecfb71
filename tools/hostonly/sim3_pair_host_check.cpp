// sim3_pair_host_check.cpp -- cs_sim3_pair.h WITHOUT a GPU: the per-pair routine the kernel runs with 64 lanes, run here with one worker
// (cs::Sim3PairSerial) over a dumped batch, pair after pair.  tests/test_sim3_pair_ref.py builds it with g++ (once plain, once under the
// address and undefined-behaviour sanitizers), writes the dump, and compares what is printed with the numpy statement.
//
//   sim3_pair_host_check opt|lin DUMP
//
// DUMP (text, every number in %.17g): n_pairs n_matches / iterations_first iterations_more_clean iterations_more_outliers
// robust_second_round min_inliers th2 huber_delta / per pair: S (8) intr (8) fix_scale first_match end_match / per match: the 18 doubles of
// a record (cs_sim3_pair.h).
// opt prints per pair "pair f it0 it1 n_inliers chi0 chi1 S[8]" and "inl f <flags>"; lin prints per match "lin i e[4] J[28]".
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../cube_slam_wu_amd/csrc/cs_sim3_pair.h"

int main(int argc, char** argv) {
  if (argc != 3 || (std::strcmp(argv[1], "opt") && std::strcmp(argv[1], "lin"))) { std::fprintf(stderr, "usage: %s opt|lin DUMP\n", argv[0]); return 2; }
  const bool lin = !std::strcmp(argv[1], "lin");
  FILE* f = std::fopen(argv[2], "r");
  if (!f) { std::perror(argv[2]); return 2; }
  int n_pairs = 0, n_matches = 0;
  cs::Sim3PairSchedule p;
  bool ok = std::fscanf(f, "%d %d", &n_pairs, &n_matches) == 2 && n_pairs >= 0 && n_matches >= 0;
  ok = ok && std::fscanf(f, "%d %d %d %d %d %lf %lf", &p.iterations_first, &p.iterations_more_clean, &p.iterations_more_outliers, &p.robust_second_round, &p.min_inliers,
                         &p.th2, &p.huber_delta) == 7;
  if (!ok) { std::fprintf(stderr, "bad header\n"); return 2; }
  std::vector<double> S(8 * (size_t)n_pairs), intr(8 * (size_t)n_pairs), rec((size_t)cs::SIM3_PAIR_MATCH_DOUBLES * n_matches);
  std::vector<int> fix(n_pairs), first(n_pairs), end(n_pairs);
  for (int i = 0; i < n_pairs && ok; i++) {
    for (int k = 0; k < 8 && ok; k++) ok = std::fscanf(f, "%lf", &S[8 * (size_t)i + k]) == 1;
    for (int k = 0; k < 8 && ok; k++) ok = std::fscanf(f, "%lf", &intr[8 * (size_t)i + k]) == 1;
    ok = ok && std::fscanf(f, "%d %d %d", &fix[i], &first[i], &end[i]) == 3 && 0 <= first[i] && first[i] <= end[i] && end[i] <= n_matches;
  }
  for (size_t k = 0; k < rec.size() && ok; k++) ok = std::fscanf(f, "%lf", &rec[k]) == 1;
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "bad dump\n"); return 2; }

  std::vector<unsigned char> level(n_matches);
  std::vector<double> err(4 * (size_t)n_matches), jac(28 * (size_t)n_matches);
  for (int i = 0; i < n_pairs; i++) {
    cs::Sim3PairProblem F;
    F.rec = rec.data() + (size_t)first[i] * cs::SIM3_PAIR_MATCH_DOUBLES;
    F.n = end[i] - first[i];
    for (int k = 0; k < 8; k++) F.intr[k] = intr[8 * (size_t)i + k];
    F.fix_scale = fix[i] != 0;
    cs::Sim3PairSerial w;
    cs::Sim3 St = cs::sim3_load(&S[8 * (size_t)i]);
    if (lin) {
      cs::sim3_pair_inspect(w, F, St, err.data() + 4 * (size_t)first[i], jac.data() + 28 * (size_t)first[i]);
      continue;
    }
    int iters[2], n_in = 0;
    double chi[2], v[8];
    cs::sim3_pair_optimize(w, F, p, St, level.data() + first[i], iters, chi, n_in);
    cs::sim3_store(St, v);
    std::printf("pair %d %d %d %d %.17g %.17g", i, iters[0], iters[1], n_in, chi[0], chi[1]);
    for (int k = 0; k < 8; k++) std::printf(" %.17g", v[k]);
    std::printf("\ninl %d ", i);
    for (int m = first[i]; m < end[i]; m++) std::putchar(level[m] ? '1' : '0');
    std::printf("\n");
  }
  if (lin)
    for (int m = 0; m < n_matches; m++) {
      std::printf("lin %d", m);
      for (int k = 0; k < 4; k++) std::printf(" %.17g", err[4 * (size_t)m + k]);
      for (int k = 0; k < 28; k++) std::printf(" %.17g", jac[28 * (size_t)m + k]);
      std::printf("\n");
    }
  std::printf("sim3_pair_host_check: ok\n");
  return 0;
}
