// lm_policy_check -- host-only run of the Levenberg-Marquardt policy (csrc/cs_lm.h) over fixed sequences of trial results, driven the way
// cs_ba_optimize and cs_pgo_optimize drive it.  Prints what went in and what the policy made of it, doubles as hex floats;
// tests/test_lm_policy.py replays the printed inputs through the float64 transcription of g2o's loop (tests/pgo_ref.py) and compares.
//   hipcc -O2 -std=c++17 -ffp-contract=off tools/microbench/lm_policy_check.cpp -o build_tmp/lm_policy_check && build_tmp/lm_policy_check
//   seq  <name> <user lambda> <max |H_jj|> <max trials> <iterations asked for>
//   step <iteration> <currentChi in> <tempChi> <scale> <solved>  ->  <rho> <accepted> <lambda> <ni> <currentChi out>
//   iter <iteration> <trials> <currentChi> <lambda> <bad iterations> <stop>
#include "../../cube_slam_wu_amd/csrc/cs_lm.h"

#include <cstdio>
#include <vector>

namespace {

const double INF = std::numeric_limits<double>::infinity();

struct Trial { double tempChi, scale; bool solved; };
struct Iter { double currentChi; std::vector<Trial> trials; };      // (an iteration that asks for more trials than listed gets its last one again)
struct Seq { const char* name; double user_lambda, max_diag; int max_trials; std::vector<Iter> iters; };

const std::vector<Seq> SEQS = {
  // accepted trials: rho = 0.25 and 0.75 (either side of 1/2; 1 - (2 rho - 1)^3 is above 2/3 up to rho = 0.85: the upper clamp), 0.9 (between the clamps:
  // the one place where pow's value reaches lambda), 0.98 (the lower clamp, 1/3)
  {"accept", 0.0, 4.0e3, 10, {{100.0, {{75.0, 99.999, true}}}, {75.0, {{37.5, 49.999, true}}}, {37.5, {{19.5, 19.999, true}}}, {19.5, {{9.7, 9.999, true}}}}},
  // a user lambda; rejections up to max_trials: the optimisation ends there and the third iteration is never asked for
  {"reject_to_max", 0.5, 1.0, 5, {{10.0, {{9.0, 2.0, true}}}, {9.0, {{9.5, 1.0, true}, {12.0, 1.0, true}}}, {9.0, {{1.0, 1.0, true}}}}},
  // a failed factorisation: neither its chi2 nor its negative scale term (which would make rho positive) counts; then tempChi = inf from a solve
  // that went through (rho = -inf), then an accepted trial
  {"failed", 0.0, 2.5e2, 10, {{50.0, {{60.0, -5.0, false}, {40.0, -5.0, false}, {INF, 3.0, true}, {45.0, 9.999, true}}}, {45.0, {{44.0, 1.999, true}}}}},
  // tempChi = inf over a negative scale term: rho = +inf is positive but the chi2 is not finite -- rejected, and the iteration ends (rho is not < 0)
  {"inf_positive_rho", 0.0, 1.0, 10, {{50.0, {{INF, -3.0, true}}}, {50.0, {{45.0, 9.999, true}}}}},
  // a negative scale term of a solve that went through: rho < 0 although chi2 fell -- rejected, as g2o does
  {"negative_scale", 1e-3, 1.0, 3, {{8.0, {{7.0, -2.0, true}, {7.5, 0.499, true}}}}},
  // rho == 0 (chi2 unchanged): one trial, rejected, and the optimisation ends
  {"rho_zero", 0.0, 1.0, 10, {{3.0, {{3.0, 1.0, true}}}, {3.0, {{2.0, 1.0, true}}}}},
  // three iterations in a row that gain less than a thousandth end the optimisation: two of them, one good (the count starts again), three
  {"bad_iterations", 0.0, 1.0e2, 10, {{1000.0, {{999.5, 0.999, true}}}, {999.5, {{999.0, 0.999, true}}}, {999.0, {{900.0, 197.999, true}}}, {900.0, {{899.5, 0.999, true}}},
                                      {899.5, {{899.0, 0.999, true}}}, {899.0, {{898.5, 0.999, true}}}, {898.5, {{1.0, 1.0, true}}}}},
};

}  // namespace

int main() {
  for (const Seq& q : SEQS) {
    printf("seq %s %a %a %d %d\n", q.name, q.user_lambda, q.max_diag, q.max_trials, (int)q.iters.size());
    cs::LmState lm;
    for (size_t it = 0; it < q.iters.size(); it++) {
      double currentChi = q.iters[it].currentChi;
      const double iniChi = currentChi;
      if (it == 0) cs::lm_begin(lm, q.user_lambda, q.max_diag);
      double rho = 0;
      int qmax = 0;
      do {
        const Trial& t = q.iters[it].trials[std::min((size_t)qmax, q.iters[it].trials.size() - 1)];
        printf("step %d %a %a %a %d", (int)it, currentChi, t.tempChi, t.scale, t.solved ? 1 : 0);
        const bool accepted = cs::lm_trial(lm, currentChi, t.tempChi, t.scale, t.solved, rho);
        printf(" -> %a %d %a %a %a\n", rho, accepted ? 1 : 0, lm.lambda, lm.ni, currentChi);
        qmax++;
      } while (cs::lm_again(rho, qmax, q.max_trials));
      const bool stop = cs::lm_stop(lm, rho, qmax, q.max_trials, iniChi, currentChi);
      printf("iter %d %d %a %a %d %d\n", (int)it, qmax, currentChi, lm.lambda, lm.n_bad, stop ? 1 : 0);
      if (stop) break;
    }
  }
  return 0;
}
