// cs_lm.h -- the Levenberg-Marquardt policy of g2o's OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.cpp:61-163),
// stated once for cs_ba_optimize (ba_host.cpp) and cs_pgo_optimize (pgo_host.cpp): lambda's first value, a trial's accept / reject arithmetic,
// the retry and stop rules.  Host only; what a loop DOES on either verdict stays with the loop.  (Compiled with -ffp-contract=off, like both.)
#pragma once
#include <algorithm>
#include <cmath>
#include <limits>

namespace cs {
struct LmState { double lambda = 0, ni = 2; int n_bad = 0; };   // _currentLambda, _ni, _nBad (iterations in a row that gained less than a thousandth of their chi2)
// iteration 0 (:93-97); computeLambdaInit (:166-180) with tau = 1e-5, max_diag = max |H_jj| over the free vertices; a user value wins (:168-169)
inline void lm_begin(LmState& s, double user_lambda_init, double max_diag) { s = LmState{user_lambda_init > 0 ? user_lambda_init : 1e-5 * max_diag, 2, 0}; }
// One trial's verdict (:126-147): true = accepted, currentChi <- tempChi; false = rejected, the caller pops.  A failed factorisation left garbage
// in x: its chi2 counts as the largest double (:126-127) and its scale term as zero, so that a negative scale cannot turn the sign of rho.
inline bool lm_trial(LmState& s, double& currentChi, double tempChi, double scale, bool solved, double& rho) {
  if (!solved) { tempChi = std::numeric_limits<double>::max(); scale = 0.0; }
  rho = currentChi - tempChi;
  scale += 1e-3;
  rho /= scale;
  if (rho > 0 && std::isfinite(tempChi)) {
    double alpha = 1. - std::pow((2 * rho - 1), 3);
    alpha = std::min(alpha, 2. / 3.);          // _goodStepUpperScale
    s.lambda *= std::max(1. / 3., alpha);      // _goodStepLowerScale
    s.ni = 2;
    currentChi = tempChi;
    return true;
  }
  s.lambda *= s.ni;
  s.ni *= 2;
  return false;
}
// another trial of the same iteration (:149)
inline bool lm_again(double rho, int qmax, int max_trials) { return rho < 0 && qmax < max_trials; }
// after an iteration's last trial (:151-161): true = the optimisation ends here
inline bool lm_stop(LmState& s, double rho, int qmax, int max_trials, double iniChi, double currentChi) {
  if (qmax == max_trials || rho == 0) return true;
  if ((iniChi - currentChi) * 1e3 < iniChi) s.n_bad++; else s.n_bad = 0;
  return s.n_bad >= 3;
}
}  // namespace cs
