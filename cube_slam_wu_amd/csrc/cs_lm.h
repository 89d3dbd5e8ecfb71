// cs_lm.h -- the Levenberg-Marquardt policy of g2o's OptimizationAlgorithmLevenberg::solve (core/optimization_algorithm_levenberg.cpp:61-163),
// stated once, for host and device: lambda's first value, a trial's accept / reject arithmetic, the retry and stop rules.  The host loops of
// cs_ba_optimize (ba_lm.cpp) and cs_pgo_optimize (pgo_host.cpp) call it, and so does the per-wavefront loop of cs_dense_lm.h that
// pose_kernels.hip and sim3_pair_kernels.hip run.  What a loop DOES on either verdict stays with the loop.  (Compiled with
// -ffp-contract=off, like all of them.)
#pragma once
#include <float.h>
#include <math.h>

#if defined(__HIPCC__)
#define CS_HD __host__ __device__ __forceinline__
#else
#ifndef CS_HD
#define CS_HD static inline
#endif
#endif

namespace cs {
struct LmState { double lambda = 0, ni = 2; int n_bad = 0; };   // _currentLambda, _ni, _nBad (iterations in a row that gained less than a thousandth of their chi2)
// iteration 0 (:93-97); computeLambdaInit (:166-180) with tau = 1e-5, max_diag = max |H_jj| over the free vertices; a user value wins (:168-169)
CS_HD void lm_begin(LmState& s, double user_lambda_init, double max_diag) { s = LmState{user_lambda_init > 0 ? user_lambda_init : 1e-5 * max_diag, 2, 0}; }
// One trial's verdict (:126-147): true = accepted, currentChi <- tempChi; false = rejected, the caller pops.  A failed factorisation left garbage
// in x: its chi2 counts as the largest double (:126-127) and its scale term as zero, so that a negative scale cannot turn the sign of rho.
CS_HD bool lm_trial(LmState& s, double& currentChi, double tempChi, double scale, bool solved, double& rho) {
  if (!solved) { tempChi = DBL_MAX; scale = 0.0; }
  rho = currentChi - tempChi;
  scale += 1e-3;
  rho /= scale;
  if (rho > 0 && isfinite(tempChi)) {
    double alpha = 1. - pow(2 * rho - 1, 3.0);   // (the double exponent: the same libm routine on host and device)
    alpha = fmin(alpha, 2. / 3.);                // _goodStepUpperScale  (rho > 0: alpha is no NaN, fmin / fmax are std::min / std::max)
    s.lambda *= fmax(1. / 3., alpha);            // _goodStepLowerScale
    s.ni = 2;
    currentChi = tempChi;
    return true;
  }
  s.lambda *= s.ni;
  s.ni *= 2;
  return false;
}
// another trial of the same iteration (:149)
CS_HD bool lm_again(double rho, int qmax, int max_trials) { return rho < 0 && qmax < max_trials; }
// after an iteration's last trial (:151-161): true = the optimisation ends here
CS_HD bool lm_stop(LmState& s, double rho, int qmax, int max_trials, double iniChi, double currentChi) {
  if (qmax == max_trials || rho == 0) return true;
  if ((iniChi - currentChi) * 1e3 < iniChi) s.n_bad++; else s.n_bad = 0;
  return s.n_bad >= 3;
}
}  // namespace cs
