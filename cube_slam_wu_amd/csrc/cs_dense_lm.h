// cs_dense_lm.h -- SparseOptimizer::optimize(iterations) (core/sparse_optimizer.cpp:354-419) with OptimizationAlgorithmLevenberg::solve
// (core/optimization_algorithm_levenberg.cpp:61-189) for a graph of ONE free vertex of N dimensions, for host and device: the N x N system
// goes through an LDL^T without pivoting, the policy is cs_lm.h's.  pose_kernels.hip runs it per wavefront with N = 6 (a frame's pose),
// cs_sim3_pair.h with N = 7 (a keyframe pair's Sim(3)).  Every scalar here is the same in all workers of a problem, so on the device the
// control flow never diverges.  FP64, -ffp-contract=off.
#pragma once
#include "cs_lm.h"

#if defined(__HIPCC__)
#define CS_HD_MEMBER __host__ __device__ __forceinline__      // (CS_HD is `static inline` on the host, which a member function cannot be)
#define CS_UNROLL _Pragma("unroll")      // constant trip counts: every array below has to stay in registers on the device
#define CS_NOUNROLL _Pragma("nounroll")
#else
#define CS_HD_MEMBER inline
#define CS_UNROLL
#define CS_NOUNROLL
#endif

namespace cs {

// (H + lambda I) x = b by LDL^T without pivoting, H = the N (N + 1) / 2 upper entries row by row; false when a pivot is not positive
// (LinearSolverDense's isPositive(), solvers/linear_solver_dense.h:104-111)
template <int N>
CS_HD bool ldlt_solve(const double* H, double lambda, const double* b, double* x) {
  double A[N * N], D[N], y[N];
  {
    int k = 0;
    CS_UNROLL
    for (int i = 0; i < N; i++)
      CS_UNROLL
      for (int j = i; j < N; j++, k++) { A[N * i + j] = H[k]; A[N * j + i] = H[k]; }
  }
  CS_UNROLL
  for (int i = 0; i < N; i++) A[(N + 1) * i] += lambda;
  bool ok = true;
  CS_UNROLL
  for (int j = 0; j < N; j++) {
    double d = A[(N + 1) * j];
    CS_UNROLL
    for (int k = 0; k < j; k++) d -= A[N * j + k] * A[N * j + k] * D[k];
    if (!(d > 0)) ok = false;
    D[j] = d;
    CS_UNROLL
    for (int i = j + 1; i < N; i++) {
      double s = A[N * i + j];
      CS_UNROLL
      for (int k = 0; k < j; k++) s -= A[N * i + k] * A[N * j + k] * D[k];
      A[N * i + j] = s / d;
    }
  }
  CS_UNROLL
  for (int i = 0; i < N; i++) {
    double s = b[i];
    CS_UNROLL
    for (int k = 0; k < i; k++) s -= A[N * i + k] * y[k];
    y[i] = s;
  }
  CS_UNROLL
  for (int i = 0; i < N; i++) y[i] /= D[i];
  CS_UNROLL
  for (int i = N - 1; i >= 0; i--) {
    double s = y[i];
    CS_UNROLL
    for (int k = i + 1; k < N; k++) s -= A[N * k + i] * x[k];
    x[i] = s;
  }
  return ok;
}

// optimize(iterations) from state S.  The problem P supplies
//   P.linearize(S, H, b, chi)   computeActiveErrors + buildSystem at S: H (upper entries, row by row), b and activeRobustChi2
//   P.chi2(S)                   activeRobustChi2 at S (sparse_optimizer.cpp:100-114)
//   P.oplus(S, x)               the vertex's oplusImpl
// Returns what optimize() returns, the iterations run; chi = the activeRobustChi2 of the state S ends on.  No loop is unbounded.
// Zero iterations stay a loop of no trips, not an early return: on the device the return costs the pose kernel its second wave per SIMD.
template <int N, class Problem, class State>
CS_HD int dense_lm_round(const Problem P, State& S, int iterations, int max_trials, double& chi) {
  int done = 0;
  if (iterations <= 0) chi = P.chi2(S);
  LmState lm;
  for (int it = 0; it < iterations; it++) {
    double H[N * (N + 1) / 2], b[N];
    P.linearize(S, H, b, chi);
    if (it == 0) {                                   // computeLambdaInit (:166-180) over the diagonal of the packed H
      double md = 0.0;
      int k = 0;
      CS_UNROLL
      for (int j = 0; j < N; k += N - j, j++) md = fmax(fabs(H[k]), md);
      lm_begin(lm, 0.0, md);
    }
    const double iniChi = chi;
    double rho = 0.0;
    int qmax = 0;
    do {
      double x[N];
      const bool solved = ldlt_solve<N>(H, lm.lambda, b, x);
      double tempChi = DBL_MAX, scale = 0.0;         // (what lm_trial makes of a failed factorisation; x is not looked at then)
      State Sn = S;
      if (solved) {
        Sn = P.oplus(S, x);
        tempChi = P.chi2(Sn);
        CS_UNROLL
        for (int j = 0; j < N; j++) scale += x[j] * (lm.lambda * x[j] + b[j]);      // computeScale (:182-189)
      }
      if (lm_trial(lm, chi, tempChi, scale, solved, rho)) S = Sn;
      qmax++;
    } while (lm_again(rho, qmax, max_trials));
    done++;
    if (lm_stop(lm, rho, qmax, max_trials, iniChi, chi)) break;
  }
  return done;
}

}  // namespace cs
