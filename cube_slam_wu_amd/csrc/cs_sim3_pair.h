// cs_sim3_pair.h -- Sim(3) alignment of one keyframe pair, for host and device (include/cubeslam_hip.h: cs_sim3_*).
//
// One pair is a g2o graph of ONE free VertexSim3Expmap (types/types_seven_dof_expmap.h:48-94, cam_map1 / cam_map2 :74-88) and, per match,
// two binary edges whose other vertex is a FIXED VertexSBAPointXYZ:
//   EdgeSim3ProjectXYZ          :130-149   e12 = obs1 - cam_map1(project(S.map(P2)))
//   EdgeInverseSim3ProjectXYZ   :152-171   e21 = obs2 - cam_map2(project(S^-1.map(P1)))
// Both have linearizeOplus commented out (:147, :169): the Jacobian is BaseBinaryEdge's numeric default (core/base_binary_edge.hpp:130-205),
// central differences with delta = 1e-9 through VertexSim3Expmap::oplusImpl (cs_sim3.h: sim3_oplus).  The quadratic form is
// BaseBinaryEdge::constructQuadraticForm's (:55-120) with the point fixed, the kernel RobustKernelHuber (cs_robust.h), the optimiser
// cs_dense_lm.h's dense_lm_round with N = 7: OptimizationAlgorithmLevenberg in the policy of cs_lm.h over a 7 x 7 LDL^T, the loop
// pose_kernels.hip runs with N = 6.  The two-round schedule with the classification between the rounds is ORB-SLAM2's
// Optimizer::OptimizeSim3, which is NOT IN THE REFERENCE.
//
// sim3_pair_optimize is written over a "wave" W: `lane` of `stride` workers share a pair's matches (worker l owns matches l, l + stride,
// ...), W::sum adds one value per worker and hands every worker the same total, W::load reads a match record, W::put / W::get / W::sync publish the 15 states of a
// linearisation (W::reread, once per match: the states are read again, not kept in registers over the loop).  sim3_pair_kernels.hip runs it with 64 lanes, a butterfly and LDS; tools/hostonly/sim3_pair_host_check.cpp with one
// worker and an array.  FP64, -ffp-contract=off.
#pragma once
#include "cs_dense_lm.h"
#include "cs_robust.h"
#include "cs_sim3.h"

namespace cs {

// One match as the kernel reads it: 18 doubles = 144 bytes, a multiple of 16.
//   [0..2] P1 (the point in camera 1)   [3..5] P2 (in camera 2)   [6..7] obs1   [8..9] obs2   [10..13] info12   [14..17] info21 (row-major 2 x 2)
enum { SIM3_PAIR_MATCH_DOUBLES = 18, SIM3_PAIR_STATES = 15, SIM3_PAIR_STATE_DOUBLES = 16, SIM3_PAIR_MAX_ITERATIONS = 100, SIM3_PAIR_MAX_TRIALS = 10 };

constexpr double SIM3_PAIR_DELTA = 1e-9;      // base_binary_edge.hpp:147

struct Sim3PairMatch {
  double P1[3], P2[3], o1[2], o2[2], W12[4], W21[4];
};

CS_HD Sim3PairMatch sim3_pair_match(const double* v) {
  Sim3PairMatch m;
  CS_UNROLL
  for (int k = 0; k < 3; k++) { m.P1[k] = v[k]; m.P2[k] = v[3 + k]; }
  CS_UNROLL
  for (int k = 0; k < 2; k++) { m.o1[k] = v[6 + k]; m.o2[k] = v[8 + k]; }
  CS_UNROLL
  for (int k = 0; k < 4; k++) { m.W12[k] = v[10 + k]; m.W21[k] = v[14 + k]; }
  return m;
}

// match i of the pair; W::load reads the record's 18 doubles (the device: as aligned double2s)
template <class W, class F_>
CS_HD Sim3PairMatch sim3_pair_load(const W& w, const F_& F, int i) {
  double v[SIM3_PAIR_MATCH_DOUBLES];
  w.load(F.rec + (size_t)i * SIM3_PAIR_MATCH_DOUBLES, v);
  return sim3_pair_match(v);
}

struct Sim3PairSchedule {      // cs_sim3_pair_params
  int iterations_first, iterations_more_clean, iterations_more_outliers;
  int robust_second_round, min_inliers;
  double th2, huber_delta;
};

struct Sim3PairProblem {
  const double* rec;           // the pair's first match record
  int n;
  double intr[8];              // fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2
  bool fix_scale;
};

// obs - cam_map(project(T.map(P))): project divides by the depth (types_six_dof_expmap.h project2d), cam_map is v * f + c.
// intr4 = fx fy cx cy of the camera the point is projected into; T is S for e12 and S^-1 for e21.
CS_HD void sim3_pair_edge_error(const Sim3& T, const double* P, const double* obs, const double* intr4, double* e) {
  double pc[3];
  sim3_map(T, P, pc);
  e[0] = obs[0] - (pc[0] / pc[2] * intr4[0] + intr4[2]);
  e[1] = obs[1] - (pc[1] / pc[2] * intr4[1] + intr4[3]);
}

// e^T Omega e (BaseEdge::chi2) and Omega e
CS_HD double sim3_pair_chi2(const double* W, const double* e, double* We) {
  We[0] = W[0] * e[0] + W[1] * e[1];
  We[1] = W[2] * e[0] + W[3] * e[1];
  return e[0] * We[0] + e[1] * We[1];
}

// A state as it is published: S (8 doubles, Sim3::operator[] order) and S^-1 (8 more).
CS_HD void sim3_pair_state_pack(const Sim3& S, double* v) { sim3_store(S, v); sim3_store(sim3_inv(S), v + 8); }

// State k of a linearisation: 0 = S itself; 1 + 2 d = S (+) delta e_d; 2 + 2 d = S (+) -delta e_d (base_binary_edge.hpp:181-194).
// Under fix_scale the two states of d = 6 are the same bits (oplusImpl zeroes update[6]), hence a seventh column of exact zeros.
CS_HD Sim3 sim3_pair_state(const Sim3& S, int k, bool fix_scale) {
  if (k == 0) return S;
  const int d = (k - 1) >> 1;
  const double step = ((k - 1) & 1) ? -SIM3_PAIR_DELTA : SIM3_PAIR_DELTA;
  double u[7];
  CS_UNROLL
  for (int i = 0; i < 7; i++) u[i] = (i == d) ? step : 0.0;
  return sim3_oplus(S, u, fix_scale);
}

// One edge's numeric Jacobian from the 14 published perturbed states: column d = (e(+delta e_d) - e(-delta e_d)) * (1 / (2 delta)).
// `inverse` picks S^-1 (EdgeInverseSim3ProjectXYZ).  J is 2 x 7, row-major.
template <class W>
CS_HD void sim3_pair_edge_jacobian(const W& w, bool inverse, const double* P, const double* obs, const double* intr4, double* J) {
  const double scalar = 1.0 / (2 * SIM3_PAIR_DELTA);
  // The seven dimensions stay a loop (unrolled, their 14 projections in flight at once take more registers than the device has); column d
  // is put in its place by selects, so that J needs no indexed storage.
  CS_UNROLL
  for (int k = 0; k < 14; k++) J[k] = 0.0;
  CS_NOUNROLL
  for (int d = 0; d < 7; d++) {
    double ep[2], em[2];
    sim3_pair_edge_error(sim3_load(w.get(1 + 2 * d) + (inverse ? 8 : 0)), P, obs, intr4, ep);
    sim3_pair_edge_error(sim3_load(w.get(2 + 2 * d) + (inverse ? 8 : 0)), P, obs, intr4, em);
    const double c0 = scalar * (ep[0] - em[0]), c1 = scalar * (ep[1] - em[1]);
    CS_UNROLL
    for (int k = 0; k < 7; k++) { J[k] = (k == d) ? c0 : J[k]; J[7 + k] = (k == d) ? c1 : J[7 + k]; }
  }
}

// constructQuadraticForm for the free vertex (base_binary_edge.hpp:87-113; without a kernel rho' = 1):
//   b -= rho' J^T Omega e,  H += J^T (rho' Omega) J;   h = the 28 upper entries row by row, We = Omega e
CS_HD void sim3_pair_quadratic_form(const double* J, const double* Wm, const double* We, double r1, double* h, double* g) {
  double WJ[14];
  CS_UNROLL
  for (int a = 0; a < 7; a++) {
    WJ[a] = r1 * (Wm[0] * J[a] + Wm[1] * J[7 + a]);
    WJ[7 + a] = r1 * (Wm[2] * J[a] + Wm[3] * J[7 + a]);
  }
  int k = 0;
  CS_UNROLL
  for (int a = 0; a < 7; a++) {
    g[a] -= r1 * (J[a] * We[0] + J[7 + a] * We[1]);
    CS_UNROLL
    for (int c = a; c < 7; c++, k++) h[k] += J[a] * WJ[c] + J[7 + a] * WJ[7 + c];
  }
}

// The 15 states of a linearisation at S, one per worker, published through W.
template <class W>
CS_HD void sim3_pair_publish_states(W& w, const Sim3& S, bool fix_scale) {
  w.sync();                                            // the readers of the previous linearisation are done
  for (int k = w.lane; k < SIM3_PAIR_STATES; k += w.stride) {
    double v[SIM3_PAIR_STATE_DOUBLES];
    sim3_pair_state_pack(sim3_pair_state(S, k, fix_scale), v);
    w.put(k, v);
  }
  w.sync();
}

// Both plain chi2 of a match at (S, S^-1)
CS_HD void sim3_pair_match_chi2(const Sim3PairProblem& F, const Sim3PairMatch& m, const Sim3& S, const Sim3& Si, double& c12, double& c21) {
  double e[2], We[2];
  sim3_pair_edge_error(S, m.P2, m.o1, F.intr, e);
  c12 = sim3_pair_chi2(m.W12, e, We);
  sim3_pair_edge_error(Si, m.P1, m.o2, F.intr + 4, e);
  c21 = sim3_pair_chi2(m.W21, e, We);
}

// activeRobustChi2 at S over the pair's active matches (sparse_optimizer.cpp:100-114)
template <class W>
CS_HD double sim3_pair_active_chi2(const W& w, const Sim3PairProblem& F, const unsigned char* level, const Sim3& S, double huber) {
  const Sim3 Si = sim3_inv(S);
  double acc = 0.0;
  for (int i = w.lane; i < F.n; i += w.stride) {
    if (!level[i]) continue;
    const Sim3PairMatch m = sim3_pair_load(w, F, i);
    double c12, c21, r0, r1;
    sim3_pair_match_chi2(F, m, S, Si, c12, c21);
    huber_rho(c12, huber, r0, r1); acc += r0;
    huber_rho(c21, huber, r0, r1); acc += r0;
  }
  return w.sum(acc);
}

// computeActiveErrors + linearizeOplus + constructQuadraticForm of every active edge: H (28 upper entries, row by row), b, chi2
template <class W>
CS_HD void sim3_pair_linearize(W& w, const Sim3PairProblem& F, const unsigned char* level, const Sim3& S, double huber, double* H, double* b, double& chi) {
  sim3_pair_publish_states(w, S, F.fix_scale);
  const Sim3 S0 = sim3_load(w.get(0)), S0i = sim3_load(w.get(0) + 8);
  double h[28], g[7], acc = 0.0;
  CS_UNROLL
  for (int k = 0; k < 28; k++) h[k] = 0.0;
  CS_UNROLL
  for (int k = 0; k < 7; k++) g[k] = 0.0;
  for (int i = w.lane; i < F.n; i += w.stride) {
    if (!level[i]) continue;
    w.reread();
    const Sim3PairMatch m = sim3_pair_load(w, F, i);
    double e[2], We[2], J[14], r0, r1;
    sim3_pair_edge_error(S0, m.P2, m.o1, F.intr, e);
    huber_rho(sim3_pair_chi2(m.W12, e, We), huber, r0, r1); acc += r0;
    sim3_pair_edge_jacobian(w, false, m.P2, m.o1, F.intr, J);
    sim3_pair_quadratic_form(J, m.W12, We, r1, h, g);
    sim3_pair_edge_error(S0i, m.P1, m.o2, F.intr + 4, e);
    huber_rho(sim3_pair_chi2(m.W21, e, We), huber, r0, r1); acc += r0;
    sim3_pair_edge_jacobian(w, true, m.P1, m.o2, F.intr + 4, J);
    sim3_pair_quadratic_form(J, m.W21, We, r1, h, g);
  }
  CS_UNROLL
  for (int k = 0; k < 28; k++) H[k] = w.sum(h[k]);
  CS_UNROLL
  for (int k = 0; k < 7; k++) b[k] = w.sum(g[k]);
  chi = w.sum(acc);
}

// Inspection (cs_sim3_pairs_linearize): what computeError + linearizeOplus leave in _error and _jacobianOplusXj of every match's two edges
// at S.  err = n x 4 (e12, e21), jac = n x 2 x 2 x 7 (edge, row, column).
template <class W>
CS_HD void sim3_pair_inspect(W& w, const Sim3PairProblem& F, const Sim3& S, double* err, double* jac) {
  sim3_pair_publish_states(w, S, F.fix_scale);
  const Sim3 S0 = sim3_load(w.get(0)), S0i = sim3_load(w.get(0) + 8);
  for (int i = w.lane; i < F.n; i += w.stride) {
    w.reread();
    const Sim3PairMatch m = sim3_pair_load(w, F, i);
    double e[2], J[14];
    sim3_pair_edge_error(S0, m.P2, m.o1, F.intr, e);
    err[4 * (size_t)i] = e[0]; err[4 * (size_t)i + 1] = e[1];
    sim3_pair_edge_jacobian(w, false, m.P2, m.o1, F.intr, J);
    CS_UNROLL
    for (int k = 0; k < 14; k++) jac[28 * (size_t)i + k] = J[k];
    sim3_pair_edge_error(S0i, m.P1, m.o2, F.intr + 4, e);
    err[4 * (size_t)i + 2] = e[0]; err[4 * (size_t)i + 3] = e[1];
    sim3_pair_edge_jacobian(w, true, m.P1, m.o2, F.intr + 4, J);
    CS_UNROLL
    for (int k = 0; k < 14; k++) jac[28 * (size_t)i + 14 + k] = J[k];
  }
}

// The pair as cs_dense_lm.h's problem: one free VertexSim3Expmap under the pair's active matches
template <class W>
struct Sim3PairLm {
  W& w;
  const Sim3PairProblem& F;
  const unsigned char* level;
  double huber;
  CS_HD_MEMBER void linearize(const Sim3& S, double* H, double* b, double& chi) const { sim3_pair_linearize(w, F, level, S, huber, H, b, chi); }
  CS_HD_MEMBER double chi2(const Sim3& S) const { return sim3_pair_active_chi2(w, F, level, S, huber); }
  CS_HD_MEMBER Sim3 oplus(const Sim3& S, const double* x) const { return sim3_oplus(S, x, F.fix_scale); }
};

// optimize(iterations) on the pair's active matches, from S (cs_dense_lm.h).  iterations <= SIM3_PAIR_MAX_ITERATIONS: the host refuses more.
template <class W>
CS_HD int sim3_pair_round(W& w, const Sim3PairProblem& F, const unsigned char* level, Sim3& S, double huber, int iterations, double& currentChi) {
  return dense_lm_round<7>(Sim3PairLm<W>{w, F, level, huber}, S, iterations, SIM3_PAIR_MAX_TRIALS, currentChi);
}

// The classification between and after the rounds: an active match with e^T Omega e > th2 on either edge loses both edges
// (optimizer.removeEdge on both); a removed match is not looked at again.  Evaluated at S.  Returns the matches left.
template <class W>
CS_HD int sim3_pair_classify(const W& w, const Sim3PairProblem& F, unsigned char* level, const Sim3& S, double th2) {
  const Sim3 Si = sim3_inv(S);
  int left = 0;
  for (int i = w.lane; i < F.n; i += w.stride) {
    if (!level[i]) continue;
    const Sim3PairMatch m = sim3_pair_load(w, F, i);
    double c12, c21;
    sim3_pair_match_chi2(F, m, S, Si, c12, c21);
    const unsigned char in = (c12 > th2 || c21 > th2) ? 0 : 1;
    level[i] = in;
    left += in;
  }
  return w.sum(left);
}

// ORB-SLAM2's Optimizer::OptimizeSim3 (NOT IN THE REFERENCE) for one pair: optimize(iterations_first), classify, then
// optimize(iterations_more_outliers or iterations_more_clean) from the state the first round ended on, classify again.  `level` is one
// byte per match, written by the worker that owns the match and read back by it alone; on return it holds the inlier flags.
template <class W>
CS_HD void sim3_pair_optimize(W& w, const Sim3PairProblem& F, const Sim3PairSchedule& p, Sim3& S, unsigned char* level, int* iters2, double* chi2, int& n_inliers) {
  for (int i = w.lane; i < F.n; i += w.stride) level[i] = 1;
  iters2[0] = iters2[1] = 0;
  chi2[0] = chi2[1] = 0.0;
  int left = F.n;                                      // matches still in the graph
  for (int r = 0; r < 2; r++) {
    const double huber = (r == 0 || p.robust_second_round) ? p.huber_delta : 0.0;
    const int iterations = r == 0 ? p.iterations_first : (left < F.n ? p.iterations_more_outliers : p.iterations_more_clean);
    if (left > 0) iters2[r] = sim3_pair_round(w, F, level, S, huber, iterations, chi2[r]);
    left = sim3_pair_classify(w, F, level, S, p.th2);
    if (r == 0 && left < p.min_inliers) {              // `if (nCorrespondences - nBad < 10) return 0;`
      for (int i = w.lane; i < F.n; i += w.stride) level[i] = 0;
      left = 0;
      break;
    }
  }
  n_inliers = left;
}

// One worker, the states in an array: the sequential form (tools/hostonly/sim3_pair_host_check.cpp, and the statement the kernel is read against).
struct Sim3PairSerial {
  int lane = 0, stride = 1;
  double st[SIM3_PAIR_STATES * SIM3_PAIR_STATE_DOUBLES];
  double sum(double v) const { return v; }
  int sum(int v) const { return v; }
  void put(int k, const double* v) { for (int j = 0; j < SIM3_PAIR_STATE_DOUBLES; j++) st[SIM3_PAIR_STATE_DOUBLES * k + j] = v[j]; }
  const double* get(int k) const { return st + SIM3_PAIR_STATE_DOUBLES * k; }
  void load(const double* rec, double* v) const { for (int j = 0; j < SIM3_PAIR_MATCH_DOUBLES; j++) v[j] = rec[j]; }
  void sync() {}
  void reread() const {}
};

}  // namespace cs
