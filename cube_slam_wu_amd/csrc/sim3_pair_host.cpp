// sim3_pair_host.cpp -- the C ABI of the batched Sim(3) alignment of keyframe pairs (include/cubeslam_hip.h: cs_sim3_*).
//
// What an ORB-SLAM2-derived loop closer does once per loop candidate with g2o -- one free VertexSim3Expmap, per match an
// EdgeSim3ProjectXYZ and an EdgeInverseSim3ProjectXYZ against fixed points (types/types_seven_dof_expmap.h:48-171), two optimize() rounds
// with a classification between them -- for many pairs in ONE kernel launch (sim3_pair_kernels.hip).  The host checks every argument,
// packs the matches into 144-byte records, uploads everything with one copy, launches, and downloads everything with one copy.
// There is no CPU fallback.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/cubeslam_hip.h"
#include "cs_batch_handle.h"
#include "sim3_pair_types.h"

// d_in = [S0 | intr | records | match_ptr | fix_scale], d_out = [S_out | chi2 | iterations | n_inliers | inlier] or [err | jac]
struct cs_sim3_pairs : cs::BatchHandle {};

namespace {

bool all_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

int check_params(const cs_sim3_pair_params* p) {
  if (!p) { cs_set_error("cs_sim3: NULL parameters"); return CS_ERR_INVALID_ARG; }
  const int its[3] = {p->iterations_first, p->iterations_more_clean, p->iterations_more_outliers};
  for (int k = 0; k < 3; k++)
    if (its[k] < 0 || its[k] > cs::SIM3_PAIR_MAX_ITERATIONS) { cs_set_error("cs_sim3: an iteration count must be 0..100"); return CS_ERR_INVALID_ARG; }
  if (!std::isfinite(p->th2) || !std::isfinite(p->huber_delta)) { cs_set_error("cs_sim3: th2 / huber_delta not finite"); return CS_ERR_INVALID_ARG; }
  return CS_OK;
}

// What both entries check before anything is launched.  *n_matches = match_ptr[n_pairs].
int check_pairs(const char* who, int n_pairs, const double* S12_in, const double* intr8, const unsigned char* fix_scale, const int* match_ptr,
                const double* P1, const double* P2, const double* obs1, const double* obs2, const double* info12, const double* info21, size_t* n_matches) {
  auto fail = [&](const char* what) { cs_set_error((std::string(who) + ": " + what).c_str()); return CS_ERR_INVALID_ARG; };
  if (!S12_in || !intr8 || !fix_scale || !match_ptr) return fail("NULL argument");
  if (int rc = cs::check_partition(std::string(who) + ": match_ptr", match_ptr, n_pairs)) return rc;
  const size_t n = (size_t)match_ptr[n_pairs];
  if (n > (size_t)INT_MAX / 28) return fail("too many matches for one call");      // every index the kernel forms, the Jacobians' included, fits an int
  if (n > 0 && (!P1 || !P2 || !obs1 || !obs2)) return fail("NULL match array");
  if (!all_finite(S12_in, 8 * (size_t)n_pairs) || !all_finite(intr8, 8 * (size_t)n_pairs)) return fail("a state or an intrinsic is not finite");
  for (int f = 0; f < n_pairs; f++)
    if (!(S12_in[8 * (size_t)f + 7] > 0)) return fail("a scale is not positive");
  if (!all_finite(P1, 3 * n) || !all_finite(P2, 3 * n) || !all_finite(obs1, 2 * n) || !all_finite(obs2, 2 * n)) return fail("a point or a keypoint is not finite");
  if ((info12 && !all_finite(info12, 4 * n)) || (info21 && !all_finite(info21, 4 * n))) return fail("an information matrix is not finite");
  *n_matches = n;
  return CS_OK;
}

struct InLayout { size_t S, intr, rec, ptr, fs, bytes; };

InLayout in_layout(size_t np, size_t n) {
  cs::Layout in;
  InLayout L;
  L.S = in.add(8 * np * 8);
  L.intr = in.add(8 * np * 8);
  L.rec = in.add(n * cs::SIM3_PAIR_MATCH_DOUBLES * 8);
  L.ptr = in.add((np + 1) * 4);
  L.fs = in.add(np);
  L.bytes = in.bytes;
  return L;
}

void pack_inputs(unsigned char* h, const InLayout& L, size_t np, size_t n, const double* S12_in, const double* intr8, const unsigned char* fix_scale, const int* match_ptr,
                 const double* P1, const double* P2, const double* obs1, const double* obs2, const double* info12, const double* info21) {
  std::memcpy(h + L.S, S12_in, 8 * np * 8);
  std::memcpy(h + L.intr, intr8, 8 * np * 8);
  std::memcpy(h + L.ptr, match_ptr, (np + 1) * 4);
  std::memcpy(h + L.fs, fix_scale, np);
  double* rec = reinterpret_cast<double*>(h + L.rec);
  for (size_t i = 0; i < n; i++, rec += cs::SIM3_PAIR_MATCH_DOUBLES) {
    for (int k = 0; k < 3; k++) { rec[k] = P1[3 * i + k]; rec[3 + k] = P2[3 * i + k]; }
    for (int k = 0; k < 2; k++) { rec[6 + k] = obs1[2 * i + k]; rec[8 + k] = obs2[2 * i + k]; }
    for (int k = 0; k < 4; k++) {
      const double id = (k == 0 || k == 3) ? 1.0 : 0.0;
      rec[10 + k] = info12 ? info12[4 * i + k] : id;
      rec[14 + k] = info21 ? info21[4 * i + k] : id;
    }
  }
}

void set_inputs(cs::Sim3PairLaunch& a, unsigned char* d, const InLayout& L, int n_pairs) {
  std::memset(&a, 0, sizeof(a));
  a.n_pairs = n_pairs;
  a.S0 = reinterpret_cast<const double*>(d + L.S);
  a.intr = reinterpret_cast<const double*>(d + L.intr);
  a.rec = reinterpret_cast<const double*>(d + L.rec);
  a.match_ptr = reinterpret_cast<const int*>(d + L.ptr);
  a.fix_scale = d + L.fs;
}

}  // namespace

extern "C" {

void cs_sim3_pair_default_params(cs_sim3_pair_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->iterations_first = 5;
  p->iterations_more_clean = 5;
  p->iterations_more_outliers = 10;
  p->th2 = 10.0;
  p->huber_delta = std::sqrt(10.0);
  p->robust_second_round = 1;
  p->min_inliers = 10;
}

int cs_sim3_pairs_create(int device, cs_sim3_pairs** out) { return cs::batch_create(device, out); }

void cs_sim3_pairs_destroy(cs_sim3_pairs* B) { cs::batch_destroy(B); }

int cs_sim3_pairs_optimize(cs_sim3_pairs* B, const cs_sim3_pair_params* p, int n_pairs, const double* S12_in, const double* intr8, const unsigned char* fix_scale,
                           const int* match_ptr, const double* P1, const double* P2, const double* obs1, const double* obs2, const double* info12, const double* info21,
                           double* S12_out, unsigned char* inlier_out, int* n_inliers_out, double* chi2_out, int* iterations_done) {
  if (!B || n_pairs < 0) { cs_set_error("cs_sim3_pairs_optimize: no handle or a negative pair count"); return CS_ERR_INVALID_ARG; }
  int rc = check_params(p); if (rc) return rc;
  if (n_pairs == 0) { B->kernel_ms = B->host_ms = 0; B->ran = true; return CS_OK; }
  const double t_begin = cs::now_ms();
  size_t n = 0;
  rc = check_pairs("cs_sim3_pairs_optimize", n_pairs, S12_in, intr8, fix_scale, match_ptr, P1, P2, obs1, obs2, info12, info21, &n); if (rc) return rc;
  if (!S12_out || !n_inliers_out || (n > 0 && !inlier_out)) { cs_set_error("cs_sim3_pairs_optimize: NULL output"); return CS_ERR_INVALID_ARG; }
  B->ran = false;                                      // (a refused call leaves the last run's timing in place; one that fails from here on does not)
  const size_t np = (size_t)n_pairs;

  // ---- layout of the two buffers
  const InLayout L = in_layout(np, n);
  cs::Layout out;
  const size_t out_S = out.add(8 * np * 8), out_chi = out.add(2 * np * 8), out_it = out.add(2 * np * 4), out_ni = out.add(np * 4), out_lv = out.add(n);

  cs::Sim3PairLaunch a;
  auto pack = [&] {
    pack_inputs(B->h_in.p, L, np, n, S12_in, intr8, fix_scale, match_ptr, P1, P2, obs1, obs2, info12, info21);
    set_inputs(a, B->d_in.p, L, n_pairs);
    a.sched.iterations_first = p->iterations_first; a.sched.iterations_more_clean = p->iterations_more_clean; a.sched.iterations_more_outliers = p->iterations_more_outliers;
    a.sched.robust_second_round = p->robust_second_round ? 1 : 0; a.sched.min_inliers = p->min_inliers;
    a.sched.th2 = p->th2; a.sched.huber_delta = p->huber_delta;
    a.S_out = reinterpret_cast<double*>(B->d_out.p + out_S);
    a.chi2_out = reinterpret_cast<double*>(B->d_out.p + out_chi);
    a.iters_out = reinterpret_cast<int*>(B->d_out.p + out_it);
    a.n_inliers = reinterpret_cast<int*>(B->d_out.p + out_ni);
    a.inlier = B->d_out.p + out_lv;
  };
  rc = cs::batch_round_trip(*B, L.bytes, out.bytes, true, pack, [&] { cs::sim3_pair_launch(a, B->st); }); if (rc) return rc;

  std::memcpy(S12_out, B->h_out.p + out_S, 8 * np * 8);
  if (chi2_out) std::memcpy(chi2_out, B->h_out.p + out_chi, 2 * np * 8);
  if (iterations_done) std::memcpy(iterations_done, B->h_out.p + out_it, 2 * np * 4);
  std::memcpy(n_inliers_out, B->h_out.p + out_ni, np * 4);
  if (n) std::memcpy(inlier_out, B->h_out.p + out_lv, n);
  B->host_ms = cs::now_ms() - t_begin;
  B->ran = true;
  return CS_OK;
}

int cs_sim3_pairs_last_timing(const cs_sim3_pairs* B, double* kernel_ms, double* host_ms) { return cs::batch_last_timing(B, kernel_ms, host_ms); }

int cs_sim3_optimize_pairs(int device, const cs_sim3_pair_params* p, int n_pairs, const double* S12_in, const double* intr8, const unsigned char* fix_scale,
                           const int* match_ptr, const double* P1, const double* P2, const double* obs1, const double* obs2, const double* info12, const double* info21,
                           double* S12_out, unsigned char* inlier_out, int* n_inliers_out, double* chi2_out, int* iterations_done) {
  if (n_pairs < 0) { cs_set_error("cs_sim3_optimize_pairs: a negative pair count"); return CS_ERR_INVALID_ARG; }
  cs_sim3_pairs* B = nullptr;
  int rc = cs_sim3_pairs_create(device, &B);
  if (rc) return rc;
  rc = cs_sim3_pairs_optimize(B, p, n_pairs, S12_in, intr8, fix_scale, match_ptr, P1, P2, obs1, obs2, info12, info21, S12_out, inlier_out, n_inliers_out, chi2_out, iterations_done);
  cs_sim3_pairs_destroy(B);
  return rc;
}

int cs_sim3_pairs_linearize(int device, int n_pairs, const double* S12_in, const double* intr8, const unsigned char* fix_scale, const int* match_ptr,
                            const double* P1, const double* P2, const double* obs1, const double* obs2, double* err4, double* jac28) {
  if (n_pairs < 0) { cs_set_error("cs_sim3_pairs_linearize: a negative pair count"); return CS_ERR_INVALID_ARG; }
  if (n_pairs == 0) return CS_OK;
  size_t n = 0;
  int rc = check_pairs("cs_sim3_pairs_linearize", n_pairs, S12_in, intr8, fix_scale, match_ptr, P1, P2, obs1, obs2, nullptr, nullptr, &n); if (rc) return rc;
  if (n == 0) return CS_OK;
  if (!err4 || !jac28) { cs_set_error("cs_sim3_pairs_linearize: NULL output"); return CS_ERR_INVALID_ARG; }
  cs_sim3_pairs* B = nullptr;
  rc = cs_sim3_pairs_create(device, &B);
  if (rc) return rc;
  cs::Guard<cs_sim3_pairs> g(B, cs_sim3_pairs_destroy);     // (this call's own handle: never disarmed)
  const size_t np = (size_t)n_pairs;
  const InLayout L = in_layout(np, n);
  cs::Layout out;
  const size_t out_err = out.add(4 * n * 8), out_jac = out.add(28 * n * 8);
  cs::Sim3PairLaunch a;
  auto pack = [&] {
    pack_inputs(B->h_in.p, L, np, n, S12_in, intr8, fix_scale, match_ptr, P1, P2, obs1, obs2, nullptr, nullptr);
    set_inputs(a, B->d_in.p, L, n_pairs);
    a.err = reinterpret_cast<double*>(B->d_out.p + out_err);
    a.jac = reinterpret_cast<double*>(B->d_out.p + out_jac);
  };
  rc = cs::batch_round_trip(*B, L.bytes, out.bytes, false, pack, [&] { cs::sim3_pair_launch_linearize(a, B->st); }); if (rc) return rc;
  std::memcpy(err4, B->h_out.p + out_err, 4 * n * 8);
  std::memcpy(jac28, B->h_out.p + out_jac, 28 * n * 8);
  return CS_OK;
}

}  // extern "C"
