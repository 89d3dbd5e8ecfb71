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

using cs::all_finite;

int check_params(const cs_sim3_pair_params* p) {
  const cs::Refuse refuse{"cs_sim3"};
  if (!p) return refuse("NULL parameters");
  const int its[3] = {p->iterations_first, p->iterations_more_clean, p->iterations_more_outliers};
  for (int k = 0; k < 3; k++)
    if (its[k] < 0 || its[k] > cs::SIM3_PAIR_MAX_ITERATIONS) return refuse("an iteration count must be 0..100");
  if (!std::isfinite(p->th2) || !std::isfinite(p->huber_delta)) return refuse("th2 / huber_delta not finite");
  return CS_OK;
}

// What both entries check before anything is launched.  *n_matches = match_ptr[n_pairs].
int check_pairs(const char* who, int n_pairs, const double* S12_in, const double* intr8, const unsigned char* fix_scale, const int* match_ptr,
                const double* P1, const double* P2, const double* obs1, const double* obs2, const double* info12, const double* info21, size_t* n_matches) {
  const cs::Refuse refuse{who};
  if (!S12_in || !intr8 || !fix_scale || !match_ptr) return refuse("NULL argument");
  if (int rc = cs::check_partition(std::string(who) + ": match_ptr", match_ptr, n_pairs)) return rc;
  const size_t n = (size_t)match_ptr[n_pairs];
  if (n > (size_t)INT_MAX / 28) return refuse("too many matches for one call");      // every index the kernel forms, the Jacobians' included, fits an int
  if (n > 0 && (!P1 || !P2 || !obs1 || !obs2)) return refuse("NULL match array");
  if (!all_finite(S12_in, 8 * (size_t)n_pairs) || !all_finite(intr8, 8 * (size_t)n_pairs)) return refuse("a state or an intrinsic is not finite");
  for (int f = 0; f < n_pairs; f++)
    if (!(S12_in[8 * (size_t)f + 7] > 0)) return refuse("a scale is not positive");
  if (!all_finite(P1, 3 * n) || !all_finite(P2, 3 * n) || !all_finite(obs1, 2 * n) || !all_finite(obs2, 2 * n)) return refuse("a point or a keypoint is not finite");
  if ((info12 && !all_finite(info12, 4 * n)) || (info21 && !all_finite(info21, 4 * n))) return refuse("an information matrix is not finite");
  *n_matches = n;
  return CS_OK;
}

// the parts of d_in, in their order
struct InLayout {
  cs::Layout all;
  cs::Part<double> S, intr, rec;
  cs::Part<int> ptr;
  cs::Part<unsigned char> fs;
  InLayout(size_t np, size_t n)
      : S(all.add<double>(8 * np)), intr(all.add<double>(8 * np)), rec(all.add<double>(n * cs::SIM3_PAIR_MATCH_DOUBLES)), ptr(all.add<int>(np + 1)),
        fs(all.add<unsigned char>(np)) {}
};

void pack_inputs(cs::PinBuf<unsigned char>& h, const InLayout& L, size_t n, const double* S12_in, const double* intr8, const unsigned char* fix_scale, const int* match_ptr,
                 const double* P1, const double* P2, const double* obs1, const double* obs2, const double* info12, const double* info21) {
  cs::copy_in(L.S, h, S12_in);
  cs::copy_in(L.intr, h, intr8);
  cs::copy_in(L.ptr, h, match_ptr);
  cs::copy_in(L.fs, h, fix_scale);
  double* rec = L.rec.at(h.p);
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
  a.S0 = L.S.at(d); a.intr = L.intr.at(d); a.rec = L.rec.at(d); a.match_ptr = L.ptr.at(d); a.fix_scale = L.fs.at(d);
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
  const cs::Refuse refuse{"cs_sim3_pairs_optimize"};
  if (!B || n_pairs < 0) return refuse("no handle or a negative pair count");
  int rc = check_params(p); if (rc) return rc;
  cs::BatchCall call(*B);
  if (n_pairs == 0) return call.empty();
  size_t n = 0;
  rc = check_pairs("cs_sim3_pairs_optimize", n_pairs, S12_in, intr8, fix_scale, match_ptr, P1, P2, obs1, obs2, info12, info21, &n); if (rc) return rc;
  if (!S12_out || !n_inliers_out || (n > 0 && !inlier_out)) return refuse("NULL output");
  call.point_of_no_return();                           // (behind the checks: cs_batch_handle.h, BatchCall)
  const size_t np = (size_t)n_pairs;

  // ---- layout of the two buffers
  const InLayout L(np, n);
  cs::Layout out;
  const auto out_S = out.add<double>(8 * np), out_chi = out.add<double>(2 * np);
  const auto out_it = out.add<int>(2 * np), out_ni = out.add<int>(np);
  const auto out_lv = out.add<unsigned char>(n);

  cs::Sim3PairLaunch a;
  auto pack = [&] {
    pack_inputs(B->h_in, L, n, S12_in, intr8, fix_scale, match_ptr, P1, P2, obs1, obs2, info12, info21);
    set_inputs(a, B->d_in.p, L, n_pairs);
    a.sched.iterations_first = p->iterations_first; a.sched.iterations_more_clean = p->iterations_more_clean; a.sched.iterations_more_outliers = p->iterations_more_outliers;
    a.sched.robust_second_round = p->robust_second_round ? 1 : 0; a.sched.min_inliers = p->min_inliers;
    a.sched.th2 = p->th2; a.sched.huber_delta = p->huber_delta;
    unsigned char* d = B->d_out.p;
    a.S_out = out_S.at(d); a.chi2_out = out_chi.at(d); a.iters_out = out_it.at(d); a.n_inliers = out_ni.at(d); a.inlier = out_lv.at(d);
  };
  rc = cs::batch_round_trip(*B, L.all.bytes, out.bytes, true, pack, [&] { cs::sim3_pair_launch(a, B->st); }); if (rc) return rc;

  cs::copy_out(out_S, B->h_out, S12_out);
  if (chi2_out) cs::copy_out(out_chi, B->h_out, chi2_out);
  if (iterations_done) cs::copy_out(out_it, B->h_out, iterations_done);
  cs::copy_out(out_ni, B->h_out, n_inliers_out);
  if (n) cs::copy_out(out_lv, B->h_out, inlier_out);
  return call.done();
}

int cs_sim3_pairs_last_timing(const cs_sim3_pairs* B, double* kernel_ms, double* host_ms) { return cs::batch_last_timing(B, kernel_ms, host_ms); }

int cs_sim3_optimize_pairs(int device, const cs_sim3_pair_params* p, int n_pairs, const double* S12_in, const double* intr8, const unsigned char* fix_scale,
                           const int* match_ptr, const double* P1, const double* P2, const double* obs1, const double* obs2, const double* info12, const double* info21,
                           double* S12_out, unsigned char* inlier_out, int* n_inliers_out, double* chi2_out, int* iterations_done) {
  if (n_pairs < 0) return cs::Refuse{"cs_sim3_optimize_pairs"}("a negative pair count");
  return cs::batch_one_shot<cs_sim3_pairs>(device, [&](cs_sim3_pairs* B) -> int {
    return cs_sim3_pairs_optimize(B, p, n_pairs, S12_in, intr8, fix_scale, match_ptr, P1, P2, obs1, obs2, info12, info21, S12_out, inlier_out, n_inliers_out, chi2_out, iterations_done);
  });
}

int cs_sim3_pairs_linearize(int device, int n_pairs, const double* S12_in, const double* intr8, const unsigned char* fix_scale, const int* match_ptr,
                            const double* P1, const double* P2, const double* obs1, const double* obs2, double* err4, double* jac28) {
  const cs::Refuse refuse{"cs_sim3_pairs_linearize"};
  if (n_pairs < 0) return refuse("a negative pair count");
  if (n_pairs == 0) return CS_OK;
  size_t n = 0;
  int rc = check_pairs("cs_sim3_pairs_linearize", n_pairs, S12_in, intr8, fix_scale, match_ptr, P1, P2, obs1, obs2, nullptr, nullptr, &n); if (rc) return rc;
  if (n == 0) return CS_OK;
  if (!err4 || !jac28) return refuse("NULL output");
  return cs::batch_one_shot<cs_sim3_pairs>(device, [&](cs_sim3_pairs* B) -> int {
    const InLayout L((size_t)n_pairs, n);
    cs::Layout out;
    const auto out_err = out.add<double>(4 * n), out_jac = out.add<double>(28 * n);
    cs::Sim3PairLaunch a;
    auto pack = [&] {
      pack_inputs(B->h_in, L, n, S12_in, intr8, fix_scale, match_ptr, P1, P2, obs1, obs2, nullptr, nullptr);
      set_inputs(a, B->d_in.p, L, n_pairs);
      a.err = out_err.at(B->d_out.p); a.jac = out_jac.at(B->d_out.p);
    };
    rc = cs::batch_round_trip(*B, L.all.bytes, out.bytes, false, pack, [&] { cs::sim3_pair_launch_linearize(a, B->st); }); if (rc) return rc;
    cs::copy_out(out_err, B->h_out, err4);
    cs::copy_out(out_jac, B->h_out, jac28);
    return CS_OK;
  });
}

}  // extern "C"
