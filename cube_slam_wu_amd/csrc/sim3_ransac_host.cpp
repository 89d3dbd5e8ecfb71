// sim3_ransac_host.cpp -- the C ABI of the batched Sim(3) RANSAC of keyframe pairs (include/cubeslam_hip.h: cs_sim3_ransac_*).
//
// What an ORB-SLAM2-derived loop closer does once per loop candidate with Sim3Solver -- a RANSAC over 3-point Horn alignments of the
// matched map points, whose first hypothesis with more than min_inliers inliers is the start of Optimizer::OptimizeSim3 -- for many pairs
// in ONE kernel launch (sim3_ransac_kernels.hip).  The host checks every argument, works out each pair's iteration budget in double,
// packs the matches into 64-byte records, uploads everything with one copy, launches, and downloads everything with one copy.
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
#include "sim3_ransac_types.h"

// d_in = [intr | records | match_ptr | max_its | seed | fix_scale], d_out = [S_out | found | hyp | iterations | n_inliers | inlier] or [S_each | count_each]
struct cs_sim3_ransac : cs::BatchHandle {};

namespace {

using cs::all_finite;
using cs::none_negative;

int check_params(const cs_sim3_ransac_params* p) {
  const cs::Refuse refuse{"cs_sim3_ransac"};
  if (!p) return refuse("NULL parameters");
  if (!(p->probability > 0 && p->probability < 1)) return refuse("probability must be inside (0, 1)");
  if (p->min_inliers < 0) return refuse("min_inliers must not be negative");
  if (p->max_iterations < 1 || p->max_iterations > cs::SIM3_RANSAC_MAX_ITERATIONS) return refuse("max_iterations must be 1..1024");
  return CS_OK;
}

// What both entries check before anything is launched.  *n_matches = match_ptr[n_pairs].
int check_pairs(const char* who, int n_pairs, const double* intr8, const unsigned char* fix_scale, const unsigned long long* seed, const int* match_ptr,
                const double* P1, const double* P2, const double* max_err1, const double* max_err2, size_t* n_matches) {
  const cs::Refuse refuse{who};
  if (!intr8 || !fix_scale || !seed || !match_ptr) return refuse("NULL argument");
  if (int rc = cs::check_partition(std::string(who) + ": match_ptr", match_ptr, n_pairs)) return rc;
  const size_t n = (size_t)match_ptr[n_pairs];
  if (n > (size_t)INT_MAX / cs::SIM3_RANSAC_STAGED_DOUBLES) return refuse("too many matches for one call");      // every index the kernel forms fits an int
  if (n > 0 && (!P1 || !P2 || !max_err1 || !max_err2)) return refuse("NULL match array");
  if (!all_finite(intr8, 8 * (size_t)n_pairs)) return refuse("an intrinsic is not finite");
  if (!all_finite(P1, 3 * n) || !all_finite(P2, 3 * n)) return refuse("a point is not finite");
  if (!all_finite(max_err1, n) || !all_finite(max_err2, n)) return refuse("a threshold is not finite");
  if (!none_negative(max_err1, n) || !none_negative(max_err2, n)) return refuse("a threshold is negative");
  *n_matches = n;
  return CS_OK;
}

// the parts of d_in, in their order
struct InLayout {
  cs::Layout all;
  cs::Part<double> intr, rec;
  cs::Part<int> ptr, its;
  cs::Part<unsigned long long> seed;
  cs::Part<unsigned char> fs;
  InLayout(size_t np, size_t n)
      : intr(all.add<double>(8 * np)), rec(all.add<double>(n * cs::SIM3_RANSAC_MATCH_DOUBLES)), ptr(all.add<int>(np + 1)), its(all.add<int>(np)),
        seed(all.add<unsigned long long>(np)), fs(all.add<unsigned char>(np)) {}
};

// p == nullptr: the inspection form, which has no budget
void pack_inputs(cs::PinBuf<unsigned char>& h, const InLayout& L, size_t np, size_t n, const cs_sim3_ransac_params* p, const double* intr8, const unsigned char* fix_scale,
                 const unsigned long long* seed, const int* match_ptr, const double* P1, const double* P2, const double* max_err1, const double* max_err2) {
  cs::copy_in(L.intr, h, intr8);
  cs::copy_in(L.ptr, h, match_ptr);
  cs::copy_in(L.seed, h, seed);
  cs::copy_in(L.fs, h, fix_scale);
  int* its = L.its.at(h.p);
  for (size_t f = 0; f < np; f++) its[f] = p ? cs::sim3_ransac_budget(match_ptr[f + 1] - match_ptr[f], p->probability, p->min_inliers, p->max_iterations) : 0;
  double* rec = L.rec.at(h.p);
  for (size_t i = 0; i < n; i++, rec += cs::SIM3_RANSAC_MATCH_DOUBLES) {
    for (int k = 0; k < 3; k++) { rec[k] = P1[3 * i + k]; rec[3 + k] = P2[3 * i + k]; }
    rec[6] = max_err1[i];
    rec[7] = max_err2[i];
  }
}

void set_inputs(cs::Sim3RansacLaunch& a, unsigned char* d, const InLayout& L, int n_pairs) {
  std::memset(&a, 0, sizeof(a));
  a.n_pairs = n_pairs;
  a.intr = L.intr.at(d); a.rec = L.rec.at(d); a.match_ptr = L.ptr.at(d); a.max_its = L.its.at(d); a.seed = L.seed.at(d); a.fix_scale = L.fs.at(d);
}

}  // namespace

extern "C" {

void cs_sim3_ransac_default_params(cs_sim3_ransac_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->probability = 0.99;
  p->min_inliers = 20;
  p->max_iterations = 300;
}

int cs_sim3_ransac_create(int device, cs_sim3_ransac** out) { return cs::batch_create(device, out); }

void cs_sim3_ransac_destroy(cs_sim3_ransac* B) { cs::batch_destroy(B); }

int cs_sim3_ransac_run(cs_sim3_ransac* B, const cs_sim3_ransac_params* p, int n_pairs, const double* intr8, const unsigned char* fix_scale, const unsigned long long* seed,
                       const int* match_ptr, const double* P1, const double* P2, const double* max_err1, const double* max_err2,
                       int* found_out, int* hyp_out, int* iterations_out, double* S12_out, unsigned char* inlier_out, int* n_inliers_out) {
  const cs::Refuse refuse{"cs_sim3_ransac_run"};
  if (!B || n_pairs < 0) return refuse("no handle or a negative pair count");
  int rc = check_params(p); if (rc) return rc;
  cs::BatchCall call(*B);
  if (n_pairs == 0) return call.empty();
  size_t n = 0;
  rc = check_pairs("cs_sim3_ransac_run", n_pairs, intr8, fix_scale, seed, match_ptr, P1, P2, max_err1, max_err2, &n); if (rc) return rc;
  if (!found_out || !S12_out || !n_inliers_out || (n > 0 && !inlier_out)) return refuse("NULL output");
  call.point_of_no_return();                           // (behind the checks: cs_batch_handle.h, BatchCall)
  const size_t np = (size_t)n_pairs;

  const InLayout L(np, n);
  cs::Layout out;
  const auto out_S = out.add<double>(8 * np);
  const auto out_found = out.add<int>(np), out_hyp = out.add<int>(np), out_it = out.add<int>(np), out_ni = out.add<int>(np);
  const auto out_fl = out.add<unsigned char>(n);

  cs::Sim3RansacLaunch a;
  auto pack = [&] {
    pack_inputs(B->h_in, L, np, n, p, intr8, fix_scale, seed, match_ptr, P1, P2, max_err1, max_err2);
    set_inputs(a, B->d_in.p, L, n_pairs);
    a.min_inliers = p->min_inliers;
    unsigned char* d = B->d_out.p;
    a.S_out = out_S.at(d); a.found = out_found.at(d); a.hyp = out_hyp.at(d); a.iterations = out_it.at(d); a.n_inliers = out_ni.at(d); a.inlier = out_fl.at(d);
  };
  rc = cs::batch_round_trip(*B, L.all.bytes, out.bytes, true, pack, [&] { cs::sim3_ransac_launch(a, false, B->st); }); if (rc) return rc;

  cs::copy_out(out_S, B->h_out, S12_out);
  cs::copy_out(out_found, B->h_out, found_out);
  if (hyp_out) cs::copy_out(out_hyp, B->h_out, hyp_out);
  if (iterations_out) cs::copy_out(out_it, B->h_out, iterations_out);
  cs::copy_out(out_ni, B->h_out, n_inliers_out);
  if (n) cs::copy_out(out_fl, B->h_out, inlier_out);
  return call.done();
}

int cs_sim3_ransac_last_timing(const cs_sim3_ransac* B, double* kernel_ms, double* host_ms) { return cs::batch_last_timing(B, kernel_ms, host_ms); }

int cs_sim3_ransac_pairs(int device, const cs_sim3_ransac_params* p, int n_pairs, const double* intr8, const unsigned char* fix_scale, const unsigned long long* seed,
                         const int* match_ptr, const double* P1, const double* P2, const double* max_err1, const double* max_err2,
                         int* found_out, int* hyp_out, int* iterations_out, double* S12_out, unsigned char* inlier_out, int* n_inliers_out) {
  if (n_pairs < 0) return cs::Refuse{"cs_sim3_ransac_pairs"}("a negative pair count");
  return cs::batch_one_shot<cs_sim3_ransac>(device, [&](cs_sim3_ransac* B) -> int {
    return cs_sim3_ransac_run(B, p, n_pairs, intr8, fix_scale, seed, match_ptr, P1, P2, max_err1, max_err2, found_out, hyp_out, iterations_out, S12_out, inlier_out, n_inliers_out);
  });
}

int cs_sim3_ransac_triplets(unsigned long long seed, int n_matches, int n_hyp, int* out3) {
  if (n_matches < 3 || n_hyp < 0 || (n_hyp > 0 && !out3)) return cs::Refuse{"cs_sim3_ransac_triplets"}("fewer than three matches, a negative count or a NULL output");
  for (int h = 0; h < n_hyp; h++) cs::sim3_ransac_triple(seed, h, n_matches, out3 + 3 * (size_t)h);
  return CS_OK;
}

int cs_sim3_ransac_hypotheses(int device, int n_pairs, const double* intr8, const unsigned char* fix_scale, const unsigned long long* seed, const int* match_ptr,
                              const double* P1, const double* P2, const double* max_err1, const double* max_err2, int n_hyp, double* S12_each, int* count_each) {
  const cs::Refuse refuse{"cs_sim3_ransac_hypotheses"};
  if (n_pairs < 0) return refuse("a negative pair count");
  if (n_hyp < 1 || n_hyp > cs::SIM3_RANSAC_MAX_ITERATIONS) return refuse("n_hyp must be 1..1024");
  if (n_pairs == 0) return CS_OK;
  size_t n = 0;
  int rc = check_pairs("cs_sim3_ransac_hypotheses", n_pairs, intr8, fix_scale, seed, match_ptr, P1, P2, max_err1, max_err2, &n); if (rc) return rc;
  if (!S12_each || !count_each) return refuse("NULL output");
  return cs::batch_one_shot<cs_sim3_ransac>(device, [&](cs_sim3_ransac* B) -> int {
    const size_t np = (size_t)n_pairs, each = np * (size_t)n_hyp;
    const InLayout L(np, n);
    cs::Layout out;
    const auto out_S = out.add<double>(8 * each);
    const auto out_cnt = out.add<int>(each);
    cs::Sim3RansacLaunch a;
    auto pack = [&] {
      pack_inputs(B->h_in, L, np, n, nullptr, intr8, fix_scale, seed, match_ptr, P1, P2, max_err1, max_err2);
      set_inputs(a, B->d_in.p, L, n_pairs);
      a.n_hyp = n_hyp;
      a.S_each = out_S.at(B->d_out.p); a.count_each = out_cnt.at(B->d_out.p);
    };
    rc = cs::batch_round_trip(*B, L.all.bytes, out.bytes, false, pack, [&] { cs::sim3_ransac_launch(a, true, B->st); }); if (rc) return rc;
    cs::copy_out(out_S, B->h_out, S12_each);
    cs::copy_out(out_cnt, B->h_out, count_each);
    return CS_OK;
  });
}

}  // extern "C"
