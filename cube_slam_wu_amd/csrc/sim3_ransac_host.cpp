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

bool all_finite(const double* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!std::isfinite(v[i])) return false;
  return true;
}

bool none_negative(const double* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!(v[i] >= 0)) return false;
  return true;
}

int check_params(const cs_sim3_ransac_params* p) {
  if (!p) { cs_set_error("cs_sim3_ransac: NULL parameters"); return CS_ERR_INVALID_ARG; }
  if (!(p->probability > 0 && p->probability < 1)) { cs_set_error("cs_sim3_ransac: probability must be inside (0, 1)"); return CS_ERR_INVALID_ARG; }
  if (p->min_inliers < 0) { cs_set_error("cs_sim3_ransac: min_inliers must not be negative"); return CS_ERR_INVALID_ARG; }
  if (p->max_iterations < 1 || p->max_iterations > cs::SIM3_RANSAC_MAX_ITERATIONS) { cs_set_error("cs_sim3_ransac: max_iterations must be 1..1024"); return CS_ERR_INVALID_ARG; }
  return CS_OK;
}

// What both entries check before anything is launched.  *n_matches = match_ptr[n_pairs].
int check_pairs(const char* who, int n_pairs, const double* intr8, const unsigned char* fix_scale, const unsigned long long* seed, const int* match_ptr,
                const double* P1, const double* P2, const double* max_err1, const double* max_err2, size_t* n_matches) {
  auto fail = [&](const char* what) { cs_set_error((std::string(who) + ": " + what).c_str()); return CS_ERR_INVALID_ARG; };
  if (!intr8 || !fix_scale || !seed || !match_ptr) return fail("NULL argument");
  if (int rc = cs::check_partition(std::string(who) + ": match_ptr", match_ptr, n_pairs)) return rc;
  const size_t n = (size_t)match_ptr[n_pairs];
  if (n > (size_t)INT_MAX / cs::SIM3_RANSAC_STAGED_DOUBLES) return fail("too many matches for one call");      // every index the kernel forms fits an int
  if (n > 0 && (!P1 || !P2 || !max_err1 || !max_err2)) return fail("NULL match array");
  if (!all_finite(intr8, 8 * (size_t)n_pairs)) return fail("an intrinsic is not finite");
  if (!all_finite(P1, 3 * n) || !all_finite(P2, 3 * n)) return fail("a point is not finite");
  if (!all_finite(max_err1, n) || !all_finite(max_err2, n)) return fail("a threshold is not finite");
  if (!none_negative(max_err1, n) || !none_negative(max_err2, n)) return fail("a threshold is negative");
  *n_matches = n;
  return CS_OK;
}

struct InLayout { size_t intr, rec, ptr, its, seed, fs, bytes; };

InLayout in_layout(size_t np, size_t n) {
  cs::Layout in;
  InLayout L;
  L.intr = in.add(8 * np * 8);
  L.rec = in.add(n * cs::SIM3_RANSAC_MATCH_DOUBLES * 8);
  L.ptr = in.add((np + 1) * 4);
  L.its = in.add(np * 4);
  L.seed = in.add(np * 8);
  L.fs = in.add(np);
  L.bytes = in.bytes;
  return L;
}

// p == nullptr: the inspection form, which has no budget
void pack_inputs(unsigned char* h, const InLayout& L, size_t np, size_t n, const cs_sim3_ransac_params* p, const double* intr8, const unsigned char* fix_scale,
                 const unsigned long long* seed, const int* match_ptr, const double* P1, const double* P2, const double* max_err1, const double* max_err2) {
  std::memcpy(h + L.intr, intr8, 8 * np * 8);
  std::memcpy(h + L.ptr, match_ptr, (np + 1) * 4);
  std::memcpy(h + L.seed, seed, np * 8);
  std::memcpy(h + L.fs, fix_scale, np);
  int* its = reinterpret_cast<int*>(h + L.its);
  for (size_t f = 0; f < np; f++) its[f] = p ? cs::sim3_ransac_budget(match_ptr[f + 1] - match_ptr[f], p->probability, p->min_inliers, p->max_iterations) : 0;
  double* rec = reinterpret_cast<double*>(h + L.rec);
  for (size_t i = 0; i < n; i++, rec += cs::SIM3_RANSAC_MATCH_DOUBLES) {
    for (int k = 0; k < 3; k++) { rec[k] = P1[3 * i + k]; rec[3 + k] = P2[3 * i + k]; }
    rec[6] = max_err1[i];
    rec[7] = max_err2[i];
  }
}

void set_inputs(cs::Sim3RansacLaunch& a, unsigned char* d, const InLayout& L, int n_pairs) {
  std::memset(&a, 0, sizeof(a));
  a.n_pairs = n_pairs;
  a.intr = reinterpret_cast<const double*>(d + L.intr);
  a.rec = reinterpret_cast<const double*>(d + L.rec);
  a.match_ptr = reinterpret_cast<const int*>(d + L.ptr);
  a.max_its = reinterpret_cast<const int*>(d + L.its);
  a.seed = reinterpret_cast<const unsigned long long*>(d + L.seed);
  a.fix_scale = d + L.fs;
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
  if (!B || n_pairs < 0) { cs_set_error("cs_sim3_ransac_run: no handle or a negative pair count"); return CS_ERR_INVALID_ARG; }
  int rc = check_params(p); if (rc) return rc;
  if (n_pairs == 0) { B->kernel_ms = B->host_ms = 0; B->ran = true; return CS_OK; }
  const double t_begin = cs::now_ms();
  size_t n = 0;
  rc = check_pairs("cs_sim3_ransac_run", n_pairs, intr8, fix_scale, seed, match_ptr, P1, P2, max_err1, max_err2, &n); if (rc) return rc;
  if (!found_out || !S12_out || !n_inliers_out || (n > 0 && !inlier_out)) { cs_set_error("cs_sim3_ransac_run: NULL output"); return CS_ERR_INVALID_ARG; }
  B->ran = false;                                      // (a refused call leaves the last run's timing in place; one that fails from here on does not)
  const size_t np = (size_t)n_pairs;

  const InLayout L = in_layout(np, n);
  cs::Layout out;
  const size_t out_S = out.add(8 * np * 8), out_found = out.add(np * 4), out_hyp = out.add(np * 4), out_it = out.add(np * 4), out_ni = out.add(np * 4), out_fl = out.add(n);

  cs::Sim3RansacLaunch a;
  auto pack = [&] {
    pack_inputs(B->h_in.p, L, np, n, p, intr8, fix_scale, seed, match_ptr, P1, P2, max_err1, max_err2);
    set_inputs(a, B->d_in.p, L, n_pairs);
    a.min_inliers = p->min_inliers;
    a.S_out = reinterpret_cast<double*>(B->d_out.p + out_S);
    a.found = reinterpret_cast<int*>(B->d_out.p + out_found);
    a.hyp = reinterpret_cast<int*>(B->d_out.p + out_hyp);
    a.iterations = reinterpret_cast<int*>(B->d_out.p + out_it);
    a.n_inliers = reinterpret_cast<int*>(B->d_out.p + out_ni);
    a.inlier = B->d_out.p + out_fl;
  };
  rc = cs::batch_round_trip(*B, L.bytes, out.bytes, true, pack, [&] { cs::sim3_ransac_launch(a, false, B->st); }); if (rc) return rc;

  std::memcpy(S12_out, B->h_out.p + out_S, 8 * np * 8);
  std::memcpy(found_out, B->h_out.p + out_found, np * 4);
  if (hyp_out) std::memcpy(hyp_out, B->h_out.p + out_hyp, np * 4);
  if (iterations_out) std::memcpy(iterations_out, B->h_out.p + out_it, np * 4);
  std::memcpy(n_inliers_out, B->h_out.p + out_ni, np * 4);
  if (n) std::memcpy(inlier_out, B->h_out.p + out_fl, n);
  B->host_ms = cs::now_ms() - t_begin;
  B->ran = true;
  return CS_OK;
}

int cs_sim3_ransac_last_timing(const cs_sim3_ransac* B, double* kernel_ms, double* host_ms) { return cs::batch_last_timing(B, kernel_ms, host_ms); }

int cs_sim3_ransac_pairs(int device, const cs_sim3_ransac_params* p, int n_pairs, const double* intr8, const unsigned char* fix_scale, const unsigned long long* seed,
                         const int* match_ptr, const double* P1, const double* P2, const double* max_err1, const double* max_err2,
                         int* found_out, int* hyp_out, int* iterations_out, double* S12_out, unsigned char* inlier_out, int* n_inliers_out) {
  if (n_pairs < 0) { cs_set_error("cs_sim3_ransac_pairs: a negative pair count"); return CS_ERR_INVALID_ARG; }
  cs_sim3_ransac* B = nullptr;
  int rc = cs_sim3_ransac_create(device, &B);
  if (rc) return rc;
  rc = cs_sim3_ransac_run(B, p, n_pairs, intr8, fix_scale, seed, match_ptr, P1, P2, max_err1, max_err2, found_out, hyp_out, iterations_out, S12_out, inlier_out, n_inliers_out);
  cs_sim3_ransac_destroy(B);
  return rc;
}

int cs_sim3_ransac_triplets(unsigned long long seed, int n_matches, int n_hyp, int* out3) {
  if (n_matches < 3 || n_hyp < 0 || (n_hyp > 0 && !out3)) { cs_set_error("cs_sim3_ransac_triplets: fewer than three matches, a negative count or a NULL output"); return CS_ERR_INVALID_ARG; }
  for (int h = 0; h < n_hyp; h++) cs::sim3_ransac_triple(seed, h, n_matches, out3 + 3 * (size_t)h);
  return CS_OK;
}

int cs_sim3_ransac_hypotheses(int device, int n_pairs, const double* intr8, const unsigned char* fix_scale, const unsigned long long* seed, const int* match_ptr,
                              const double* P1, const double* P2, const double* max_err1, const double* max_err2, int n_hyp, double* S12_each, int* count_each) {
  if (n_pairs < 0) { cs_set_error("cs_sim3_ransac_hypotheses: a negative pair count"); return CS_ERR_INVALID_ARG; }
  if (n_hyp < 1 || n_hyp > cs::SIM3_RANSAC_MAX_ITERATIONS) { cs_set_error("cs_sim3_ransac_hypotheses: n_hyp must be 1..1024"); return CS_ERR_INVALID_ARG; }
  if (n_pairs == 0) return CS_OK;
  size_t n = 0;
  int rc = check_pairs("cs_sim3_ransac_hypotheses", n_pairs, intr8, fix_scale, seed, match_ptr, P1, P2, max_err1, max_err2, &n); if (rc) return rc;
  if (!S12_each || !count_each) { cs_set_error("cs_sim3_ransac_hypotheses: NULL output"); return CS_ERR_INVALID_ARG; }
  cs_sim3_ransac* B = nullptr;
  rc = cs_sim3_ransac_create(device, &B);
  if (rc) return rc;
  cs::Guard<cs_sim3_ransac> g(B, cs_sim3_ransac_destroy);     // (this call's own handle: never disarmed)
  const size_t np = (size_t)n_pairs, each = np * (size_t)n_hyp;
  const InLayout L = in_layout(np, n);
  cs::Layout out;
  const size_t out_S = out.add(8 * each * 8), out_cnt = out.add(each * 4);
  cs::Sim3RansacLaunch a;
  auto pack = [&] {
    pack_inputs(B->h_in.p, L, np, n, nullptr, intr8, fix_scale, seed, match_ptr, P1, P2, max_err1, max_err2);
    set_inputs(a, B->d_in.p, L, n_pairs);
    a.n_hyp = n_hyp;
    a.S_each = reinterpret_cast<double*>(B->d_out.p + out_S);
    a.count_each = reinterpret_cast<int*>(B->d_out.p + out_cnt);
  };
  rc = cs::batch_round_trip(*B, L.bytes, out.bytes, false, pack, [&] { cs::sim3_ransac_launch(a, true, B->st); }); if (rc) return rc;
  std::memcpy(S12_each, B->h_out.p + out_S, 8 * each * 8);
  std::memcpy(count_each, B->h_out.p + out_cnt, each * 4);
  return CS_OK;
}

}  // extern "C"
