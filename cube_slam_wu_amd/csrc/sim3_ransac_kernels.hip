// sim3_ransac_kernels.hip -- Sim(3) RANSAC of keyframe pairs, many pairs per launch (include/cubeslam_hip.h: cs_sim3_ransac_*).
//
// The arithmetic is cs_sim3_ransac.h's (the Sim3Solver steps it restates are named there); this file gives it its wave: one wavefront
// per pair and ONE LANE, ONE HYPOTHESIS.  Lane l of hypothesis block b draws the triple of hypothesis 64 b + l, runs the Horn solve on it
// and counts its own inliers in a register; nothing is reduced.  The matches come from LDS: the wave stages the pair's matches in chunks
// of SIM3_RANSAC_CHUNK = 64 (lane l loads packed match l of the chunk as aligned double2s, projects both stored points once and writes
// the 12-double staged record to the wave's own slice), then every lane walks the chunk reading the SAME address -- identical addresses
// broadcast, so the walk has no bank conflict.  (The staging writes, 96 bytes apart, do conflict; there is one of them per 64 reads.)
// A pair that fits one chunk is staged once, not once per hypothesis block.
//
// Selection per block of 64 hypotheses is the sequential rule of cs_sim3_ransac.h: lanes past max_its are masked out; a ballot of
// count > min_inliers takes the LOWEST lane as the winner and ends the search; otherwise the block's best is the largest count with ties
// to the HIGHEST lane, and it replaces the stored best on >=, so a later block wins ties against an earlier one.  The up to 63
// hypotheses evaluated past a winner are never looked at.  The chosen lane's hypothesis is then shared with all lanes and one more pass,
// lanes over matches, writes the flags with the routines and operands of the count.
//
// A wave touches no other wave's slice and the kernel has no barrier: a wavefront whose pair does not exist leaves at once.  Every
// loop is bounded by max_its <= 1024 or by the pair's match count.  FP64, -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "cs_wave.h"
#include "sim3_ransac_types.h"

namespace cs {
namespace {

enum { WAVE_LDS_DOUBLES = SIM3_RANSAC_CHUNK * SIM3_RANSAC_STAGED_DOUBLES };
static_assert(SIM3_RANSAC_CHUNK == 64, "one staged match per lane");

// one wave, program order: the fence keeps the compiler from moving LDS accesses across it
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ long long wave_max_all(long long v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) { const long long o = __shfl_xor(v, m, 64); v = o > v ? o : v; }
  return v;
}

__device__ __forceinline__ Sim3RansacHyp hyp_from_lane(const Sim3RansacHyp& H, int src) {
  Sim3RansacHyp B;
#pragma unroll
  for (int k = 0; k < 4; k++) B.q[k] = __shfl(H.q[k], src, 64);
#pragma unroll
  for (int k = 0; k < 3; k++) B.t[k] = __shfl(H.t[k], src, 64);
  B.s = __shfl(H.s, src, 64);
  return B;
}

template <bool INSPECT>
__global__ void __launch_bounds__(64 * SIM3_RANSAC_WAVES_PER_BLOCK) sim3_ransac_kernel(const Sim3RansacLaunch a) {
  __shared__ __attribute__((aligned(16))) double lds[SIM3_RANSAC_WAVES_PER_BLOCK * WAVE_LDS_DOUBLES];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int f = blockIdx.x * SIM3_RANSAC_WAVES_PER_BLOCK + wave;
  if (f >= a.n_pairs) return;                        // (a whole wavefront leaves: there is no barrier in this kernel)
  const int lane = threadIdx.x & 63;
  double* st = lds + wave * WAVE_LDS_DOUBLES;

  const int m0 = a.match_ptr[f];
  const int n = a.match_ptr[f + 1] - m0;
  const double* __restrict__ rec = a.rec + (size_t)m0 * SIM3_RANSAC_MATCH_DOUBLES;
  double intr[8];
#pragma unroll
  for (int k = 0; k < 8; k++) intr[k] = a.intr[8 * (size_t)f + k];
  const bool fix_scale = a.fix_scale[f] != 0;
  const uint64_t seed = a.seed[f];
  int max_its = INSPECT ? a.n_hyp : a.max_its[f];
  if (max_its > SIM3_RANSAC_MAX_ITERATIONS) max_its = SIM3_RANSAC_MAX_ITERATIONS;      // (the host sends nothing larger; the loops below hold whatever it sends)
  if (n < 3) max_its = 0;                                                              // (a triple needs three matches)

  Sim3RansacResult r;
  sim3_ransac_result_init(r, max_its);
  Sim3RansacHyp best;
#pragma unroll
  for (int k = 0; k < 4; k++) best.q[k] = (k == 0) ? 1.0 : 0.0;
  best.t[0] = best.t[1] = best.t[2] = 0.0;
  best.s = 1.0;
  int best_count = 0;

  for (int h0 = 0; h0 < max_its; h0 += 64) {
    const int h = h0 + lane;
    const bool active = h < max_its;
    // ---- the lane's own triple and its Horn solve (a masked lane computes too: h is a valid counter, its result is not used)
    int idx[3];
    sim3_ransac_triple(seed, h, n, idx);
    double X1[9], X2[9];
#pragma unroll
    for (int k = 0; k < 3; k++) {
      double v[SIM3_RANSAC_MATCH_DOUBLES];
      load_record<SIM3_RANSAC_MATCH_DOUBLES>(rec + (size_t)idx[k] * SIM3_RANSAC_MATCH_DOUBLES, v);
#pragma unroll
      for (int i = 0; i < 3; i++) { X1[3 * k + i] = v[i]; X2[3 * k + i] = v[3 + i]; }
    }
    Sim3RansacHyp H;
    const bool valid = sim3_ransac_hypothesis(X1, X2, fix_scale, H) && active;
    const Sim3RansacMaps T = sim3_ransac_maps(H);

    // ---- its inliers, the matches as broadcasts from LDS
    int count = 0;
    for (int c0 = 0; c0 < n; c0 += SIM3_RANSAC_CHUNK) {
      const int cn = (n - c0 < SIM3_RANSAC_CHUNK) ? n - c0 : SIM3_RANSAC_CHUNK;
      if (h0 == 0 || n > SIM3_RANSAC_CHUNK) {          // (a single chunk staged for the first block is still there)
        wave_sync();
        if (lane < cn) {
          double v[SIM3_RANSAC_MATCH_DOUBLES], m[SIM3_RANSAC_STAGED_DOUBLES];
          load_record<SIM3_RANSAC_MATCH_DOUBLES>(rec + (size_t)(c0 + lane) * SIM3_RANSAC_MATCH_DOUBLES, v);
          sim3_ransac_stage(v, intr, m);
          double2* dst = reinterpret_cast<double2*>(st + lane * SIM3_RANSAC_STAGED_DOUBLES);
#pragma unroll
          for (int k = 0; k < SIM3_RANSAC_STAGED_DOUBLES / 2; k++) dst[k] = make_double2(m[2 * k], m[2 * k + 1]);
        }
        wave_sync();
      }
      for (int i = 0; i < cn; i++) {
        double m[SIM3_RANSAC_STAGED_DOUBLES];
        load_record<SIM3_RANSAC_STAGED_DOUBLES>(st + i * SIM3_RANSAC_STAGED_DOUBLES, m);
        count += sim3_ransac_inlier(T, m, intr) ? 1 : 0;
      }
    }

    if (INSPECT) {
      if (active) {
        double S[8];
        sim3_ransac_store(H, S);
        const size_t at = (size_t)f * a.n_hyp + h;
#pragma unroll
        for (int k = 0; k < 8; k++) a.S_each[8 * at + k] = valid ? S[k] : ((k == 3 || k == 7) ? 1.0 : 0.0);      // refused: the identity
        a.count_each[at] = valid ? count : -1;
      }
      continue;
    }

    // ---- the sequential rule over these 64
    const unsigned long long win = __ballot(valid && count > a.min_inliers);
    int src, src_count;
    if (win) {
      src = __ffsll((long long)win) - 1;
      src_count = __shfl(count, src, 64);
    } else {
      const long long key = wave_max_all(valid ? (long long)count * 64 + lane : -1LL);
      if (key < 0) continue;                           // every hypothesis of the block refused
      src = (int)(key & 63);
      src_count = (int)(key >> 6);
      if (src_count < best_count) continue;
    }
    best = hyp_from_lane(H, src);
    best_count = src_count;
    r.hyp = h0 + src;
    if (win) { r.found = 1; r.iterations = r.hyp + 1; break; }
  }

  if (INSPECT) {
    if (max_its == 0) {                                // fewer than three matches: no hypothesis exists
      for (int h = lane; h < a.n_hyp; h += 64) {
        const size_t at = (size_t)f * a.n_hyp + h;
#pragma unroll
        for (int k = 0; k < 8; k++) a.S_each[8 * at + k] = (k == 3 || k == 7) ? 1.0 : 0.0;
        a.count_each[at] = -1;
      }
    }
    return;
  }

  // ---- the flags: lanes over matches, the routines and operands of the count
  if (r.hyp >= 0) {
    r.n_inliers = best_count;
    sim3_ransac_store(best, r.S12);
    const Sim3RansacMaps T = sim3_ransac_maps(best);
    for (int i = lane; i < n; i += 64) {
      double v[SIM3_RANSAC_MATCH_DOUBLES], m[SIM3_RANSAC_STAGED_DOUBLES];
      load_record<SIM3_RANSAC_MATCH_DOUBLES>(rec + (size_t)i * SIM3_RANSAC_MATCH_DOUBLES, v);
      sim3_ransac_stage(v, intr, m);
      a.inlier[m0 + i] = sim3_ransac_inlier(T, m, intr) ? 1 : 0;
    }
  } else {
    for (int i = lane; i < n; i += 64) a.inlier[m0 + i] = 0;
  }
  if (lane == 0) {
    a.found[f] = r.found;
    a.hyp[f] = r.hyp;
    a.iterations[f] = r.iterations;
    a.n_inliers[f] = r.n_inliers;
#pragma unroll
    for (int k = 0; k < 8; k++) a.S_out[8 * (size_t)f + k] = r.S12[k];
  }
}

}  // namespace

void sim3_ransac_launch(const Sim3RansacLaunch& a, bool inspect, hipStream_t st) {
  if (a.n_pairs <= 0) return;
  const int blocks = (a.n_pairs + SIM3_RANSAC_WAVES_PER_BLOCK - 1) / SIM3_RANSAC_WAVES_PER_BLOCK;
  if (inspect) hipLaunchKernelGGL(sim3_ransac_kernel<true>, dim3(blocks), dim3(64 * SIM3_RANSAC_WAVES_PER_BLOCK), 0, st, a);
  else hipLaunchKernelGGL(sim3_ransac_kernel<false>, dim3(blocks), dim3(64 * SIM3_RANSAC_WAVES_PER_BLOCK), 0, st, a);
}

}  // namespace cs
