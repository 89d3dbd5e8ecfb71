// sim3_pair_kernels.hip -- Sim(3) alignment of keyframe pairs, many pairs per launch (include/cubeslam_hip.h: cs_sim3_*).
//
// The arithmetic and the control flow are cs_sim3_pair.h's sim3_pair_optimize (the g2o lines it restates are cited there); this file
// gives it its wave: one wavefront per pair, the whole optimisation -- both rounds, every iteration and trial -- inside one launch, as
// pose_kernels.hip does for a frame.  Lane l owns the pair's matches l, l + 64, ...; its share of the 28 upper entries of H, of b and of
// chi2 is summed over the lanes by cs_wave.h's wave_sum_all (a butterfly: a fixed order, and the same bits in every lane), so every lane holds the same system, runs the same 7 x 7 factorisation and takes the
// same LM decisions: the control flow never diverges, and a pair's result is the same bits at any position in any batch.
//
// The 15 states of a linearisation (S, S (+) +-delta e_d, each with its inverse: 240 doubles) are wave-uniform.  Lanes 0..14 build one
// each and write it to the wave's own slice of LDS; every lane then reads them back as broadcasts, the matches in the outer loop and the
// seven dimensions inside.  A wave touches no other wave's slice and the kernel has no barrier: a wavefront whose pair does not exist
// leaves at once.  FP64, -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "cs_wave.h"
#include "sim3_pair_types.h"

namespace cs {
namespace {

// 17, not 16, doubles between two states: the 15 writers of one component then hit 15 different LDS banks
enum { STATE_PITCH = SIM3_PAIR_STATE_DOUBLES + 1, WAVE_LDS_DOUBLES = SIM3_PAIR_STATES * STATE_PITCH };

struct Wave64 {
  int lane, stride;
  double* st;                    // this wave's WAVE_LDS_DOUBLES of LDS
  __device__ __forceinline__ double sum(double v) const { return wave_sum_all(v); }
  __device__ __forceinline__ int sum(int v) const { return wave_sum_all(v); }
  __device__ __forceinline__ void put(int k, const double* v) {
#pragma unroll
    for (int j = 0; j < SIM3_PAIR_STATE_DOUBLES; j++) st[STATE_PITCH * k + j] = v[j];
  }
  __device__ __forceinline__ const double* get(int k) const { return st + STATE_PITCH * k; }
  __device__ __forceinline__ void load(const double* __restrict__ rec, double* v) const { load_record<SIM3_PAIR_MATCH_DOUBLES>(rec, v); }      // 144 bytes
  // one wave, program order: the fence keeps the compiler from moving LDS accesses across it
  // 240 doubles are not to live in VGPRs across the match loop: behind this fence the compiler reads the states from LDS again
  __device__ __forceinline__ void reread() const { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); }
  __device__ __forceinline__ void sync() const {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
};

__device__ __forceinline__ Sim3PairProblem pair_problem(const Sim3PairLaunch& a, int f, int& m0) {
  Sim3PairProblem F;
  m0 = a.match_ptr[f];
  F.n = a.match_ptr[f + 1] - m0;
  F.rec = a.rec + (size_t)m0 * SIM3_PAIR_MATCH_DOUBLES;
#pragma unroll
  for (int k = 0; k < 8; k++) F.intr[k] = a.intr[8 * (size_t)f + k];
  F.fix_scale = a.fix_scale[f] != 0;
  return F;
}

__global__ void __launch_bounds__(64 * SIM3_PAIR_WAVES_PER_BLOCK) sim3_pair_kernel(const Sim3PairLaunch a) {
  __shared__ double lds[SIM3_PAIR_WAVES_PER_BLOCK * WAVE_LDS_DOUBLES];
  const int f = blockIdx.x * SIM3_PAIR_WAVES_PER_BLOCK + (threadIdx.x >> 6);
  if (f >= a.n_pairs) return;                        // (a whole wavefront leaves: there is no barrier in this kernel)
  Wave64 w{(int)(threadIdx.x & 63), 64, lds + (threadIdx.x >> 6) * WAVE_LDS_DOUBLES};
  int m0;
  const Sim3PairProblem F = pair_problem(a, f, m0);
  Sim3 S = sim3_load(a.S0 + 8 * (size_t)f);          // Sim3 is never renormalised (cs_sim3.h)
  int iters[2], n_in;
  double chi[2];
  sim3_pair_optimize(w, F, a.sched, S, a.inlier + m0, iters, chi, n_in);
  if (w.lane == 0) {
    sim3_store(S, a.S_out + 8 * (size_t)f);
    a.iters_out[2 * f] = iters[0]; a.iters_out[2 * f + 1] = iters[1];
    a.chi2_out[2 * f] = chi[0]; a.chi2_out[2 * f + 1] = chi[1];
    a.n_inliers[f] = n_in;
  }
}

__global__ void __launch_bounds__(64 * SIM3_PAIR_WAVES_PER_BLOCK) sim3_pair_linearize_kernel(const Sim3PairLaunch a) {
  __shared__ double lds[SIM3_PAIR_WAVES_PER_BLOCK * WAVE_LDS_DOUBLES];
  const int f = blockIdx.x * SIM3_PAIR_WAVES_PER_BLOCK + (threadIdx.x >> 6);
  if (f >= a.n_pairs) return;
  Wave64 w{(int)(threadIdx.x & 63), 64, lds + (threadIdx.x >> 6) * WAVE_LDS_DOUBLES};
  int m0;
  const Sim3PairProblem F = pair_problem(a, f, m0);
  sim3_pair_inspect(w, F, sim3_load(a.S0 + 8 * (size_t)f), a.err + 4 * (size_t)m0, a.jac + 28 * (size_t)m0);
}

}  // namespace

void sim3_pair_launch(const Sim3PairLaunch& a, hipStream_t st) {
  if (a.n_pairs <= 0) return;
  const int blocks = (a.n_pairs + SIM3_PAIR_WAVES_PER_BLOCK - 1) / SIM3_PAIR_WAVES_PER_BLOCK;
  hipLaunchKernelGGL(sim3_pair_kernel, dim3(blocks), dim3(64 * SIM3_PAIR_WAVES_PER_BLOCK), 0, st, a);
}

void sim3_pair_launch_linearize(const Sim3PairLaunch& a, hipStream_t st) {
  if (a.n_pairs <= 0) return;
  const int blocks = (a.n_pairs + SIM3_PAIR_WAVES_PER_BLOCK - 1) / SIM3_PAIR_WAVES_PER_BLOCK;
  hipLaunchKernelGGL(sim3_pair_linearize_kernel, dim3(blocks), dim3(64 * SIM3_PAIR_WAVES_PER_BLOCK), 0, st, a);
}

}  // namespace cs
