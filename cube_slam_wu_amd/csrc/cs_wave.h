// cs_wave.h -- the device-side pieces the kernels share: the two wavefront sums (ba_kernels.hip, band_kernels.hip, bcr_kernels.hip use the
// one for lane 0; pose_kernels.hip and sim3_pair_kernels.hip the one for every lane), the aligned record load of the batch kernels, the
// prologue of the chunked ones (triangulate_kernels.hip, orb_search_kernels.hip), and the accumulator type of v_mfma_f64_16x16x4_f64.
#pragma once
#include <hip/hip_runtime.h>

#include "cs_chunk.h"

namespace cs {

// the total is valid in lane 0 only
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

// The total in EVERY lane, by a butterfly (lane ^ 32, ^ 16, ... ^ 1): a fixed order, and -- both partners add the same two numbers -- the
// same bits in every lane, so that what is computed from it needs no broadcast.  T = double or int.
template <class T>
__device__ __forceinline__ T wave_sum_all(T v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// A record of N doubles (N even) behind a 16-byte aligned address, read as double2s (the hosts pack the records behind a 256-byte aligned
// base, and a record is a multiple of 16 bytes)
template <int N>
__device__ __forceinline__ void load_record(const double* __restrict__ rec, double* v) {
  static_assert(N % 2 == 0, "a record is read two doubles at a time");
  const double2* p = reinterpret_cast<const double2*>(rec);
#pragma unroll
  for (int k = 0; k < N / 2; k++) { const double2 t = p[k]; v[2 * k] = t.x; v[2 * k + 1] = t.y; }
}

// The prologue of a kernel that gives every wavefront one chunk and every lane one item of it (blocks of WAVES wavefronts, no barrier):
// false = leave -- the whole wavefront when there is no chunk for it, a lane when it is past the chunk's count.  `ch` is wave-uniform.
template <int WAVES>
__device__ __forceinline__ bool wave_chunk(const Chunk* chunk, int n_chunks, Chunk& ch, int& lane) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c = blockIdx.x * WAVES + wave;
  if (c >= n_chunks) return false;
  ch = chunk[c];
  lane = threadIdx.x & 63;
  return lane < ch.count;
}

typedef double ba_v4d __attribute__((ext_vector_type(4)));

}  // namespace cs
