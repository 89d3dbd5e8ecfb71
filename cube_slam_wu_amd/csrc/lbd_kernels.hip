// lbd_kernels.hip -- line band descriptors and their Hamming matching on the device (gfx950, wave64):
//   BinaryDescriptor::computeLBD + binaryConversion   line_lbd/libs/binary_descriptor.cpp:1150-1513, :405-416, :769-773
//   BinaryDescriptorMatcher::match                    (brute force here: the same distances and set of minimisers, ties to the lowest train row)
// The arithmetic is cs_lbd.h's, which states the numerical contract; this file only deals the work to lanes.
//   lbd_describe_kernel   one wavefront per line.  Lane h < 63 walks support row h of the detector's resident packed map (the gathers do not depend on
//                         the accumulators; the sums do, and keep the reference's order); the 63 x 4 row sums go through LDS to lanes 0..8, which own a
//                         band each and form its eight ordered sums, mean and std; lane 0 normalises the 72 floats in order (nothing is tree-reduced);
//                         lanes 0..31 form a byte of the binary descriptor each.
//   lbd_match_kernel      lanes are queries (8 words in registers); the train rows pass through LDS in tiles of 64 and are read as broadcasts, 8 popcounts
//                         a pair; each lane keeps the smallest distance, its train row and the second-smallest distance.
// All stores are ordinary vector stores.
#include <hip/hip_runtime.h>

#include "lbd_types.h"

namespace cs {

__global__ __launch_bounds__(64) void lbd_describe_kernel(const unsigned char* __restrict__ p3, int W, int H, const LbdLine* __restrict__ lines, int n,
                                                          const LbdWeights* __restrict__ weights, unsigned char* __restrict__ desc32, float* __restrict__ desc72) {
  __shared__ float rows[4 * LBD_ROWS];
  __shared__ float des[LBD_FLOATS];
  __shared__ LbdWeights w;
  const int line = blockIdx.x, lane = threadIdx.x;
  if (line >= n) return;                                  // (uniform over the workgroup)
  {
    const float* src = (const float*)weights;
    float* dst = (float*)&w;
    for (int i = lane; i < (int)(sizeof(LbdWeights) / sizeof(float)); i += 64) dst[i] = src[i];
  }
  const LbdLine L = lines[line];
  if (lane < LBD_ROWS) {
    const LbdMapP3 m{p3 + 3 * (size_t)W * (size_t)H * (size_t)L.image};
    float r[4];
    lbd_row_sums(m, W, H, L, lane, r);
    rows[4 * lane] = r[0]; rows[4 * lane + 1] = r[1]; rows[4 * lane + 2] = r[2]; rows[4 * lane + 3] = r[3];
  }
  __syncthreads();
  if (lane < LBD_BANDS) lbd_band(rows, w.g, w.l, lane, des);
  __syncthreads();
  if (lane == 0) lbd_normalise(des);
  __syncthreads();
  if (lane < LBD_BYTES) desc32[(size_t)line * LBD_BYTES + lane] = lbd_binary_byte(des, lane);
  if (desc72) {
    float* o = desc72 + (size_t)line * LBD_FLOATS;
    o[lane] = des[lane];
    if (lane + 64 < LBD_FLOATS) o[lane + 64] = des[lane + 64];
  }
}

void launch_lbd_describe(const unsigned char* p3, int W, int H, const LbdLine* lines, int n, const LbdWeights* weights, unsigned char* desc32, float* desc72, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(lbd_describe_kernel, dim3((unsigned)n), dim3(64), 0, st, p3, W, H, lines, n, weights, desc32, desc72);
}

enum { MATCH_TILE = 64 };

// blockIdx.y = pair, blockIdx.x = tile of 64 queries of that pair
__global__ __launch_bounds__(64) void lbd_match_kernel(const unsigned* __restrict__ q32, const int* __restrict__ q_ptr, const unsigned* __restrict__ t32, const int* __restrict__ t_ptr,
                                                       int pair0, int* __restrict__ train_idx, int* __restrict__ dist, int* __restrict__ dist2) {
  __shared__ unsigned tile[MATCH_TILE][8];
  const int pair = pair0 + blockIdx.y, lane = threadIdx.x;
  const int q0 = q_ptr[pair], nq = q_ptr[pair + 1] - q0, t0 = t_ptr[pair], nt = t_ptr[pair + 1] - t0;
  if ((int)blockIdx.x * MATCH_TILE >= nq) return;         // (uniform over the workgroup)
  const int qi = blockIdx.x * MATCH_TILE + lane;
  const bool live = qi < nq;
  unsigned q[8];
  for (int k = 0; k < 8; k++) q[k] = live ? q32[8 * (size_t)(q0 + qi) + k] : 0u;
  int best = 1 << 20, second = 1 << 20, best_at = -1;
  for (int base = 0; base < nt; base += MATCH_TILE) {
    const int nb = nt - base < MATCH_TILE ? nt - base : MATCH_TILE;
    __syncthreads();
    if (lane < nb) for (int k = 0; k < 8; k++) tile[lane][k] = t32[8 * (size_t)(t0 + base + lane) + k];
    __syncthreads();
    for (int j = 0; j < nb; j++) {
      int d = 0;
      for (int k = 0; k < 8; k++) d += __popc(q[k] ^ tile[j][k]);
      if (d < best) { second = best; best = d; best_at = base + j; }
      else if (d < second) second = d;
    }
  }
  if (live) {
    const size_t o = (size_t)(q0 + qi);
    train_idx[o] = best_at;
    dist[o] = nt > 0 ? best : -1;
    if (dist2) dist2[o] = nt > 1 ? second : -1;
  }
}

void launch_lbd_match(int n_pairs, int max_nq, const unsigned* q32, const int* q_ptr, const unsigned* t32, const int* t_ptr, int* train_idx, int* dist, int* dist2, hipStream_t st) {
  if (n_pairs <= 0 || max_nq <= 0) return;
  const unsigned tiles = (unsigned)((max_nq + MATCH_TILE - 1) / MATCH_TILE);
  for (int p0 = 0; p0 < n_pairs; p0 += 65535) {           // gridDim.y limit
    const int np = n_pairs - p0 < 65535 ? n_pairs - p0 : 65535;
    hipLaunchKernelGGL(lbd_match_kernel, dim3(tiles, (unsigned)np), dim3(64), 0, st, q32, q_ptr, t32, t_ptr, p0, train_idx, dist, dist2);
  }
}

}  // namespace cs
