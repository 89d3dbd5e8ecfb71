// lbd_types.h -- what lbd_host.cpp hands to lbd_kernels.hip (line band descriptors and their Hamming matching).
#pragma once
#include <hip/hip_runtime.h>

#include "cs_lbd.h"

namespace cs {

// lbd_describe_kernel: one wavefront per line.  lines[i].image selects the packed map p3 + 3 N image (N = W H; the layout of lines_types.h).
// desc32: n x 32 bytes; desc72: n x 72 floats or null.  weights: one LbdWeights on the device.
void launch_lbd_describe(const unsigned char* p3, int W, int H, const LbdLine* lines, int n, const LbdWeights* weights, unsigned char* desc32, float* desc72, hipStream_t st);

// lbd_match_kernel: n_pairs (query set, train set) pairs in CSR form -- pair p's queries are rows q_ptr[p] .. q_ptr[p + 1] of q32 (8 words a row),
// its train rows t_ptr[p] .. t_ptr[p + 1] of t32.  Per query row: the nearest train row's index within its set (-1: empty set), the distance
// (-1: empty set) and the second-smallest distance (-1: fewer than two train rows).  Ties go to the lowest train index.  max_nq: the largest query set.
void launch_lbd_match(int n_pairs, int max_nq, const unsigned* q32, const int* q_ptr, const unsigned* t32, const int* t_ptr, int* train_idx, int* dist, int* dist2, hipStream_t st);

}  // namespace cs
