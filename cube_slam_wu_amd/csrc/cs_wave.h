// cs_wave.h -- the two device-side pieces the BA kernels and the reduced-system solvers share (ba_kernels.hip, band_kernels.hip,
// bcr_kernels.hip): the wavefront sum and the accumulator type of v_mfma_f64_16x16x4_f64.
#pragma once
#include <hip/hip_runtime.h>

namespace cs {

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  return v;
}

typedef double ba_v4d __attribute__((ext_vector_type(4)));

}  // namespace cs
