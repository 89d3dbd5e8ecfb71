// cs_atan2_float.h -- atan2 in single precision for DECISIONS of the sweep's kernels (vp_step in detect_kernels.hip, the pair tests
// of line_setup_kernels.hip): the caller compares inside a margin and decides exactly with cs_atan2 where the float cannot tell.
#pragma once
#include <hip/hip_runtime.h>

namespace cs {

// atan2 in float, all quadrants: |error| < 2.5e-6 rad (tests/test_device_decisions.py; budget in the comment above vp_step's helpers).
// *usable = false for a zero or non-finite argument pair: the caller then decides exactly.
__device__ __forceinline__ float atan2_float(float fy, float fx, bool* usable) {
  const float PI_F = 3.14159274f, HPI_F = 1.57079637f;
  const float ay = fabsf(fy), ax = fabsf(fx);
  const float hi = fmaxf(ax, ay), lo = fminf(ax, ay);
  const float q = lo * __builtin_amdgcn_rcpf(hi), q2 = q * q;
  float at = -0.01172120f;
  at = __builtin_fmaf(at, q2, 0.05265332f);
  at = __builtin_fmaf(at, q2, -0.11643287f);
  at = __builtin_fmaf(at, q2, 0.19354346f);
  at = __builtin_fmaf(at, q2, -0.33262347f);
  at = __builtin_fmaf(at, q2, 0.99997726f);
  at = at * q;
  if (ay > ax) at = HPI_F - at;
  if (fx < 0.0f) at = PI_F - at;
  if (fy < 0.0f) at = -at;
  *usable = hi > 0.0f && hi < 3.0e38f;
  return at;
}

}  // namespace cs
