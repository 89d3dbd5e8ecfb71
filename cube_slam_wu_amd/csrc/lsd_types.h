// lsd_types.h -- what lsd_host.cpp hands to lsd_kernels.hip (the per-pixel stages of the LSD branch of the line-segment producer).
#pragma once
#include <hip/hip_runtime.h>

namespace cs {

struct LsdGauss { double k[7]; };                  // getGaussianKernel(7, 0.75, CV_64F)
struct LsdScaleTab {                               // resize's per-column / per-row source offsets and weights (computed on the host)
  const int* xo; const float* xa;                  // W_s offsets, 2 W_s weights
  const int* yo; const float* ya;                  // H_s offsets, 2 H_s weights
};

void launch_lsd_maps(const unsigned char* gray, int W, int H, int Ws, int Hs, const LsdGauss& G, const LsdScaleTab& T, double rho, double* blur, char* out, size_t out_stride, hipStream_t st, int n_images);

}  // namespace cs
