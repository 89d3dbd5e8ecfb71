// lines_types.h -- what lines_host.cpp hands to lines_kernels.hip (the per-pixel stages of the EDLines branch of the line-segment producer).
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace cs {

// What goes back to the host, THREE bytes per pixel (round 6; a 32-bit word until then -- the copy back is the batch's longest stage): the Sobel
// derivatives (dxImg_, dyImg_; |.| <= 4 x 255 = 1020: eleven bits each) and the anchor flag, little endian,
//   bits 0..10  dx (two's complement)        bit 11  anchor        bits 12..22  dy (two's complement)        bit 23  0
// i.e. bits 11..22 are 2 dy + anchor as before.  The thresholded gradient / 4 (gImg_) and the direction map (dirImg_: |dx| < |dy| = horizontal) are
// functions of dx and dy that the host stage evaluates where it reads them (lines_host.cpp, Maps).  Image i's map starts at p3 + 3 N i.
struct LineMaps {
  unsigned char* p3;
};

// per kept segment, beside its end points: EDLineDetector's lineDirection_ and the number of chain pixels the fitted line kept
struct LineExtra { float direction; int num_pixels; };

// the blur's taps: getGaussianKernel(5, 1.0, CV_32F) rounded to 8-bit fixed point, as createSeparableLinearFilter does for 8-bit images (k[2] is the centre)
inline void lines_blur_taps(int k[3]) {
  float cf[5]; double sum = 0;
  for (int i = 0; i < 5; i++) { const double x = i - 2.0; cf[i] = (float)std::exp(-0.5 * x * x); sum += cf[i]; }
  sum = 1. / sum;
  for (int i = 0; i < 3; i++) k[i] = (int)std::nearbyint((double)(float)(cf[i] * sum) * 256.0);
}

void launch_lines_maps(const unsigned char* gray, int W, int H, const LineMaps& m, const int k[3], int grad_thr, int anchor_thr, int scan, hipStream_t st, int n_images);

}  // namespace cs
