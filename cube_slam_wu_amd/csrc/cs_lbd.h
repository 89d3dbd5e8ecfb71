// cs_lbd.h -- the arithmetic of the line band descriptor, one owner for the device kernel (lbd_kernels.hip), the host side
// (lbd_host.cpp) and the host-only check program (tools/hostonly/lbd_host_check.cpp):
//   BinaryDescriptor::computeLBD        line_lbd/libs/binary_descriptor.cpp:1150-1513   (default parameters: widthOfBand_ = 7, NUM_OF_BANDS = 9)
//   BinaryDescriptor::setWidthOfBand    :146-177    the Gaussian weights
//   combinations[32][2], binaryConversion  :74-107, :405-416, :769-773    the 32-byte binary form
// Nothing here iterates; every step is a fixed sequence of single-precision operations, and that sequence IS the contract (the std
// terms cancel, so no tolerance can define "right": tests/lbd_ref.py restates the same sequence in numpy float32 and everything is held to
// it bit for bit).  The rules:
//   Weights.      Computed in double on the host as :146-177 does -- with its integer divisions: u = (21 - 1) / 2 = 10, sigma = (14 + 1) / 2 = 7
//                 for the local weights, u = sigma = (63 - 1) / 2 = 31 for the global ones -- and rounded to float where the reference casts
//                 them (:1328, :1342, :1358, :1371).
//   Direction.    dL = ((float)cos((double)direction), (float)sin((double)direction)), libm, on the host, handed to the kernel per line (the
//                 reference's unqualified cos(float) is taken in its double form); dO = (-dL[1], dL[0]).
//   Start.        halfWidth = (numOfPixels - 1) / 2 (integer, towards zero), halfHeight = 31, lineMiddlePoint = (float)(0.5 * ((double)s + (double)e)),
//                 sCorX0 = -dL[0] * halfWidth + dL[1] * halfHeight + middleX, sCorY0 = -dL[1] * halfWidth - dL[0] * halfHeight + middleY, left to
//                 right in float (:1270-1271).
//   Walk.         Row h starts at sCor0 after h sequential updates sCorX0 -= dL[1]; sCorY0 += dL[0] (a running sum, not h * dL); along the row
//                 sCorX += dL[0]; sCorY += dL[1], a running sum too.  The pixel is roundf() (half away from zero) of the position, clamped to
//                 [0, W - 1] x [0, H - 1].  (The reference converts the rounded value to short before it clamps; the clamp is applied to the
//                 float here, which is the same wherever the short conversion is defined.)
//   Per pixel.    gDL = dx * dL[0] + dy * dL[1], gDO = dx * dO[0] + dy * dO[1]: two rounded products and one rounded sum, NO fused multiply-add
//                 (the Makefile's -ffp-contract=off).  The four row sums accumulate in pixel order wID = 0 .. numOfPixels - 1.
//   Bands.        A row contributes to its own band, then the band above, then the band below (:1341-1380); rows go in order hID = 0 .. 62, so each
//                 of a band's eight sums is a fixed sequence of at most 21 additions.  The squares are (c * c) * (row * row), as written.
//   sqrt, 1 / x.  sqrtf is the correctly rounded one, 1 / sqrtf(x) is that followed by a correctly rounded division: no rsq, no fast division,
//                 no fast-math flag (hipcc's default for gfx950 lowers both to the refined sequences).
//   Normalising.  tempM, tempS and the final temp accumulate in the element order of :1430-1440 and :1473-1476.
//   Clamp.        desVec[i] > 0.4 compares against the DOUBLE 0.4 and stores 0.4f.  A NaN stays NaN.
//   NaN.          Real behaviour, kept: a flat support region gives 1 / sqrt(0) = inf, 0 * inf = NaN, all 72 floats NaN, every comparison false,
//                 32 zero bytes.  A variance that rounds below zero gives NaN in the std half only.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace cs {

enum { LBD_BAND_W = 7, LBD_BANDS = 9, LBD_ROWS = LBD_BAND_W * LBD_BANDS, LBD_FLOATS = 8 * LBD_BANDS, LBD_BYTES = 32 };

// gaussCoefG_ (63) and gaussCoefL_ (21), each rounded to float where the reference reads it
struct LbdWeights { float g[LBD_ROWS], l[3 * LBD_BAND_W]; };

inline void lbd_weights(LbdWeights& w) {
  double u = (double)((LBD_BAND_W * 3 - 1) / 2);
  double sigma = (double)((LBD_BAND_W * 2 + 1) / 2);
  double invsigma2 = -1 / (2 * sigma * sigma);
  for (int i = 0; i < LBD_BAND_W * 3; i++) { const double dis = i - u; w.l[i] = (float)std::exp(dis * dis * invsigma2); }
  u = (double)((LBD_BANDS * LBD_BAND_W - 1) / 2);
  sigma = u;
  invsigma2 = -1 / (2 * sigma * sigma);
  for (int i = 0; i < LBD_ROWS; i++) { const double dis = i - u; w.g[i] = (float)std::exp(dis * dis * invsigma2); }
}

// One line as the kernel takes it: direction vector, first pixel position of support row 0, length of the support region.
struct LbdLine { float dl0, dl1, x0, y0; int n; int image; };

// the host half of a line's set-up (libm cos / sin in double; the start of the support region, :1250-1271)
inline LbdLine lbd_line(float sx, float sy, float ex, float ey, float direction, int num_pixels, int image) {
  LbdLine L;
  L.dl0 = (float)std::cos((double)direction);
  L.dl1 = (float)std::sin((double)direction);
  const short half_w = (short)((num_pixels - 1) / 2), half_h = (short)((LBD_ROWS - 1) / 2);
  const float mx = (float)(0.5 * ((double)sx + (double)ex)), my = (float)(0.5 * ((double)sy + (double)ey));
  const float a = -L.dl0 * (float)half_w, b = L.dl1 * (float)half_h;
  L.x0 = (a + b) + mx;
  const float c = -L.dl1 * (float)half_w, d = L.dl0 * (float)half_h;
  L.y0 = (c - d) + my;
  L.n = num_pixels;
  L.image = image;
  return L;
}

// The detector's packed map (lines_types.h): three bytes per pixel, dx in bits 0..10, dy in bits 12..22, both two's complement.
struct LbdMapP3 {
  const unsigned char* p3;
  __host__ __device__ void at(size_t i, float& dx, float& dy) const {
    const unsigned char* q = p3 + 3 * i;
    const unsigned w = (unsigned)q[0] | ((unsigned)q[1] << 8) | ((unsigned)q[2] << 16);
    dx = (float)((int)(w << 21) >> 21);
    dy = (float)((int)(w << 9) >> 21);
  }
};
// plain short planes (the host-only check program)
struct LbdMapPlanes {
  const short *dx_, *dy_;
  __host__ __device__ void at(size_t i, float& dx, float& dy) const { dx = (float)dx_[i]; dy = (float)dy_[i]; }
};

// one step of the walk along a row: the pixel under (x, y) -- roundf, clamped into the map -- and the running sum to the next position
template <class Map>
__host__ __device__ inline void lbd_gather(const Map& m, int W, int H, float dl0, float dl1, float& x, float& y, float& dx, float& dy) {
  const float rx = roundf(x), ry = roundf(y), xmax = (float)(W - 1), ymax = (float)(H - 1);
  const int xc = rx > 0 ? (rx > xmax ? W - 1 : (int)rx) : 0, yc = ry > 0 ? (ry > ymax ? H - 1 : (int)ry) : 0;     // (never out of the map, whatever x is)
  m.at((size_t)yc * (size_t)W + (size_t)xc, dx, dy);
  x = x + dl0; y = y + dl1;
}
// one pixel into the four row sums s = pgdL, ngdL, pgdO, ngdO
__host__ __device__ inline void lbd_accumulate(float dx, float dy, float dl0, float dl1, float s[4]) {
  const float do0 = -dl1, do1 = dl0;
  const float a = dx * dl0, b = dy * dl1, gl = a + b;
  const float c = dx * do0, d = dy * do1, go = c + d;
  if (gl > 0) s[0] = s[0] + gl; else s[1] = s[1] - gl;
  if (go > 0) s[2] = s[2] + go; else s[3] = s[3] - go;
}

// support row h of a line: the start after h running updates, then the walk.  out: pgdL, ngdL, pgdO, ngdO row sums, unweighted.
// The positions are a running sum of their own and the gathers depend on nothing but them, so four are issued ahead; the sums then take the
// four values in pixel order.
template <class Map>
__host__ __device__ inline void lbd_row_sums(const Map& m, int W, int H, const LbdLine& L, int h, float out[4]) {
  enum { AHEAD = 4 };
  float x = L.x0, y = L.y0;
  for (int k = 0; k < h; k++) { x = x - L.dl1; y = y + L.dl0; }
  out[0] = 0; out[1] = 0; out[2] = 0; out[3] = 0;
  int w = 0;
  for (; w + AHEAD <= L.n; w += AHEAD) {
    float dx[AHEAD], dy[AHEAD];
    for (int k = 0; k < AHEAD; k++) lbd_gather(m, W, H, L.dl0, L.dl1, x, y, dx[k], dy[k]);
    for (int k = 0; k < AHEAD; k++) lbd_accumulate(dx[k], dy[k], L.dl0, L.dl1, out);
  }
  for (; w < L.n; w++) {
    float dx, dy;
    lbd_gather(m, W, H, L.dl0, L.dl1, x, y, dx, dy);
    lbd_accumulate(dx, dy, L.dl0, L.dl1, out);
  }
}

// Band b: its eight sums over the rows of bands b - 1 (weight l[h % 7], "the band below" of those rows), b (l[h % 7 + 7]) and b + 1
// (l[h % 7 + 14], "the band above") in row order, then mean / std (:1394-1421) into des[8 b .. 8 b + 7].  rows: [63][4] as lbd_row_sums writes them.
__host__ __device__ inline void lbd_band(const float* rows, const float* wg, const float* wl, int b, float* des) {
  float pl = 0, nl = 0, pl2 = 0, nl2 = 0, po = 0, no = 0, po2 = 0, no2 = 0;
  const int h_begin = b > 0 ? (b - 1) * LBD_BAND_W : 0, h_end = b < LBD_BANDS - 1 ? (b + 2) * LBD_BAND_W : LBD_ROWS;
  for (int h = h_begin; h < h_end; h++) {
    const int hb = h / LBD_BAND_W, r = h - hb * LBD_BAND_W;
    const float g = wg[h];
    const float rpl = g * rows[4 * h], rnl = g * rows[4 * h + 1], rpo = g * rows[4 * h + 2], rno = g * rows[4 * h + 3];
    const float rpl2 = rpl * rpl, rnl2 = rnl * rnl, rpo2 = rpo * rpo, rno2 = rno * rno;
    const float c = wl[hb == b ? r + LBD_BAND_W : (hb > b ? r + 2 * LBD_BAND_W : r)];
    const float cc = c * c;
    pl = pl + c * rpl; nl = nl + c * rnl;
    pl2 = pl2 + cc * rpl2; nl2 = nl2 + cc * rnl2;
    po = po + c * rpo; no = no + c * rno;
    po2 = po2 + cc * rpo2; no2 = no2 + cc * rno2;
  }
  const float inv_n = (b == 0 || b == LBD_BANDS - 1) ? (float)(1.0 / (LBD_BAND_W * 2.0)) : (float)(1.0 / (LBD_BAND_W * 3.0));
  float* d = des + 8 * b;
  float t;
  t = pl * inv_n; d[0] = t; { const float q = pl2 * inv_n, s = t * t; d[4] = sqrtf(q - s); }
  t = nl * inv_n; d[1] = t; { const float q = nl2 * inv_n, s = t * t; d[5] = sqrtf(q - s); }
  t = po * inv_n; d[2] = t; { const float q = po2 * inv_n, s = t * t; d[6] = sqrtf(q - s); }
  t = no * inv_n; d[3] = t; { const float q = no2 * inv_n, s = t * t; d[7] = sqrtf(q - s); }
}

// the two normalisations, the clamp at 0.4 and the re-normalisation (:1423-1482), in place on the 72 floats
__host__ __device__ inline void lbd_normalise(float* des) {
  float tm = 0, ts = 0;
  for (int i = 0; i < LBD_FLOATS; i += 8) {
    for (int k = 0; k < 4; k++) { const float p = des[i + k] * des[i + k]; tm = tm + p; }
    for (int k = 4; k < 8; k++) { const float p = des[i + k] * des[i + k]; ts = ts + p; }
  }
  tm = 1.0f / sqrtf(tm);
  ts = 1.0f / sqrtf(ts);
  for (int i = 0; i < LBD_FLOATS; i++) {
    float v = des[i] * ((i & 4) ? ts : tm);
    if ((double)v > 0.4) v = 0.4f;
    des[i] = v;
  }
  float t = 0;
  for (int i = 0; i < LBD_FLOATS; i++) { const float p = des[i] * des[i]; t = t + p; }
  t = 1.0f / sqrtf(t);
  for (int i = 0; i < LBD_FLOATS; i++) des[i] = des[i] * t;
}

// byte `comb` of the binary descriptor: bit i = des[8 a + i] > des[8 b + i] for the comb-th pair (a, b), a < b, in the order of
// combinations[32][2]: (0, 1..6), (1, 2..6), (2, 3..8), (3, 4..8), (4, 5..8), (5, 6..8), (6, 7..8), (7, 8)
__host__ __device__ inline void lbd_pair(int comb, int& a, int& b) {
  const int first[8] = {0, 6, 11, 17, 22, 26, 29, 31}, second[8] = {1, 2, 3, 4, 5, 6, 7, 8};
  a = 0;
  for (int k = 1; k < 8; k++) if (comb >= first[k]) a = k;
  b = second[a] + (comb - first[a]);
}
__host__ __device__ inline unsigned char lbd_binary_byte(const float* des, int comb) {
  int a, b;
  lbd_pair(comb, a, b);
  unsigned r = 0;
  for (int i = 0; i < 8; i++) if (des[8 * a + i] > des[8 * b + i]) r |= 1u << i;
  return (unsigned char)r;
}

// one line start to end in a plain loop: what the kernel computes with one lane per row (the check program; tests)
template <class Map>
inline void lbd_describe_one(const Map& m, int W, int H, const LbdLine& L, const LbdWeights& w, float des72[LBD_FLOATS], unsigned char desc32[LBD_BYTES]) {
  float rows[4 * LBD_ROWS];
  for (int h = 0; h < LBD_ROWS; h++) lbd_row_sums(m, W, H, L, h, rows + 4 * h);
  for (int b = 0; b < LBD_BANDS; b++) lbd_band(rows, w.g, w.l, b, des72);
  lbd_normalise(des72);
  for (int c = 0; c < LBD_BYTES; c++) desc32[c] = lbd_binary_byte(des72, c);
}

}  // namespace cs
