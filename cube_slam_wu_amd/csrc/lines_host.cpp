// lines_host.cpp -- the line-segment producer behind the C ABI:
//   line_lbd_detect::detect_filter_lines(gray, lines)     line_lbd/class/line_lbd_allclass.cpp:199-235   (use_LSD = false: EDLines;
//                                                          the graph driver sets line_length_thres = 15, object_slam/src/main_obj.cpp:504-505)
// i.e. BinaryDescriptor::detect -> OctaveKeyLines -> EDLineDetector::EDline (libs/binary_descriptor.cpp:421-590, :796-1148, :1583-2905),
// one octave.  The per-pixel stages (Gaussian blur, Sobel, gradient / direction maps, anchors) run on the device
// (csrc/lines_kernels.hip); what is sequential by definition stays here:
//   smart routing   (EdgeDrawing :1672-2381)   anchors in column-major scan order, two routed walks per anchor, chains under 16 pixels dropped
//   line extraction (EDline :2383-2630)        least-squares fit of the first 15 pixels, extension with at most 3 consecutive outliers,
//                                              refits from running float normal equations (the reference's Mat_<float> members)
//   validation      (LineValidation_ :2793-2874, nfa descriptor.hpp:764-848), end points, start / end order (OctaveKeyLines :1074-1143)
// The arithmetic follows the reference operation for operation (same types: float normal-equation terms, double solve, float end points);
// tests/test_lines_gpu.py holds it to the CPU restatement of the same detector bit for bit.  No CPU fallback for the device stages.
// How a batch of images goes through the device and the worker pool is cs_image_batch.h's business (shared with lsd_host.cpp): this file supplies
// the scratch, what to launch for a run of images, and the host stage of one image.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cubeslam_hip.h"
#include "cs_hip_util.h"
#include "cs_image_batch.h"
#include "cs_nfa.h"
#include "detect_hooks.h"
#include "lines_types.h"

namespace {

// EDLineDetector() :1515-1526 and BinaryDescriptor::Params() :110-117
struct EdParams { int grad_thr = 80, anchor_thr = 8, scan = 2, min_len = 15, try_time = 6, skip = 2, max_outlier = 3; double fit_err = 1.6; };

// Host copy of the device's packed map (pinned staging of the detector's scratch): one word per pixel = dx | (2 dy + anchor) << 16
// (lines_kernels.hip).  The reference's gImg_ and dirImg_ are functions of dx and dy, evaluated where they are read:
//   gImg_ = cvRound((|dx| + |dy| thresholded at gradienThreshold_ + 1) / 4)     binary_descriptor.cpp:1630-1640
//   dirImg_ = |dx| < |dy| ? Horizontal : Vertical
struct Maps {
  int W = 0, H = 0, grad_thr = 0;
  const unsigned char* p3 = nullptr;      // three bytes per pixel (lines_kernels.hip, LineMaps): dx | anchor << 11 | dy << 12; readable up to p3 + 3 N + 1
  unsigned word(size_t at) const { unsigned w; std::memcpy(&w, p3 + 3 * at, 4); return w; }      // (the fourth byte is the next pixel's, or the pad)
  int dx(size_t at) const { return (int)(word(at) << 21) >> 21; }
  int dy(size_t at) const { return (int)(word(at) << 9) >> 21; }
  bool anchor(size_t at) const { return (p3[3 * at + 1] >> 3) & 1; }
  short g(size_t at) const {
    const int s = std::abs(dx(at)) + std::abs(dy(at)), v = s > grad_thr + 1 ? s : 0, q = v >> 2, r = v & 3;
    return (short)(q + ((r == 3) || (r == 2 && (q & 1))));        // round half to even
  }
  bool horizontal(size_t at) const { return std::abs(dx(at)) < std::abs(dy(at)); }
  bool horizontal(unsigned x, unsigned y) const { return horizontal((size_t)y * W + x); }
};

// the 32-bit packing of the CPU restatement's map (dx | (2 dy + anchor) << 16) in the device's three bytes (tools/hostonly, tests)
inline void maps_pack3(const int* pk, size_t n, std::vector<unsigned char>& out) {
  out.assign(3 * n + 4, 0);
  for (size_t i = 0; i < n; i++) {
    const unsigned wd = (((unsigned)(pk[i] >> 16) & 0xfffu) << 11) | ((unsigned)pk[i] & 0x7ffu);
    out[3 * i] = (unsigned char)wd; out[3 * i + 1] = (unsigned char)(wd >> 8); out[3 * i + 2] = (unsigned char)(wd >> 16);
  }
}

struct Chain { std::vector<unsigned> x, y; };

// ---- smart routing ---------------------------------------------------------------------------------------------------------
// A walk advances one pixel per step in one of four headings.  Per heading: the three candidate neighbours in the order the
// reference compares them (first, straight, third) and the image sides that end the walk.
enum Heading { UP = 1, RIGHT = 2, DOWN = 3, LEFT = 4 };
struct Step { int dx[3], dy[3]; };
static const Step kStep[5] = {
    {{0, 0, 0}, {0, 0, 0}},
    {{+1, 0, -1}, {-1, -1, -1}},   // up:    up-right, up, up-left
    {{+1, +1, +1}, {-1, 0, +1}},   // right: up-right, right, down-right
    {{+1, 0, -1}, {+1, +1, +1}},   // down:  down-right, down, down-left
    {{-1, -1, -1}, {-1, 0, +1}},   // left:  up-left, left, down-left
};

struct Router {
  const Maps& M;
  std::vector<unsigned char> taken;
  unsigned last_x = 0, last_y = 0;   // where the previous step stood (they outlive a walk, as in the reference)
  explicit Router(const Maps& m) : M(m), taken((size_t)m.W * m.H, 0) {}

  void walk(unsigned x, unsigned y, int heading, Chain& out) {
    const unsigned W = M.W, H = M.H;
    for (;;) {
      const size_t at = (size_t)y * W + x;
      if (!(M.g(at) > 0) || taken[at]) return;
      taken[at] = 1;
      out.x.push_back(x); out.y.push_back(y);
      int go;
      if (M.horizontal(at)) go = (heading == UP || heading == DOWN) ? (x > last_x ? RIGHT : LEFT) : heading;     // horizontal pixel: left or right
      else                  go = (heading == RIGHT || heading == LEFT) ? (y > last_y ? DOWN : UP) : heading;     // vertical pixel: up or down
      last_x = x; last_y = y;
      const bool at_border = go == RIGHT ? (x == W - 1 || y == 0 || y == H - 1)
                           : go == LEFT  ? (x == 0 || y == 0 || y == H - 1)
                           : go == DOWN  ? (x == 0 || x == W - 1 || y == H - 1)
                                         : (x == 0 || x == W - 1 || y == 0);
      if (at_border) return;
      const Step& s = kStep[go];
      unsigned char gv[3];   // the reference compares the gradients as unsigned char (values above 255 wrap)
      for (int q = 0; q < 3; q++) gv[q] = (unsigned char)M.g((size_t)(y + s.dy[q]) * W + (x + s.dx[q]));
      const int pick = (gv[0] >= gv[1] && gv[0] >= gv[2]) ? 0 : ((gv[2] >= gv[1] && gv[2] >= gv[0]) ? 2 : 1);
      x += s.dx[pick]; y += s.dy[pick];
      heading = go;
    }
  }
};

// ---- running least squares: value = a * coord + b with float normal-equation terms (Mat_<float> ATA, ATV) ---------------------
struct NormalEq {
  float a00 = 0, a01 = 0, a11 = 0, v0 = 0, v1 = 0;
  // the terms of a block of pixels: sums in double, stored as float (cv::gemm on CV_32F)
  static NormalEq of(const unsigned* coord, const unsigned* value, int n) {
    double s00 = 0, s01 = 0, t0 = 0, t1 = 0;
    for (int i = 0; i < n; i++) { const double c = (double)coord[i], v = (double)value[i]; s00 += c * c; s01 += c; t0 += c * v; t1 += v; }
    NormalEq r; r.a00 = (float)s00; r.a01 = (float)s01; r.a11 = (float)(double)n; r.v0 = (float)t0; r.v1 = (float)t1;
    return r;
  }
  void add(const NormalEq& o) { a00 = a00 + o.a00; a01 = a01 + o.a01; a11 = a11 + o.a11; v0 = v0 + o.v0; v1 = v1 + o.v1; }
  void solve(double& a, double& b) const {
    const double det_inv = 1.0 / ((double)a00 * (double)a11 - (double)a01 * (double)a01);
    a = det_inv * ((double)a11 * (double)v0 - (double)a01 * (double)v1);
    b = det_inv * ((double)a00 * (double)v1 - (double)a01 * (double)v0);
  }
};

// number of false alarms (descriptor.hpp:650-848): cs_nfa.h, with the log-gamma first term
double minus_log10_nfa(int n, int k, double p, double logNT) { return cs::minus_log10_nfa(n, k, p, logNT, true); }

struct Segment { float x1, y1, x2, y2, direction; int n_pixels; };     // n_pixels: chain pixels the fitted line kept (lines_.sId[k + 1] - lines_.sId[k], :2442-2626)

// ---- line extraction from the chains ------------------------------------------------------------------------------------------
struct Extractor {
  const Maps& M;
  const EdParams& P;
  double logNT;
  std::vector<unsigned> lx, ly;     // pixels of the line being grown
  Extractor(const Maps& m, const EdParams& p) : M(m), P(p), logNT(2.0 * (std::log10((double)m.W) + std::log10((double)m.H))) {}

  // gradient orientation statistics + border test + NFA (LineValidation_)
  bool accept(const double w[3], float& direction) const {
    const int n = (int)lx.size();
    int sum_gx = 0, sum_gy = 0;
    std::vector<double> level(n);
    for (int i = 0; i < n; i++) {
      const size_t at = (size_t)ly[i] * M.W + lx[i];
      const int gx = M.dx(at), gy = M.dy(at);
      sum_gx += gx; sum_gy += gy;
      level[i] = std::atan2(-(double)gx, (double)gy);
    }
    if (sum_gx == 0 && sum_gy == 0) return false;
    const double ax = std::fabs(w[1]), ay = std::fabs(w[0]);
    if (sum_gx > 0 && sum_gy >= 0) direction = (float)std::atan2(-ay, ax);
    if (sum_gx <= 0 && sum_gy > 0) direction = (float)std::atan2(ay, ax);
    if (sum_gx < 0 && sum_gy <= 0) direction = (float)std::atan2(ay, -ax);
    if (sum_gx >= 0 && sum_gy < 0) direction = (float)std::atan2(-ay, -ax);
    const double ad = std::fabs(direction);
    if ((ad < 0.15 || M_PI - ad < 0.15) && (std::fabs(w[2]) < 10 || std::fabs((unsigned)M.H - std::fabs(w[2])) < 10)) return false;     // along the top / bottom border
    if (std::fabs(ad - M_PI * 0.5) < 0.15 && (std::fabs(w[2]) < 10 || std::fabs((unsigned)M.W - std::fabs(w[2])) < 10)) return false;    // along the left / right border
    int aligned = 0;
    for (int i = 0; i < n; i++) {
      const double d = std::fabs(direction - level[i]);
      if (std::fabs(2 * M_PI - d) < 0.392699 || d < 0.392699) aligned++;
    }
    return minus_log10_nfa(n, aligned, 0.125, logNT) > 0;
  }

  void run(const Chain& c, std::vector<Segment>& out) {
    const unsigned* cx = c.x.data(); const unsigned* cy = c.y.data();
    unsigned s = 0;
    const unsigned e = (unsigned)c.x.size();
    const unsigned L = (unsigned)P.min_len;
    while (e > s + L) {
      // an initial segment: slide along the chain until 15 consecutive pixels fit a line
      NormalEq eq;
      double a = 0, b = 0, err = 0;
      bool hor = false;
      while (e > s + L) {
        hor = M.horizontal(cx[s], cy[s]);
        const unsigned* coord = (hor ? cx : cy) + s; const unsigned* value = (hor ? cy : cx) + s;
        eq = NormalEq::of(coord, value, (int)L);
        eq.solve(a, b);
        double sq = 0;
        for (unsigned i = 0; i < L; i++) { const double r = (double)value[i] - (double)coord[i] * a - b; sq += r * r; }
        err = std::sqrt(sq);
        if (err <= P.fit_err) break;
        s += P.skip;
      }
      if (err > P.fit_err) break;
      // grow it.  The orientation of the first pixel decides the parametrisation (y = a x + b or x = a y + b) for the whole line.
      lx.assign(cx + s, cx + s + L); ly.assign(cy + s, cy + s + L);
      s += L;
      double norm = 0;
      size_t grown_from = 0;      // first pixel the latest attempt added
      for (int attempt = 1;; attempt++) {
        if (attempt > 1) {
          // refit with the pixels the previous attempt added: their terms join the running (float) sums.  The parametrisation
          // test reads the line's first pixel (LeastSquaresLineFit_ :2733 / :2762).
          const bool h2 = M.horizontal(lx[0], ly[0]);
          const size_t n_new = lx.size() - grown_from;
          eq.add(NormalEq::of((h2 ? lx.data() : ly.data()) + grown_from, (h2 ? ly.data() : lx.data()) + grown_from, (int)n_new));
          eq.solve(a, b);
        }
        norm = 1 / std::sqrt(a * a + 1);
        grown_from = lx.size();
        int outliers = 0;
        while (e > s) {
          const double d = (hor ? std::fabs(a * cx[s] - cy[s] + b) : std::fabs(cx[s] - a * cy[s] - b)) * norm;
          lx.push_back(cx[s]); ly.push_back(cy[s]); s++;
          if (d > P.fit_err) { if (++outliers > P.max_outlier) break; }
          else outliers = 0;
        }
        lx.resize(lx.size() - outliers); ly.resize(ly.size() - outliers); s -= outliers;   // trailing outliers go back to the chain
        if (!(lx.size() > grown_from && attempt < P.try_time)) break;
      }
      double w[3];   // w0 x + w1 y + w2 = 0, w0^2 + w1^2 = 1
      if (hor) { w[0] = a * norm; w[1] = -1 * norm; w[2] = b * norm; }
      else { w[0] = 1 * norm; w[1] = -a * norm; w[2] = -b * norm; }
      float direction = 0;
      if (accept(w, direction)) {
        const double p1 = w[1] * w[1], p2 = w[0] * w[0], p3 = w[0] * w[1], p4 = w[2] * w[0], p5 = w[2] * w[1];
        Segment sg;
        unsigned X = lx.front(), Y = ly.front();
        sg.x1 = (float)(p1 * X - p3 * Y - p4); sg.y1 = (float)(p2 * Y - p3 * X - p5);
        X = lx.back(); Y = ly.back();
        sg.x2 = (float)(p1 * X - p3 * Y - p4); sg.y2 = (float)(p2 * Y - p3 * X - p5);
        sg.direction = direction;
        sg.n_pixels = (int)lx.size();
        out.push_back(sg);
      }
    }
  }
};

// Resident scratch of a detector's line producer (grows only): beside the driver's, the packed maps on the device and their pinned copy
struct LinesScratch : cs::ImageBatchScratch {
  cs::DevBuf<unsigned char> d_pk;
  cs::PinBuf<unsigned char> h_pin;   // per image: the packed map, 3 bytes per pixel (+ 4 bytes of pad behind the last image)
};
void lines_scratch_free(void* p) { delete (LinesScratch*)p; }      // (cs_detector_destroy has made the device current and waited for the stream)

// the sequential half of one image: routing, fitting, validation, end points (all of it independent of the other images)
// extra (optional, cap records): each kept segment's lineDirection_ and numOfPixels (OctaveKeyLines :1081-1082), what the descriptor needs beside the end points
int lines_host_stage(const Maps& M, const EdParams& P, double length_thres, float* lines4, int cap, int* n_lines, cs::LineExtra* extra = nullptr) {
  const int img_w = M.W, img_h = M.H;
  const size_t N = (size_t)img_w * img_h;
  *n_lines = 0;
  // anchors in the reference's scan order: columns outermost (:1641-1643)
  Router R(M);
  Extractor X(M, P);
  std::vector<Segment> segs;
  Chain first, second, chain;
  // The reference visits the scan grid column by column; on a row-major map that is one cache miss per probe (117 k probes, 5 KB apart, at KITTI's
  // size: 0.34 of the stage's 0.48 ms).  The grid is read ROW by row instead and its anchors dealt to their columns (a counting sort, stable: a
  // column's anchors stay in row order) -- the list below IS the reference's visiting order.
  std::vector<unsigned> col_at((size_t)img_w + 1, 0u), grid_at;
  grid_at.reserve(4096);
  for (int y = 1; y < img_h - 1; y += P.scan) {
    const unsigned char* row = M.p3 + 3 * (size_t)y * img_w + 1;      // (the anchor flag: bit 3 of a pixel's second byte)
    for (int x = 1; x < img_w - 1; x += P.scan)
      if ((row[3 * x] >> 3) & 1) { grid_at.push_back((unsigned)((size_t)y * img_w + x)); col_at[(size_t)x + 1]++; }
  }
  if (grid_at.size() > N / 5) { cs_set_error("cs_detect_lines_gray: more anchors than the reference's arrays hold"); return CS_ERR_CAPACITY; }
  for (int x = 0; x < img_w; x++) col_at[(size_t)x + 1] += col_at[x];
  std::vector<unsigned> anchors(grid_at.size());
  for (const unsigned at : grid_at) anchors[col_at[at % (unsigned)img_w]++] = at;
  for (const unsigned at_u : anchors) {
    {
      const size_t at = at_u;
      const int x = (int)(at_u % (unsigned)img_w), y = (int)(at_u / (unsigned)img_w);
      if (R.taken[at]) continue;
      first.x.clear(); first.y.clear(); second.x.clear(); second.y.clear();
      const bool hor = M.horizontal(at);
      R.walk(x, y, hor ? RIGHT : DOWN, first);
      R.taken[at] = 0;                                 // the anchor opens the second walk too
      R.walk(x, y, hor ? LEFT : UP, second);
      if ((int)(first.x.size() + second.x.size()) < P.min_len + 1) continue;     // too short: dropped, its pixels stay taken
      chain.x.assign(first.x.rbegin(), first.x.rend()); chain.y.assign(first.y.rbegin(), first.y.rend());
      chain.x.insert(chain.x.end(), second.x.begin() + 1, second.x.end()); chain.y.insert(chain.y.end(), second.y.begin() + 1, second.y.end());
      X.run(chain, segs);
    }
  }
  // OctaveKeyLines :862-875 (length), :1074-1143 (which end is the start), filter_lines: length > threshold
  int n = 0;
  for (const Segment& s : segs) {
    const float ddx = std::fabs(s.x1 - s.x2), ddy = std::fabs(s.y1 - s.y2);
    const float len = std::sqrt(ddx * ddx + ddy * ddy);
    if (!(len > (float)length_thres)) continue;
    const float ex = s.x2 - s.x1, ey = s.y2 - s.y1, dir = s.direction;
    bool flip = false;
    if (dir >= -0.75 * M_PI && dir < -0.25 * M_PI) flip = ey > 0;
    if (dir >= -0.25 * M_PI && dir < 0.25 * M_PI) flip = flip || ex < 0;
    if (dir >= 0.25 * M_PI && dir < 0.75 * M_PI) flip = flip || ey < 0;
    if ((dir >= 0.75 * M_PI && dir < M_PI) || (dir >= -M_PI && dir < -0.75 * M_PI)) flip = flip || ex > 0;
    if (n >= cap) { cs_set_error("cs_detect_lines_gray: more segments than `cap`"); return CS_ERR_CAPACITY; }
    float* o = lines4 + 4 * (size_t)n;
    if (flip) { o[0] = s.x2; o[1] = s.y2; o[2] = s.x1; o[3] = s.y1; } else { o[0] = s.x1; o[1] = s.y1; o[2] = s.x2; o[3] = s.y2; }
    if (extra) { extra[n].direction = s.direction; extra[n].num_pixels = s.n_pixels; }
    n++;
  }
  *n_lines = n;
  return CS_OK;
}

}  // namespace

// n_images gray images of one size: the per-pixel stages on the device, the packed maps copied into pinned staging, the sequential halves side by
// side on the detector's worker pool (cs::run_image_batch).  lines4[i] receives image i's segments (cap rows of 4), n_lines[i] their number.
// The entry behind cs_detect_lines_batch, with two optional extras for the descriptor path (lbd_host.cpp; detect_hooks.h): extra[i] receives image i's
// per-segment direction / pixel count, and `then` runs after the host stages and only if every image succeeded, still under the producers' lock,
// with the batch's packed maps resident on the device (image i's at d_p3 + 3 N i) and the detector's stream idle.
extern "C" int cs_internal_detect_lines_batch(cs_detector* d, const unsigned char* const* grays, int n_images, int img_w, int img_h, double length_thres, float* const* lines4, int cap,
                                              int* n_lines, cs::LineExtra* const* extra, int (*then)(void* ctx, const unsigned char* d_p3), void* then_ctx) {
  if (!d || n_images < 0 || (n_images && (!grays || !n_lines || (cap && !lines4))) || img_w < 3 || img_h < 3 || cap < 0) return CS_ERR_INVALID_ARG;
  for (int i = 0; i < n_images; i++) if (!grays[i] || (cap && !lines4[i])) return CS_ERR_INVALID_ARG;
  try {
    for (int i = 0; i < n_images; i++) n_lines[i] = 0;
    if (n_images == 0) return CS_OK;
    std::lock_guard<std::mutex> lk(*(std::mutex*)cs_internal_detector_lines_mutex(d));
    CS_HIP_TRY(hipSetDevice(cs_internal_detector_device(d)));
    hipStream_t st = (hipStream_t)cs_internal_detector_stream(d);
    void** slot = cs_internal_detector_scratch_slot(d, cs::SCRATCH_EDLINES, lines_scratch_free);
    if (!*slot) *slot = new LinesScratch();
    LinesScratch& S = *(LinesScratch*)*slot;
    const double t_begin = cs::now_ms();
    const EdParams P;
    const size_t N = (size_t)img_w * img_h, need = N * (size_t)n_images;
    CS_ENSURE(S.d_gray, need);
    CS_ENSURE(S.d_pk, 3 * need + 4);
    CS_ENSURE(S.h_pin, 3 * need + 4);
    CS_ENSURE(S.h_in, need);
    int k[3];
    cs::lines_blur_taps(k);
    auto launch = [&](int i0, int ni) {
      cs::launch_lines_maps(S.d_gray.p + (size_t)i0 * N, img_w, img_h, cs::LineMaps{S.d_pk.p + 3 * N * (size_t)i0}, k, P.grad_thr, P.anchor_thr, P.scan, st, ni);
    };
    auto stage = [&](int i) {
      Maps M; M.W = img_w; M.H = img_h; M.grad_thr = P.grad_thr; M.p3 = S.h_pin.p + 3 * N * (size_t)i;
      return lines_host_stage(M, P, length_thres, lines4 ? lines4[i] : nullptr, cap, &n_lines[i], extra ? extra[i] : nullptr);
    };
    CS_TRY(cs::run_image_batch(d, S, t_begin, grays, n_images, N, S.d_pk.p, S.h_pin.p, 3 * N, 3 * N, launch, stage));
    return then ? then(then_ctx, S.d_pk.p) : CS_OK;
  } catch (const std::exception& ex) {
    cs_set_error(std::string("cs_detect_lines_batch: ") + ex.what());
    return CS_ERR_CAPACITY;
  }
}

// n_images gray images of one size (see above)
extern "C" int cs_detect_lines_batch(cs_detector* d, const unsigned char* const* grays, int n_images, int img_w, int img_h, double length_thres, float* const* lines4, int cap,
                                     int* n_lines) {
  return cs_internal_detect_lines_batch(d, grays, n_images, img_w, img_h, length_thres, lines4, cap, n_lines, nullptr, nullptr, nullptr);
}

// timing of the last cs_detect_lines_batch / cs_detect_lines_gray of this detector: the device kernels, the host stage (wall), the whole call
extern "C" int cs_detect_lines_last_timing(cs_detector* d, double* device_ms, double* host_ms, double* total_ms) {
  if (!d) return CS_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(*(std::mutex*)cs_internal_detector_lines_mutex(d));
  const LinesScratch* S = (const LinesScratch*)*cs_internal_detector_scratch_slot(d, cs::SCRATCH_EDLINES, lines_scratch_free);
  return S ? cs::batch_last_timing(*S, device_ms, host_ms, total_ms) : CS_ERR_NOT_RUN;
}

extern "C" int cs_detect_lines_gray(cs_detector* d, const unsigned char* gray, int img_w, int img_h, double length_thres, float* lines4, int cap, int* n_lines) {
  if (!d || !gray || img_w < 3 || img_h < 3 || cap < 0 || (cap && !lines4) || !n_lines) return CS_ERR_INVALID_ARG;
  float* l4 = lines4;
  return cs_detect_lines_batch(d, &gray, 1, img_w, img_h, length_thres, &l4, cap, n_lines);
}
