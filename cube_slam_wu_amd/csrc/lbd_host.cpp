// lbd_host.cpp -- line descriptors and their matching behind the C ABI: what a line-tracking caller used the reference's libline_lbd_lib for beside
// detect_filter_lines,
//   line_lbd_detect::detect_descrip_lines(gray, keylines_out, descrips)     line_lbd/class/line_lbd_allclass.cpp:239-282   (EDLines branch)
//   line_lbd_detect::get_line_descriptors(gray, linesmat, descrips)         :190-197      (BinaryDescriptor::compute on the caller's keylines)
//   line_lbd_detect::match_line_descrip(descrips1, descrips2, matches)      :352-369      (BinaryDescriptorMatcher::match, then dist < matching_dist_thres)
// The descriptor reads the Sobel derivatives of the blurred image, which are exactly what the EDLines producer's device stage leaves resident
// (lines_kernels.hip: BinaryDescriptor::computeSobel, binary_descriptor.cpp:352-402, is the same GaussianBlur 5 x 5 sigma 1 + Sobel 16S), so detect +
// describe costs one more kernel over the maps that are already there.  The arithmetic and its contract: cs_lbd.h; the kernels: lbd_kernels.hip.
// Everything that launches them is here (lines_host.cpp knows none of it: tools/hostonly/lines_host_check.cpp builds that file alone).  Its scratch
// lives in the detector's third slot (detect_hooks.h: cs::SCRATCH_LBD), under the same lock as the two producers'.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/cubeslam_hip.h"
#include "cs_hip_util.h"
#include "cs_lbd.h"
#include "detect_hooks.h"
#include "lbd_types.h"
#include "lines_types.h"

namespace {

// Resident scratch of a detector's descriptor / matching path (grows only).
struct LbdScratch {
  cs::DevBuf<unsigned char> d_gray, d_p3, d_desc32;      // d_gray / d_p3: cs_lbd_describe_gray's own image and map (the producer's are not touched)
  cs::DevBuf<float> d_desc72;
  cs::DevBuf<cs::LbdLine> d_lines;
  cs::DevBuf<cs::LbdWeights> d_w;
  bool weights_up = false;
  cs::DevBuf<unsigned> d_q, d_t;
  cs::DevBuf<int> d_ptr, d_out;                          // q_ptr | t_ptr; train_idx | dist | dist2
  cs::Event ev0, ev1;
  double describe_ms = -1, match_ms = -1;
  std::vector<cs::LbdLine> lines;
  std::vector<unsigned char> desc;
  std::vector<int> out;
};
void lbd_scratch_free(void* p) { delete (LbdScratch*)p; }      // (cs_detector_destroy has made the device current and waited for the stream)
LbdScratch& scratch_of(cs_detector* d) {
  void** slot = cs_internal_detector_scratch_slot(d, cs::SCRATCH_LBD, lbd_scratch_free);
  if (!*slot) *slot = new LbdScratch();
  return *(LbdScratch*)*slot;
}
int events_of(LbdScratch& S) {
  if (!S.ev0) { CS_TRY(S.ev0.create()); CS_TRY(S.ev1.create()); }
  return CS_OK;
}

bool keyline_ok(const cs_keyline& k) {
  return std::isfinite(k.sx) && std::isfinite(k.sy) && std::isfinite(k.ex) && std::isfinite(k.ey) && std::isfinite(k.direction) && k.num_pixels >= 0 && k.num_pixels <= 32767;
}

// S.lines (n records over the images of d_p3) -> desc32 / desc72 on the host (n rows each; desc72 may be null).  The caller holds the producer's lock.
int describe_resident(LbdScratch& S, hipStream_t st, const unsigned char* d_p3, int W, int H, unsigned char* desc32, float* desc72) {
  const size_t n = S.lines.size();
  if (n == 0) { S.describe_ms = 0; return CS_OK; }
  int rc = events_of(S);
  if (!rc) rc = S.d_lines.ensure(n);
  if (!rc) rc = S.d_desc32.ensure(n * cs::LBD_BYTES);
  if (!rc && desc72) rc = S.d_desc72.ensure(n * cs::LBD_FLOATS);
  if (!rc) rc = S.d_w.ensure(1);
  if (rc) return rc;
  if (!S.weights_up) {
    cs::LbdWeights w;
    cs::lbd_weights(w);
    CS_HIP_TRY(hipMemcpy(S.d_w.p, &w, sizeof(w), hipMemcpyHostToDevice));
    S.weights_up = true;
  }
  CS_HIP_TRY(hipMemcpyAsync(S.d_lines.p, S.lines.data(), n * sizeof(cs::LbdLine), hipMemcpyHostToDevice, st));
  CS_HIP_TRY(hipEventRecord(S.ev0, st));
  cs::launch_lbd_describe(d_p3, W, H, S.d_lines.p, (int)n, S.d_w.p, S.d_desc32.p, desc72 ? S.d_desc72.p : nullptr, st);
  CS_HIP_TRY(hipGetLastError());
  CS_HIP_TRY(hipEventRecord(S.ev1, st));
  CS_HIP_TRY(hipMemcpyAsync(desc32, S.d_desc32.p, n * cs::LBD_BYTES, hipMemcpyDeviceToHost, st));
  if (desc72) CS_HIP_TRY(hipMemcpyAsync(desc72, S.d_desc72.p, n * cs::LBD_FLOATS * sizeof(float), hipMemcpyDeviceToHost, st));
  CS_HIP_TRY(hipStreamSynchronize(st));
  float ms = 0;
  CS_HIP_TRY(hipEventElapsedTime(&ms, S.ev0, S.ev1));
  S.describe_ms = ms;
  return CS_OK;
}

}  // namespace

extern "C" int cs_lbd_describe_gray(cs_detector* d, const unsigned char* gray, int img_w, int img_h, const cs_keyline* kl, int n, unsigned char* desc32, float* desc72) {
  if (!d || !gray || img_w < 3 || img_h < 3 || img_w > 32767 || img_h > 32767 || n < 0 || (n && (!kl || !desc32))) return CS_ERR_INVALID_ARG;
  for (int i = 0; i < n; i++)
    if (!keyline_ok(kl[i])) { cs_set_error("cs_lbd_describe_gray: a keyline with a non-finite coordinate or direction, or num_pixels outside [0, 32767]"); return CS_ERR_INVALID_ARG; }
  if (n == 0) return CS_OK;
  CS_GUARD_BEGIN
  std::lock_guard<std::mutex> lk(*(std::mutex*)cs_internal_detector_lines_mutex(d));
  CS_HIP_TRY(hipSetDevice(cs_internal_detector_device(d)));
  hipStream_t st = (hipStream_t)cs_internal_detector_stream(d);
  LbdScratch& S = scratch_of(d);
  const size_t N = (size_t)img_w * img_h;
  int rc = S.d_gray.ensure(N);
  if (!rc) rc = S.d_p3.ensure(3 * N + 4);
  if (rc) return rc;
  CS_HIP_TRY(hipMemcpyAsync(S.d_gray.p, gray, N, hipMemcpyHostToDevice, st));
  int k[3];
  cs::lines_blur_taps(k);
  cs::launch_lines_maps(S.d_gray.p, img_w, img_h, cs::LineMaps{S.d_p3.p}, k, 80, 8, 2, st, 1);     // (the thresholds only set the anchor bit, which is not read here)
  CS_HIP_TRY(hipGetLastError());
  S.lines.resize((size_t)n);
  for (int i = 0; i < n; i++) S.lines[i] = cs::lbd_line(kl[i].sx, kl[i].sy, kl[i].ex, kl[i].ey, kl[i].direction, kl[i].num_pixels, 0);
  return describe_resident(S, st, S.d_p3.p, img_w, img_h, desc32, desc72);
  CS_GUARD_END("cs_lbd_describe_gray")
}

extern "C" int cs_detect_descrip_lines_batch(cs_detector* d, const unsigned char* const* grays, int n_images, int img_w, int img_h, double length_thres, cs_keyline* const* kl,
                                             unsigned char* const* desc32, int cap, int* n_lines) {
  if (!d || n_images < 0 || (n_images && (!grays || !n_lines || (cap && (!kl || !desc32)))) || img_w < 3 || img_h < 3 || img_w > 32767 || img_h > 32767 || cap < 0) return CS_ERR_INVALID_ARG;
  for (int i = 0; i < n_images; i++) if (!grays[i] || (cap && (!kl[i] || !desc32[i]))) return CS_ERR_INVALID_ARG;
  if (n_images == 0) return CS_OK;
  CS_GUARD_BEGIN
  // the producer writes rows of four floats and the extras; the records are put together behind it
  std::unique_ptr<float[]> seg(new float[4 * (size_t)cap * n_images + 1]);
  std::unique_ptr<cs::LineExtra[]> ext(new cs::LineExtra[(size_t)cap * n_images + 1]);
  std::vector<float*> seg_of(n_images);
  std::vector<cs::LineExtra*> ext_of(n_images);
  for (int i = 0; i < n_images; i++) { seg_of[i] = seg.get() + 4 * (size_t)cap * i; ext_of[i] = ext.get() + (size_t)cap * i; }
  struct Ctx { cs_detector* d; int W, H, n_images, cap; const int* n_lines; float* const* seg; cs::LineExtra* const* ext; cs_keyline* const* kl; unsigned char* const* desc32; } ctx{
      d, img_w, img_h, n_images, cap, n_lines, seg_of.data(), ext_of.data(), kl, desc32};
  // all images' lines in one launch, after the host stages, while the maps of the whole batch are still resident
  auto then = [](void* vp, const unsigned char* d_p3) -> int {
    Ctx& c = *(Ctx*)vp;
    try {
      LbdScratch& S = scratch_of(c.d);
      S.lines.clear();
      for (int i = 0; i < c.n_images; i++)
        for (int j = 0; j < c.n_lines[i]; j++) {
          const float* s = c.seg[i] + 4 * (size_t)j;
          const cs::LineExtra& e = c.ext[i][j];
          if (e.num_pixels > 32767) { cs_set_error("cs_detect_descrip_lines: a line of more than 32767 pixels"); return CS_ERR_CAPACITY; }
          c.kl[i][j] = cs_keyline{s[0], s[1], s[2], s[3], e.direction, e.num_pixels};
          S.lines.push_back(cs::lbd_line(s[0], s[1], s[2], s[3], e.direction, e.num_pixels, i));
        }
      S.desc.resize(S.lines.size() * cs::LBD_BYTES);
      const int rc = describe_resident(S, (hipStream_t)cs_internal_detector_stream(c.d), d_p3, c.W, c.H, S.desc.data(), nullptr);
      if (rc) return rc;
      size_t at = 0;
      for (int i = 0; i < c.n_images; i++) {
        if (c.n_lines[i]) std::memcpy(c.desc32[i], S.desc.data() + at, (size_t)c.n_lines[i] * cs::LBD_BYTES);
        at += (size_t)c.n_lines[i] * cs::LBD_BYTES;
      }
      return CS_OK;
    } catch (const std::exception& ex) {
      cs_set_error(std::string("cs_detect_descrip_lines_batch: ") + ex.what());
      return CS_ERR_CAPACITY;
    }
  };
  return cs_internal_detect_lines_batch(d, grays, n_images, img_w, img_h, length_thres, seg_of.data(), cap, n_lines, ext_of.data(), then, &ctx);
  CS_GUARD_END("cs_detect_descrip_lines_batch")
}

extern "C" int cs_detect_descrip_lines_gray(cs_detector* d, const unsigned char* gray, int img_w, int img_h, double length_thres, cs_keyline* kl, unsigned char* desc32, int cap, int* n_lines) {
  if (!d || !gray || !n_lines || cap < 0 || (cap && (!kl || !desc32))) return CS_ERR_INVALID_ARG;
  cs_keyline* k1 = kl;
  unsigned char* d1 = desc32;
  return cs_detect_descrip_lines_batch(d, &gray, 1, img_w, img_h, length_thres, &k1, &d1, cap, n_lines);
}

extern "C" int cs_lbd_match_batch(cs_detector* d, int n_pairs, const unsigned char* q32, const int* q_ptr, const unsigned char* t32, const int* t_ptr, int* train_idx, int* dist, int* dist2) {
  if (!d || n_pairs < 0 || (n_pairs && (!q_ptr || !t_ptr))) return CS_ERR_INVALID_ARG;
  if (n_pairs == 0) return CS_OK;
  if (q_ptr[0] != 0 || t_ptr[0] != 0) return CS_ERR_INVALID_ARG;
  int max_nq = 0;
  for (int p = 0; p < n_pairs; p++) {
    if (q_ptr[p + 1] < q_ptr[p] || t_ptr[p + 1] < t_ptr[p]) return CS_ERR_INVALID_ARG;
    max_nq = std::max(max_nq, q_ptr[p + 1] - q_ptr[p]);
  }
  const size_t nq = (size_t)q_ptr[n_pairs], nt = (size_t)t_ptr[n_pairs];
  if (nq == 0) return CS_OK;
  if (!q32 || (nt && !t32) || !train_idx || !dist) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  std::lock_guard<std::mutex> lk(*(std::mutex*)cs_internal_detector_lines_mutex(d));
  CS_HIP_TRY(hipSetDevice(cs_internal_detector_device(d)));
  hipStream_t st = (hipStream_t)cs_internal_detector_stream(d);
  LbdScratch& S = scratch_of(d);
  const size_t np1 = (size_t)n_pairs + 1;
  int rc = events_of(S);
  if (!rc) rc = S.d_q.ensure(8 * nq);
  if (!rc) rc = S.d_t.ensure(8 * nt + 8);
  if (!rc) rc = S.d_ptr.ensure(2 * np1);
  if (!rc) rc = S.d_out.ensure(3 * nq);
  if (rc) return rc;
  CS_HIP_TRY(hipMemcpyAsync(S.d_q.p, q32, 32 * nq, hipMemcpyHostToDevice, st));
  if (nt) CS_HIP_TRY(hipMemcpyAsync(S.d_t.p, t32, 32 * nt, hipMemcpyHostToDevice, st));
  CS_HIP_TRY(hipMemcpyAsync(S.d_ptr.p, q_ptr, np1 * sizeof(int), hipMemcpyHostToDevice, st));
  CS_HIP_TRY(hipMemcpyAsync(S.d_ptr.p + np1, t_ptr, np1 * sizeof(int), hipMemcpyHostToDevice, st));
  CS_HIP_TRY(hipEventRecord(S.ev0, st));
  cs::launch_lbd_match(n_pairs, max_nq, S.d_q.p, S.d_ptr.p, S.d_t.p, S.d_ptr.p + np1, S.d_out.p, S.d_out.p + nq, S.d_out.p + 2 * nq, st);
  CS_HIP_TRY(hipGetLastError());
  CS_HIP_TRY(hipEventRecord(S.ev1, st));
  S.out.resize(3 * nq);
  CS_HIP_TRY(hipMemcpyAsync(S.out.data(), S.d_out.p, 3 * nq * sizeof(int), hipMemcpyDeviceToHost, st));
  CS_HIP_TRY(hipStreamSynchronize(st));
  float ms = 0;
  CS_HIP_TRY(hipEventElapsedTime(&ms, S.ev0, S.ev1));
  S.match_ms = ms;
  std::memcpy(train_idx, S.out.data(), nq * sizeof(int));
  std::memcpy(dist, S.out.data() + nq, nq * sizeof(int));
  if (dist2) std::memcpy(dist2, S.out.data() + 2 * nq, nq * sizeof(int));
  return CS_OK;
  CS_GUARD_END("cs_lbd_match_batch")
}

extern "C" int cs_lbd_match(cs_detector* d, const unsigned char* q32, int nq, const unsigned char* t32, int nt, int* train_idx, int* dist, int* dist2) {
  if (nq < 0 || nt < 0) return CS_ERR_INVALID_ARG;
  const int qp[2] = {0, nq}, tp[2] = {0, nt};
  return cs_lbd_match_batch(d, 1, q32, qp, t32, tp, train_idx, dist, dist2);
}

extern "C" int cs_lbd_last_timing(cs_detector* d, double* describe_kernel_ms, double* match_kernel_ms) {
  if (!d) return CS_ERR_INVALID_ARG;
  std::lock_guard<std::mutex> lk(*(std::mutex*)cs_internal_detector_lines_mutex(d));
  const LbdScratch& S = scratch_of(d);
  if (describe_kernel_ms) *describe_kernel_ms = S.describe_ms;
  if (match_kernel_ms) *match_kernel_ms = S.match_ms;
  return CS_OK;
}
