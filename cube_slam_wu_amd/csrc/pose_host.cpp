// pose_host.cpp -- the C ABI of the batched motion-only pose optimisation (include/cubeslam_hip.h: cs_pose_*).
//
// What an ORB-SLAM2-derived tracker does once per frame with g2o -- one free VertexSE3Expmap, a few hundred
// EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose (types/types_six_dof_expmap.h:208-267), a few optimize() rounds with an
// inlier / outlier classification between them -- for many frames in ONE kernel launch (pose_kernels.hip).  The host packs the
// observations into 128-byte records, uploads everything with one copy, launches, and downloads everything with one copy.
// There is no CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/cubeslam_hip.h"
#include "cs_hip_util.h"
#include "pose_types.h"

struct cs_pose_batch {
  int device = 0;
  hipStream_t st = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  cs::DevBuf<unsigned char> d_in;      // [T0 | intr | records | obs_ptr], one upload
  cs::DevBuf<unsigned char> d_out;     // [T_out | chi2 | iterations | inlier], one download
  cs::PinBuf<unsigned char> h_in, h_out;     // pinned staging of the two
  double kernel_ms = 0, host_ms = 0;
  bool ran = false;
};

namespace {

size_t align256(size_t n) { return (n + 255) & ~(size_t)255; }

int check_params(const cs_pose_params* p) {
  if (!p || p->n_rounds < 1 || p->n_rounds > cs::POSE_MAX_ROUNDS) { cs_set_error("cs_pose: n_rounds must be 1..8"); return CS_ERR_INVALID_ARG; }
  for (int r = 0; r < p->n_rounds; r++)
    if (p->iterations[r] < 0) { cs_set_error("cs_pose: negative iteration count"); return CS_ERR_INVALID_ARG; }
  return CS_OK;
}

}  // namespace

extern "C" {

void cs_pose_default_params(cs_pose_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->n_rounds = 4;
  for (int r = 0; r < 4; r++) p->iterations[r] = 10;
  p->robust_rounds = 3;
  p->restart_each_round = 1;
  p->huber_mono = std::sqrt(5.991); p->huber_stereo = std::sqrt(7.815);
  p->chi2_mono = 5.991; p->chi2_stereo = 7.815;
}

int cs_pose_batch_create(int device, cs_pose_batch** out) {
  if (!out) return CS_ERR_INVALID_ARG;
  *out = nullptr;
  { const int rc = cs::check_device(device); if (rc) return rc; }
  cs_pose_batch* B = new (std::nothrow) cs_pose_batch();
  if (!B) return CS_ERR_CAPACITY;
  struct Guard { cs_pose_batch* b; ~Guard() { if (b) cs_pose_batch_destroy(b); } } g{B};
  B->device = device;
  CS_HIP_TRY(hipSetDevice(device));
  CS_HIP_TRY(hipStreamCreateWithFlags(&B->st, hipStreamNonBlocking));
  CS_HIP_TRY(hipEventCreate(&B->ev0));
  CS_HIP_TRY(hipEventCreate(&B->ev1));
  g.b = nullptr;
  *out = B;
  return CS_OK;
}

void cs_pose_batch_destroy(cs_pose_batch* B) {
  if (!B) return;
  (void)hipSetDevice(B->device);
  if (B->st) (void)hipStreamSynchronize(B->st);
  B->d_in.release(); B->d_out.release(); B->h_in.release(); B->h_out.release();
  if (B->ev0) (void)hipEventDestroy(B->ev0);
  if (B->ev1) (void)hipEventDestroy(B->ev1);
  if (B->st) (void)hipStreamDestroy(B->st);
  delete B;
}

int cs_pose_batch_optimize(cs_pose_batch* B, const cs_pose_params* p, int n_frames, const double* Tcw7_in, const double* intr5, const int* obs_ptr,
                           const double* Xw3, const double* meas3, const double* info9, const unsigned char* is_stereo,
                           double* Tcw7_out, unsigned char* inlier_out, double* chi2_out, int* iterations_done) {
  if (!B || n_frames < 0) return CS_ERR_INVALID_ARG;
  int rc = check_params(p); if (rc) return rc;
  B->ran = false;
  if (n_frames == 0) { B->kernel_ms = B->host_ms = 0; B->ran = true; return CS_OK; }
  if (!Tcw7_in || !intr5 || !obs_ptr || !Tcw7_out) { cs_set_error("cs_pose_batch_optimize: NULL argument"); return CS_ERR_INVALID_ARG; }
  const double t_begin = cs::now_ms();
  // the kernel indexes the records by obs_ptr alone: it must be a non-decreasing partition of [0, n_obs)
  if (obs_ptr[0] != 0) { cs_set_error("cs_pose_batch_optimize: obs_ptr[0] must be 0"); return CS_ERR_INVALID_ARG; }
  for (int f = 0; f < n_frames; f++)
    if (obs_ptr[f + 1] < obs_ptr[f]) { cs_set_error("cs_pose_batch_optimize: obs_ptr must not decrease"); return CS_ERR_INVALID_ARG; }
  const size_t n_obs = (size_t)obs_ptr[n_frames];
  if (n_obs > 0 && (!Xw3 || !meas3 || !info9 || !is_stereo || !inlier_out)) { cs_set_error("cs_pose_batch_optimize: NULL observation array"); return CS_ERR_INVALID_ARG; }
  const size_t R = (size_t)p->n_rounds, nf = (size_t)n_frames;

  // ---- layout of the two buffers (every part 256-byte aligned)
  const size_t in_T = 0, in_intr = align256(in_T + 7 * nf * 8), in_obs = align256(in_intr + 5 * nf * 8), in_ptr = align256(in_obs + n_obs * cs::POSE_OBS_DOUBLES * 8),
               in_bytes = align256(in_ptr + (nf + 1) * 4);
  const size_t out_T = 0, out_chi = align256(out_T + 7 * nf * 8), out_it = align256(out_chi + nf * R * 8), out_lv = align256(out_it + nf * R * 4), out_bytes = align256(out_lv + n_obs);
  CS_HIP_TRY(hipSetDevice(B->device));
  rc = B->d_in.ensure(in_bytes); if (rc) return rc;
  rc = B->d_out.ensure(out_bytes); if (rc) return rc;
  rc = B->h_in.ensure(in_bytes); if (rc) return rc;
  rc = B->h_out.ensure(out_bytes); if (rc) return rc;

  // ---- pack
  std::memcpy(B->h_in.p + in_T, Tcw7_in, 7 * nf * 8);
  std::memcpy(B->h_in.p + in_intr, intr5, 5 * nf * 8);
  std::memcpy(B->h_in.p + in_ptr, obs_ptr, (nf + 1) * 4);
  double* rec = reinterpret_cast<double*>(B->h_in.p + in_obs);
  for (size_t i = 0; i < n_obs; i++, rec += cs::POSE_OBS_DOUBLES) {
    const double *X = Xw3 + 3 * i, *m = meas3 + 3 * i, *W = info9 + 9 * i;
    rec[0] = X[0]; rec[1] = X[1]; rec[2] = X[2];
    if (is_stereo[i]) {
      rec[3] = m[0]; rec[4] = m[1]; rec[5] = m[2];
      for (int k = 0; k < 9; k++) rec[6 + k] = W[k];
      rec[15] = 1.0;
    } else {      // EdgeSE3ProjectXYZOnlyPose: (u, v) and the upper-left 2 x 2 of the information
      rec[3] = m[0]; rec[4] = m[1]; rec[5] = 0.0;
      rec[6] = W[0]; rec[7] = W[1]; rec[8] = 0.0; rec[9] = W[3]; rec[10] = W[4]; rec[11] = 0.0; rec[12] = rec[13] = rec[14] = 0.0;
      rec[15] = 0.0;
    }
  }

  cs::PoseLaunch a;
  a.n_frames = n_frames; a.n_rounds = p->n_rounds;
  for (int r = 0; r < cs::POSE_MAX_ROUNDS; r++) a.iterations[r] = r < p->n_rounds ? p->iterations[r] : 0;
  a.robust_rounds = p->robust_rounds; a.restart_each_round = p->restart_each_round ? 1 : 0;
  a.huber_mono = p->huber_mono; a.huber_stereo = p->huber_stereo; a.chi2_mono = p->chi2_mono; a.chi2_stereo = p->chi2_stereo;
  a.T0 = reinterpret_cast<const double*>(B->d_in.p + in_T);
  a.intr = reinterpret_cast<const double*>(B->d_in.p + in_intr);
  a.obs = reinterpret_cast<const double*>(B->d_in.p + in_obs);
  a.obs_ptr = reinterpret_cast<const int*>(B->d_in.p + in_ptr);
  a.T_out = reinterpret_cast<double*>(B->d_out.p + out_T);
  a.chi2_out = reinterpret_cast<double*>(B->d_out.p + out_chi);
  a.iters_out = reinterpret_cast<int*>(B->d_out.p + out_it);
  a.inlier = B->d_out.p + out_lv;

  CS_HIP_TRY(hipMemcpyAsync(B->d_in.p, B->h_in.p, in_bytes, hipMemcpyHostToDevice, B->st));
  CS_HIP_TRY(hipEventRecord(B->ev0, B->st));
  cs::pose_launch(a, B->st);
  CS_HIP_TRY(hipGetLastError());
  CS_HIP_TRY(hipEventRecord(B->ev1, B->st));
  CS_HIP_TRY(hipMemcpyAsync(B->h_out.p, B->d_out.p, out_bytes, hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  float ms = 0;
  CS_HIP_TRY(hipEventElapsedTime(&ms, B->ev0, B->ev1));

  std::memcpy(Tcw7_out, B->h_out.p + out_T, 7 * nf * 8);
  if (chi2_out) std::memcpy(chi2_out, B->h_out.p + out_chi, nf * R * 8);
  if (iterations_done) std::memcpy(iterations_done, B->h_out.p + out_it, nf * R * 4);
  if (n_obs) std::memcpy(inlier_out, B->h_out.p + out_lv, n_obs);
  B->kernel_ms = ms;
  B->host_ms = cs::now_ms() - t_begin;
  B->ran = true;
  return CS_OK;
}

int cs_pose_batch_last_timing(const cs_pose_batch* B, double* kernel_ms, double* host_ms) {
  if (!B) return CS_ERR_INVALID_ARG;
  if (!B->ran) return CS_ERR_NOT_RUN;
  if (kernel_ms) *kernel_ms = B->kernel_ms;
  if (host_ms) *host_ms = B->host_ms;
  return CS_OK;
}

int cs_pose_optimize_batch(int device, const cs_pose_params* p, int n_frames, const double* Tcw7_in, const double* intr5, const int* obs_ptr,
                           const double* Xw3, const double* meas3, const double* info9, const unsigned char* is_stereo,
                           double* Tcw7_out, unsigned char* inlier_out, double* chi2_out, int* iterations_done) {
  cs_pose_batch* B = nullptr;
  int rc = cs_pose_batch_create(device, &B);
  if (rc) return rc;
  rc = cs_pose_batch_optimize(B, p, n_frames, Tcw7_in, intr5, obs_ptr, Xw3, meas3, info9, is_stereo, Tcw7_out, inlier_out, chi2_out, iterations_done);
  cs_pose_batch_destroy(B);
  return rc;
}

}  // extern "C"
