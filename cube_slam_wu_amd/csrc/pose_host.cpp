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
#include "cs_batch_handle.h"
#include "pose_types.h"

// d_in = [T0 | intr | records | obs_ptr], d_out = [T_out | chi2 | iterations | inlier] or [system | inlier]
struct cs_pose_batch : cs::BatchHandle {};

namespace {

int check_params(const cs_pose_params* p) {
  if (!p || p->n_rounds < 1 || p->n_rounds > cs::POSE_MAX_ROUNDS) { cs_set_error("cs_pose: n_rounds must be 1..8"); return CS_ERR_INVALID_ARG; }
  for (int r = 0; r < p->n_rounds; r++)
    if (p->iterations[r] < 0) { cs_set_error("cs_pose: negative iteration count"); return CS_ERR_INVALID_ARG; }
  return CS_OK;
}

// What both entries check of their inputs.  *n_obs = obs_ptr[n_frames].
int check_frames(const std::string& who, int n_frames, const double* Tcw7_in, const double* intr5, const int* obs_ptr, const double* Xw3, const double* meas3,
                 const double* info9, const unsigned char* is_stereo, size_t* n_obs) {
  if (!Tcw7_in || !intr5 || !obs_ptr) { cs_set_error(who + ": NULL argument"); return CS_ERR_INVALID_ARG; }
  if (int rc = cs::check_partition(who + ": obs_ptr", obs_ptr, n_frames)) return rc;
  *n_obs = (size_t)obs_ptr[n_frames];
  if (*n_obs > 0 && (!Xw3 || !meas3 || !info9 || !is_stereo)) { cs_set_error(who + ": NULL observation array"); return CS_ERR_INVALID_ARG; }
  return CS_OK;
}

struct InLayout { size_t T, intr, obs, ptr, bytes; };

InLayout in_layout(size_t nf, size_t n_obs) {
  cs::Layout in;
  InLayout L;
  L.T = in.add(7 * nf * 8);
  L.intr = in.add(5 * nf * 8);
  L.obs = in.add(n_obs * cs::POSE_OBS_DOUBLES * 8);
  L.ptr = in.add((nf + 1) * 4);
  L.bytes = in.bytes;
  return L;
}

void pack_inputs(unsigned char* h, const InLayout& L, size_t nf, size_t n_obs, const double* Tcw7_in, const double* intr5, const int* obs_ptr,
                 const double* Xw3, const double* meas3, const double* info9, const unsigned char* is_stereo) {
  std::memcpy(h + L.T, Tcw7_in, 7 * nf * 8);
  std::memcpy(h + L.intr, intr5, 5 * nf * 8);
  std::memcpy(h + L.ptr, obs_ptr, (nf + 1) * 4);
  double* rec = reinterpret_cast<double*>(h + L.obs);
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
}

void set_inputs(cs::PoseLaunch& a, unsigned char* d, const InLayout& L, int n_frames) {
  std::memset(&a, 0, sizeof(a));
  a.n_frames = n_frames;
  a.T0 = reinterpret_cast<const double*>(d + L.T);
  a.intr = reinterpret_cast<const double*>(d + L.intr);
  a.obs = reinterpret_cast<const double*>(d + L.obs);
  a.obs_ptr = reinterpret_cast<const int*>(d + L.ptr);
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

int cs_pose_batch_create(int device, cs_pose_batch** out) { return cs::batch_create(device, out); }

void cs_pose_batch_destroy(cs_pose_batch* B) { cs::batch_destroy(B); }

int cs_pose_batch_optimize(cs_pose_batch* B, const cs_pose_params* p, int n_frames, const double* Tcw7_in, const double* intr5, const int* obs_ptr,
                           const double* Xw3, const double* meas3, const double* info9, const unsigned char* is_stereo,
                           double* Tcw7_out, unsigned char* inlier_out, double* chi2_out, int* iterations_done) {
  if (!B || n_frames < 0) return CS_ERR_INVALID_ARG;
  int rc = check_params(p); if (rc) return rc;
  B->ran = false;
  if (n_frames == 0) { B->kernel_ms = B->host_ms = 0; B->ran = true; return CS_OK; }
  if (!Tcw7_out) { cs_set_error("cs_pose_batch_optimize: NULL argument"); return CS_ERR_INVALID_ARG; }
  const double t_begin = cs::now_ms();
  size_t n_obs = 0;
  rc = check_frames("cs_pose_batch_optimize", n_frames, Tcw7_in, intr5, obs_ptr, Xw3, meas3, info9, is_stereo, &n_obs); if (rc) return rc;
  if (n_obs > 0 && !inlier_out) { cs_set_error("cs_pose_batch_optimize: NULL observation array"); return CS_ERR_INVALID_ARG; }
  const size_t R = (size_t)p->n_rounds, nf = (size_t)n_frames;

  // ---- layout of the two buffers
  const InLayout L = in_layout(nf, n_obs);
  cs::Layout out;
  const size_t out_T = out.add(7 * nf * 8), out_chi = out.add(nf * R * 8), out_it = out.add(nf * R * 4), out_lv = out.add(n_obs);

  cs::PoseLaunch a;
  auto pack = [&] {
    pack_inputs(B->h_in.p, L, nf, n_obs, Tcw7_in, intr5, obs_ptr, Xw3, meas3, info9, is_stereo);
    set_inputs(a, B->d_in.p, L, n_frames);
    a.n_rounds = p->n_rounds;
    for (int r = 0; r < cs::POSE_MAX_ROUNDS; r++) a.iterations[r] = r < p->n_rounds ? p->iterations[r] : 0;
    a.robust_rounds = p->robust_rounds; a.restart_each_round = p->restart_each_round ? 1 : 0;
    a.huber_mono = p->huber_mono; a.huber_stereo = p->huber_stereo; a.chi2_mono = p->chi2_mono; a.chi2_stereo = p->chi2_stereo;
    a.T_out = reinterpret_cast<double*>(B->d_out.p + out_T);
    a.chi2_out = reinterpret_cast<double*>(B->d_out.p + out_chi);
    a.iters_out = reinterpret_cast<int*>(B->d_out.p + out_it);
    a.inlier = B->d_out.p + out_lv;
  };
  rc = cs::batch_round_trip(*B, L.bytes, out.bytes, true, pack, [&] { cs::pose_launch(a, B->st); }); if (rc) return rc;

  std::memcpy(Tcw7_out, B->h_out.p + out_T, 7 * nf * 8);
  if (chi2_out) std::memcpy(chi2_out, B->h_out.p + out_chi, nf * R * 8);
  if (iterations_done) std::memcpy(iterations_done, B->h_out.p + out_it, nf * R * 4);
  if (n_obs) std::memcpy(inlier_out, B->h_out.p + out_lv, n_obs);
  B->host_ms = cs::now_ms() - t_begin;
  B->ran = true;
  return CS_OK;
}

int cs_pose_batch_last_timing(const cs_pose_batch* B, double* kernel_ms, double* host_ms) { return cs::batch_last_timing(B, kernel_ms, host_ms); }

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

int cs_pose_linearize_batch(int device, int robust, double huber_mono, double huber_stereo, int n_frames, const double* Tcw7_in, const double* intr5,
                            const int* obs_ptr, const double* Xw3, const double* meas3, const double* info9, const unsigned char* is_stereo,
                            double* H21, double* b6, double* chi2) {
  if (n_frames < 0) { cs_set_error("cs_pose_linearize_batch: a negative frame count"); return CS_ERR_INVALID_ARG; }
  if (n_frames == 0) return CS_OK;
  size_t n_obs = 0;
  int rc = check_frames("cs_pose_linearize_batch", n_frames, Tcw7_in, intr5, obs_ptr, Xw3, meas3, info9, is_stereo, &n_obs); if (rc) return rc;
  if (!H21 || !b6 || !chi2) { cs_set_error("cs_pose_linearize_batch: NULL output"); return CS_ERR_INVALID_ARG; }
  cs_pose_batch* B = nullptr;
  rc = cs_pose_batch_create(device, &B);
  if (rc) return rc;
  cs::Guard<cs_pose_batch> g(B, cs_pose_batch_destroy);     // (this call's own handle: never disarmed)
  const size_t nf = (size_t)n_frames;
  const InLayout L = in_layout(nf, n_obs);
  cs::Layout out;
  const size_t out_sys = out.add(nf * cs::POSE_SYSTEM_DOUBLES * 8), out_lv = out.add(n_obs);
  cs::PoseLaunch a;
  auto pack = [&] {
    pack_inputs(B->h_in.p, L, nf, n_obs, Tcw7_in, intr5, obs_ptr, Xw3, meas3, info9, is_stereo);
    set_inputs(a, B->d_in.p, L, n_frames);
    a.robust_rounds = robust ? 1 : 0;
    a.huber_mono = huber_mono; a.huber_stereo = huber_stereo;
    a.system_out = reinterpret_cast<double*>(B->d_out.p + out_sys);
    a.inlier = B->d_out.p + out_lv;
  };
  rc = cs::batch_round_trip(*B, L.bytes, out.bytes, false, pack, [&] { cs::pose_launch_linearize(a, B->st); }); if (rc) return rc;
  const double* sys = reinterpret_cast<const double*>(B->h_out.p + out_sys);
  for (size_t f = 0; f < nf; f++, sys += cs::POSE_SYSTEM_DOUBLES) {
    std::memcpy(H21 + 21 * f, sys, 21 * 8);
    std::memcpy(b6 + 6 * f, sys + 21, 6 * 8);
    chi2[f] = sys[27];
  }
  return CS_OK;
}

}  // extern "C"
