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

// d_in = [T0 | intr | records | obs_ptr], d_out = [T_out | chi2 | iterations | inlier]
struct cs_pose_batch : cs::BatchHandle {};

namespace {

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

int cs_pose_batch_create(int device, cs_pose_batch** out) { return cs::batch_create(device, out); }

void cs_pose_batch_destroy(cs_pose_batch* B) { cs::batch_destroy(B); }

int cs_pose_batch_optimize(cs_pose_batch* B, const cs_pose_params* p, int n_frames, const double* Tcw7_in, const double* intr5, const int* obs_ptr,
                           const double* Xw3, const double* meas3, const double* info9, const unsigned char* is_stereo,
                           double* Tcw7_out, unsigned char* inlier_out, double* chi2_out, int* iterations_done) {
  if (!B || n_frames < 0) return CS_ERR_INVALID_ARG;
  int rc = check_params(p); if (rc) return rc;
  B->ran = false;
  if (n_frames == 0) { B->kernel_ms = B->host_ms = 0; B->ran = true; return CS_OK; }
  if (!Tcw7_in || !intr5 || !obs_ptr || !Tcw7_out) { cs_set_error("cs_pose_batch_optimize: NULL argument"); return CS_ERR_INVALID_ARG; }
  const double t_begin = cs::now_ms();
  rc = cs::check_partition("cs_pose_batch_optimize: obs_ptr", obs_ptr, n_frames); if (rc) return rc;
  const size_t n_obs = (size_t)obs_ptr[n_frames];
  if (n_obs > 0 && (!Xw3 || !meas3 || !info9 || !is_stereo || !inlier_out)) { cs_set_error("cs_pose_batch_optimize: NULL observation array"); return CS_ERR_INVALID_ARG; }
  const size_t R = (size_t)p->n_rounds, nf = (size_t)n_frames;

  // ---- layout of the two buffers
  cs::Layout in, out;
  const size_t in_T = in.add(7 * nf * 8), in_intr = in.add(5 * nf * 8), in_obs = in.add(n_obs * cs::POSE_OBS_DOUBLES * 8), in_ptr = in.add((nf + 1) * 4);
  const size_t out_T = out.add(7 * nf * 8), out_chi = out.add(nf * R * 8), out_it = out.add(nf * R * 4), out_lv = out.add(n_obs);

  cs::PoseLaunch a;
  auto pack = [&] {
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
  };
  rc = cs::batch_round_trip(*B, in.bytes, out.bytes, true, pack, [&] { cs::pose_launch(a, B->st); }); if (rc) return rc;

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

}  // extern "C"
