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
  const cs::Refuse refuse{"cs_pose"};
  if (!p || p->n_rounds < 1 || p->n_rounds > cs::POSE_MAX_ROUNDS) return refuse("n_rounds must be 1..8");
  for (int r = 0; r < p->n_rounds; r++)
    if (p->iterations[r] < 0) return refuse("negative iteration count");
  return CS_OK;
}

// What both entries check of their inputs.  *n_obs = obs_ptr[n_frames].
int check_frames(const char* who, int n_frames, const double* Tcw7_in, const double* intr5, const int* obs_ptr, const double* Xw3, const double* meas3,
                 const double* info9, const unsigned char* is_stereo, size_t* n_obs) {
  const cs::Refuse refuse{who};
  if (!Tcw7_in || !intr5 || !obs_ptr) return refuse("NULL argument");
  if (int rc = cs::check_partition(std::string(who) + ": obs_ptr", obs_ptr, n_frames)) return rc;
  *n_obs = (size_t)obs_ptr[n_frames];
  if (*n_obs > 0 && (!Xw3 || !meas3 || !info9 || !is_stereo)) return refuse("NULL observation array");
  return CS_OK;
}

// the parts of d_in, in their order
struct InLayout {
  cs::Layout all;
  cs::Part<double> T, intr, obs;
  cs::Part<int> ptr;
  InLayout(size_t nf, size_t n_obs)
      : T(all.add<double>(7 * nf)), intr(all.add<double>(5 * nf)), obs(all.add<double>(n_obs * cs::POSE_OBS_DOUBLES)), ptr(all.add<int>(nf + 1)) {}
};

void pack_inputs(cs::PinBuf<unsigned char>& h, const InLayout& L, size_t n_obs, const double* Tcw7_in, const double* intr5, const int* obs_ptr,
                 const double* Xw3, const double* meas3, const double* info9, const unsigned char* is_stereo) {
  cs::copy_in(L.T, h, Tcw7_in);
  cs::copy_in(L.intr, h, intr5);
  cs::copy_in(L.ptr, h, obs_ptr);
  double* rec = L.obs.at(h.p);
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
  a.T0 = L.T.at(d); a.intr = L.intr.at(d); a.obs = L.obs.at(d); a.obs_ptr = L.ptr.at(d);
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
  const cs::Refuse refuse{"cs_pose_batch_optimize"};
  cs::BatchCall call(*B);
  call.point_of_no_return();                           // (before the checks: cs_batch_handle.h, BatchCall)
  if (n_frames == 0) return call.empty();
  if (!Tcw7_out) return refuse("NULL argument");
  size_t n_obs = 0;
  rc = check_frames("cs_pose_batch_optimize", n_frames, Tcw7_in, intr5, obs_ptr, Xw3, meas3, info9, is_stereo, &n_obs); if (rc) return rc;
  if (n_obs > 0 && !inlier_out) return refuse("NULL observation array");
  const size_t R = (size_t)p->n_rounds, nf = (size_t)n_frames;

  // ---- layout of the two buffers
  const InLayout L(nf, n_obs);
  cs::Layout out;
  const auto out_T = out.add<double>(7 * nf), out_chi = out.add<double>(nf * R);
  const auto out_it = out.add<int>(nf * R);
  const auto out_lv = out.add<unsigned char>(n_obs);

  cs::PoseLaunch a;
  auto pack = [&] {
    pack_inputs(B->h_in, L, n_obs, Tcw7_in, intr5, obs_ptr, Xw3, meas3, info9, is_stereo);
    set_inputs(a, B->d_in.p, L, n_frames);
    a.n_rounds = p->n_rounds;
    for (int r = 0; r < cs::POSE_MAX_ROUNDS; r++) a.iterations[r] = r < p->n_rounds ? p->iterations[r] : 0;
    a.robust_rounds = p->robust_rounds; a.restart_each_round = p->restart_each_round ? 1 : 0;
    a.huber_mono = p->huber_mono; a.huber_stereo = p->huber_stereo; a.chi2_mono = p->chi2_mono; a.chi2_stereo = p->chi2_stereo;
    a.T_out = out_T.at(B->d_out.p); a.chi2_out = out_chi.at(B->d_out.p); a.iters_out = out_it.at(B->d_out.p); a.inlier = out_lv.at(B->d_out.p);
  };
  rc = cs::batch_round_trip(*B, L.all.bytes, out.bytes, true, pack, [&] { cs::pose_launch(a, B->st); }); if (rc) return rc;

  cs::copy_out(out_T, B->h_out, Tcw7_out);
  if (chi2_out) cs::copy_out(out_chi, B->h_out, chi2_out);
  if (iterations_done) cs::copy_out(out_it, B->h_out, iterations_done);
  if (n_obs) cs::copy_out(out_lv, B->h_out, inlier_out);
  return call.done();
}

int cs_pose_batch_last_timing(const cs_pose_batch* B, double* kernel_ms, double* host_ms) { return cs::batch_last_timing(B, kernel_ms, host_ms); }

int cs_pose_optimize_batch(int device, const cs_pose_params* p, int n_frames, const double* Tcw7_in, const double* intr5, const int* obs_ptr,
                           const double* Xw3, const double* meas3, const double* info9, const unsigned char* is_stereo,
                           double* Tcw7_out, unsigned char* inlier_out, double* chi2_out, int* iterations_done) {
  return cs::batch_one_shot<cs_pose_batch>(device, [&](cs_pose_batch* B) -> int {
    return cs_pose_batch_optimize(B, p, n_frames, Tcw7_in, intr5, obs_ptr, Xw3, meas3, info9, is_stereo, Tcw7_out, inlier_out, chi2_out, iterations_done);
  });
}

int cs_pose_linearize_batch(int device, int robust, double huber_mono, double huber_stereo, int n_frames, const double* Tcw7_in, const double* intr5,
                            const int* obs_ptr, const double* Xw3, const double* meas3, const double* info9, const unsigned char* is_stereo,
                            double* H21, double* b6, double* chi2) {
  const cs::Refuse refuse{"cs_pose_linearize_batch"};
  if (n_frames < 0) return refuse("a negative frame count");
  if (n_frames == 0) return CS_OK;
  size_t n_obs = 0;
  int rc = check_frames("cs_pose_linearize_batch", n_frames, Tcw7_in, intr5, obs_ptr, Xw3, meas3, info9, is_stereo, &n_obs); if (rc) return rc;
  if (!H21 || !b6 || !chi2) return refuse("NULL output");
  return cs::batch_one_shot<cs_pose_batch>(device, [&](cs_pose_batch* B) -> int {
    const size_t nf = (size_t)n_frames;
    const InLayout L(nf, n_obs);
    cs::Layout out;
    const auto out_sys = out.add<double>(nf * cs::POSE_SYSTEM_DOUBLES);
    const auto out_lv = out.add<unsigned char>(n_obs);
    cs::PoseLaunch a;
    auto pack = [&] {
      pack_inputs(B->h_in, L, n_obs, Tcw7_in, intr5, obs_ptr, Xw3, meas3, info9, is_stereo);
      set_inputs(a, B->d_in.p, L, n_frames);
      a.robust_rounds = robust ? 1 : 0;
      a.huber_mono = huber_mono; a.huber_stereo = huber_stereo;
      a.system_out = out_sys.at(B->d_out.p); a.inlier = out_lv.at(B->d_out.p);
    };
    rc = cs::batch_round_trip(*B, L.all.bytes, out.bytes, false, pack, [&] { cs::pose_launch_linearize(a, B->st); }); if (rc) return rc;
    const double* sys = out_sys.at(B->h_out.p);
    for (size_t f = 0; f < nf; f++, sys += cs::POSE_SYSTEM_DOUBLES) {
      std::memcpy(H21 + 21 * f, sys, 21 * 8);
      std::memcpy(b6 + 6 * f, sys + 21, 6 * 8);
      chi2[f] = sys[27];
    }
    return CS_OK;
  });
}

}  // extern "C"
