// pose_kernels.hip -- motion-only pose optimisation, many frames per launch (include/cubeslam_hip.h: cs_pose_*).
//
// One frame is a g2o graph of ONE free VertexSE3Expmap and the frame's unary edges
//   EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose   object_slam/Thirdparty/g2o/g2o/types/types_six_dof_expmap.h:208-267
//   computeError / cam_project / linearizeOplus                   types/types_six_dof_expmap.cpp:311-408
//   constructQuadraticForm (rho' weights Omega and -Omega e)      core/base_unary_edge.hpp:42-72
//   RobustKernelHuber with its single-precision delta^2           cs_robust.h
//   VertexSE3Expmap::oplusImpl (exp(update) * estimate)           types_six_dof_expmap.h:73-76, cs_se3.h
// driven round by round through cs_dense_lm.h's dense_lm_round with N = 6: SparseOptimizer::optimize with OptimizationAlgorithmLevenberg
// over a 6 x 6 LDL^T without pivoting (the g2o lines are cited there and in cs_lm.h).
//
// Shape: one wavefront per frame, the whole optimisation -- every round, iteration and trial -- inside one launch.  Lane l owns the frame's
// observations l, l + 64, ...: it keeps their share of the 21 upper entries of H, of b and of chi2 in registers; the 64 shares are summed
// by cs_wave.h's wave_sum_all (a butterfly over the lanes: a fixed order, and the same bits in every lane).  Every lane therefore holds the same H and b, and every lane runs the 6 x 6 factorisation on them: on a SIMD machine that
// costs what one lane costs, and the increment needs no broadcast.  All LM scalars are wave-uniform, so the control flow never diverges.
// A frame's result depends on its own data only: the same bits at any position in any batch.  FP64, -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "cs_dense_lm.h"
#include "cs_robust.h"
#include "cs_wave.h"
#include "pose_types.h"

namespace cs {
namespace {

struct Obs {
  double X[3], m[3], W[9];
  bool stereo;
};

__device__ __forceinline__ Obs obs_load(const double* __restrict__ rec) {
  double v[POSE_OBS_DOUBLES];
  load_record<POSE_OBS_DOUBLES>(rec, v);             // 128 bytes
  Obs o;
#pragma unroll
  for (int k = 0; k < 3; k++) { o.X[k] = v[k]; o.m[k] = v[3 + k]; }
#pragma unroll
  for (int k = 0; k < 9; k++) o.W[k] = v[6 + k];
  o.stereo = v[15] != 0.0;
  return o;
}

// computeError of the two edges (types_six_dof_expmap.h:218-222, :249-253) with their cam_project (.cpp:335-351).  The stereo edge's
// cam_project holds 1 / z in a `const float` (.cpp:345; the division itself is a double one, its operand being a double); its bf is the
// double member.  A mono edge's third component is 0.
__device__ __forceinline__ void obs_error(const Pose& T, const double* intr, const Obs& o, double* e, double* pc) {
  pose_map(T, o.X, pc);
  if (o.stereo) {
    const double invz = (double)(float)(1.0 / pc[2]);
    const double u = pc[0] * invz * intr[0] + intr[2];
    e[0] = o.m[0] - u;
    e[1] = o.m[1] - (pc[1] * invz * intr[1] + intr[3]);
    e[2] = o.m[2] - (u - intr[4] * invz);
  } else {
    e[0] = o.m[0] - (pc[0] / pc[2] * intr[0] + intr[2]);      // project2d, then * fx + cx
    e[1] = o.m[1] - (pc[1] / pc[2] * intr[1] + intr[3]);
    e[2] = 0.0;
  }
}

// e^T Omega e (BaseEdge::chi2) and Omega e
__device__ __forceinline__ double obs_chi2(const Obs& o, const double* e, double* We) {
#pragma unroll
  for (int i = 0; i < 3; i++) We[i] = (o.W[3 * i] * e[0] + o.W[3 * i + 1] * e[1]) + o.W[3 * i + 2] * e[2];
  return (e[0] * We[0] + e[1] * We[1]) + e[2] * We[2];
}

struct Frame {
  const double* obs;            // the frame's first record
  unsigned char* level;         // 1 = level 0 (optimised), 0 = level 1 (left out), per observation of the frame
  int n;
  double intr[5];
  double huber_mono, huber_stereo;
};

// activeRobustChi2 at pose T over the frame's level-0 observations (sparse_optimizer.cpp:100-114)
__device__ __forceinline__ double frame_chi2(const Frame& F, const Pose& T, bool robust, int lane) {
  double acc = 0.0;
  for (int i = lane; i < F.n; i += 64) {
    if (!F.level[i]) continue;
    const Obs o = obs_load(F.obs + (size_t)i * POSE_OBS_DOUBLES);
    double e[3], pc[3], We[3];
    obs_error(T, F.intr, o, e, pc);
    const double c = obs_chi2(o, e, We);
    double r0, r1;
    huber_rho(c, robust ? (o.stereo ? F.huber_stereo : F.huber_mono) : 0.0, r0, r1);
    acc += r0;
  }
  return wave_sum_all(acc);
}

// computeActiveErrors + linearizeOplus + constructQuadraticForm of every level-0 edge: H (21 upper entries, row by row), b, chi2
__device__ __forceinline__ void frame_linearize(const Frame& F, const Pose& T, bool robust, int lane, double* H, double* b, double& chi) {
  double h[21], g[6], acc = 0.0;
#pragma unroll
  for (int k = 0; k < 21; k++) h[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; k++) g[k] = 0.0;
  for (int i = lane; i < F.n; i += 64) {
    if (!F.level[i]) continue;
    const Obs o = obs_load(F.obs + (size_t)i * POSE_OBS_DOUBLES);
    double e[3], pc[3], We[3];
    obs_error(T, F.intr, o, e, pc);
    const double c = obs_chi2(o, e, We);
    double r0, r1;
    huber_rho(c, robust ? (o.stereo ? F.huber_stereo : F.huber_mono) : 0.0, r0, r1);
    acc += r0;
    // linearizeOplus (.cpp:311-333, :380-409)
    const double fx = F.intr[0], fy = F.intr[1], bf = F.intr[4];
    const double x = pc[0], y = pc[1], invz = 1.0 / pc[2], invz_2 = invz * invz;
    double J[18];
    J[0] = x * y * invz_2 * fx;
    J[1] = -(1 + (x * x * invz_2)) * fx;
    J[2] = y * invz * fx;
    J[3] = -invz * fx;
    J[4] = 0;
    J[5] = x * invz_2 * fx;
    J[6] = (1 + y * y * invz_2) * fy;
    J[7] = -x * y * invz_2 * fy;
    J[8] = -x * invz * fy;
    J[9] = 0;
    J[10] = -invz * fy;
    J[11] = y * invz_2 * fy;
    if (o.stereo) {
      J[12] = J[0] - bf * y * invz_2;
      J[13] = J[1] + bf * x * invz_2;
      J[14] = J[2];
      J[15] = J[3];
      J[16] = 0;
      J[17] = J[5] - bf * invz_2;
    } else {
#pragma unroll
      for (int k = 12; k < 18; k++) J[k] = 0.0;
    }
    // b -= rho' A^T Omega e;  A += A^T (rho' Omega) A   (base_unary_edge.hpp:56-66; without a kernel rho' = 1)
    double WJ[18];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int a = 0; a < 6; a++) WJ[6 * r + a] = r1 * ((o.W[3 * r] * J[a] + o.W[3 * r + 1] * J[6 + a]) + o.W[3 * r + 2] * J[12 + a]);
    int k = 0;
#pragma unroll
    for (int a = 0; a < 6; a++) {
      g[a] -= r1 * ((J[a] * We[0] + J[6 + a] * We[1]) + J[12 + a] * We[2]);
#pragma unroll
      for (int c2 = a; c2 < 6; c2++, k++) h[k] += (J[a] * WJ[c2] + J[6 + a] * WJ[6 + c2]) + J[12 + a] * WJ[12 + c2];
    }
  }
#pragma unroll
  for (int k = 0; k < 21; k++) H[k] = wave_sum_all(h[k]);
#pragma unroll
  for (int k = 0; k < 6; k++) b[k] = wave_sum_all(g[k]);
  chi = wave_sum_all(acc);
}

// The caller's classification between two optimize() calls: every observation, current outliers included, by its plain chi2.
// Returns the observations left at level 0, the same number in every lane.
__device__ __forceinline__ int frame_classify(const Frame& F, const Pose& T, double chi2_mono, double chi2_stereo, int lane) {
  int left = 0;
  for (int i = lane; i < F.n; i += 64) {
    const Obs o = obs_load(F.obs + (size_t)i * POSE_OBS_DOUBLES);
    double e[3], pc[3], We[3];
    obs_error(T, F.intr, o, e, pc);
    const double c = obs_chi2(o, e, We);
    const double thr = o.stereo ? chi2_stereo : chi2_mono;
    const unsigned char in = (thr > 0 && c > thr) ? 0 : 1;
    F.level[i] = in;
    left += in;
  }
  return wave_sum_all(left);
}

// The frame as cs_dense_lm.h's problem: one free VertexSE3Expmap under the frame's level-0 edges
struct FrameLm {
  const Frame& F;
  bool robust;
  int lane;
  __device__ __forceinline__ void linearize(const Pose& T, double* H, double* b, double& chi) const { frame_linearize(F, T, robust, lane, H, b, chi); }
  __device__ __forceinline__ double chi2(const Pose& T) const { return frame_chi2(F, T, robust, lane); }
  __device__ __forceinline__ Pose oplus(const Pose& T, const double* x) const { return cam_oplus(T, x); }
};

// frame f of a launch
__device__ __forceinline__ Frame frame_of(const PoseLaunch& a, int f) {
  Frame F;
  const int o0 = a.obs_ptr[f];
  F.n = a.obs_ptr[f + 1] - o0;
  F.obs = a.obs + (size_t)o0 * POSE_OBS_DOUBLES;
  F.level = a.inlier + o0;
#pragma unroll
  for (int k = 0; k < 5; k++) F.intr[k] = a.intr[5 * f + k];
  F.huber_mono = a.huber_mono; F.huber_stereo = a.huber_stereo;
  return F;
}

__global__ void __launch_bounds__(64 * POSE_WAVES_PER_BLOCK) pose_batch_kernel(const PoseLaunch a) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * POSE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
  if (f >= a.n_frames) return;                       // (a whole wavefront leaves: there is no barrier in this kernel)
  const Frame F = frame_of(a, f);
  Pose T0 = pose_load(a.T0 + 7 * f);
  pose_normalize(T0);                                // SE3Quat(const Vector7d&) normalises (types/se3quat.h:67-70)
  Pose T = T0;
  // every edge starts at level 0.  A lane reads back only what it wrote itself (observation i belongs to lane i & 63 throughout).
  for (int i = lane; i < F.n; i += 64) F.level[i] = 1;
  int n_act = F.n;                                   // level-0 edges, the same in every lane

  for (int r = 0; r < a.n_rounds; r++) {
    if (a.restart_each_round) T = T0;
    const bool robust = r < a.robust_rounds;
    int done = 0;
    double currentChi = 0.0;
    if (n_act > 0) done = dense_lm_round<6>(FrameLm{F, robust, lane}, T, a.iterations[r], 10, currentChi);
    if (lane == 0) {
      a.iters_out[f * a.n_rounds + r] = done;
      a.chi2_out[f * a.n_rounds + r] = currentChi;
    }
    n_act = frame_classify(F, T, a.chi2_mono, a.chi2_stereo, lane);
  }
  if (lane == 0) pose_store(T, a.T_out + 7 * f);
}

// Inspection (cs_pose_linearize_batch): frame_linearize, the routine every iteration above starts with, once per frame at its normalised
// T0 with every observation at level 0.  Lane 0 stores H (21), b (6) and chi2 (every lane holds the same sums).
__global__ void __launch_bounds__(64 * POSE_WAVES_PER_BLOCK) pose_linearize_kernel(const PoseLaunch a) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x * POSE_WAVES_PER_BLOCK + (threadIdx.x >> 6);
  if (f >= a.n_frames) return;
  const Frame F = frame_of(a, f);
  Pose T = pose_load(a.T0 + 7 * f);
  pose_normalize(T);
  for (int i = lane; i < F.n; i += 64) F.level[i] = 1;      // (read back by the lane that wrote it, as above)
  double H[21], b[6], chi;
  frame_linearize(F, T, a.robust_rounds != 0, lane, H, b, chi);
  if (lane == 0) {
    double* out = a.system_out + (size_t)f * POSE_SYSTEM_DOUBLES;
#pragma unroll
    for (int k = 0; k < 21; k++) out[k] = H[k];
#pragma unroll
    for (int k = 0; k < 6; k++) out[21 + k] = b[k];
    out[27] = chi;
  }
}

}  // namespace

void pose_launch(const PoseLaunch& a, hipStream_t st) {
  if (a.n_frames <= 0) return;
  const int blocks = (a.n_frames + POSE_WAVES_PER_BLOCK - 1) / POSE_WAVES_PER_BLOCK;
  hipLaunchKernelGGL(pose_batch_kernel, dim3(blocks), dim3(64 * POSE_WAVES_PER_BLOCK), 0, st, a);
}

void pose_launch_linearize(const PoseLaunch& a, hipStream_t st) {
  if (a.n_frames <= 0) return;
  const int blocks = (a.n_frames + POSE_WAVES_PER_BLOCK - 1) / POSE_WAVES_PER_BLOCK;
  hipLaunchKernelGGL(pose_linearize_kernel, dim3(blocks), dim3(64 * POSE_WAVES_PER_BLOCK), 0, st, a);
}

}  // namespace cs
