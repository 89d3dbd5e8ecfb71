// pose_types.h -- what pose_host.cpp hands to pose_kernels.hip (motion-only pose optimisation, include/cubeslam_hip.h: cs_pose_*).
#pragma once
#include <hip/hip_runtime.h>

namespace cs {

// One observation as the kernel reads it: 16 doubles = 128 bytes, one cache line per lane.
//   [0..2] Xw   [3..5] measurement (u, v, u_r; mono: u, v, 0)   [6..14] information, row-major 3 x 3 (mono: the upper-left 2 x 2, zeros elsewhere)
//   [15] 1.0 = EdgeStereoSE3ProjectXYZOnlyPose, 0.0 = EdgeSE3ProjectXYZOnlyPose
// POSE_SYSTEM_DOUBLES: what the inspection entry stores per frame -- H (21 upper entries, row by row), b (6), activeRobustChi2 (1)
enum { POSE_OBS_DOUBLES = 16, POSE_MAX_ROUNDS = 8, POSE_WAVES_PER_BLOCK = 4, POSE_SYSTEM_DOUBLES = 28 };

struct PoseLaunch {
  int n_frames, n_rounds;
  int iterations[POSE_MAX_ROUNDS];
  int robust_rounds, restart_each_round;
  double huber_mono, huber_stereo, chi2_mono, chi2_stereo;
  const double* T0;        // n_frames x 7
  const double* intr;      // n_frames x 5: fx fy cx cy bf
  const int* obs_ptr;      // n_frames + 1
  const double* obs;       // obs_ptr[n_frames] x POSE_OBS_DOUBLES
  double* T_out;           // n_frames x 7
  double* chi2_out;        // n_frames x n_rounds
  int* iters_out;          // n_frames x n_rounds
  unsigned char* inlier;   // obs_ptr[n_frames]: the level of every observation between the rounds, and the result
  double* system_out;      // pose_launch_linearize only: n_frames x POSE_SYSTEM_DOUBLES
};

void pose_launch(const PoseLaunch& a, hipStream_t st);
// Inspection (cs_pose_linearize_batch): the system of every frame at its normalised T0 over all its observations.  Of the schedule it
// reads robust_rounds alone (!= 0: the Huber kernel is on) with the two widths; it writes system_out, and inlier (all ones).
void pose_launch_linearize(const PoseLaunch& a, hipStream_t st);

}  // namespace cs
