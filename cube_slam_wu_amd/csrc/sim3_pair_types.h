// sim3_pair_types.h -- what sim3_pair_host.cpp hands to sim3_pair_kernels.hip (Sim(3) alignment of keyframe pairs, include/cubeslam_hip.h: cs_sim3_*).
#pragma once
#include <hip/hip_runtime.h>

#include "cs_sim3_pair.h"

namespace cs {

enum { SIM3_PAIR_WAVES_PER_BLOCK = 4 };

struct Sim3PairLaunch {
  int n_pairs;
  Sim3PairSchedule sched;
  const double* S0;                // n_pairs x 8
  const double* intr;              // n_pairs x 8: fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2
  const unsigned char* fix_scale;  // n_pairs
  const int* match_ptr;            // n_pairs + 1
  const double* rec;               // match_ptr[n_pairs] x SIM3_PAIR_MATCH_DOUBLES (cs_sim3_pair.h), behind a 256-byte aligned base
  // cs_sim3_optimize_pairs
  double* S_out;                   // n_pairs x 8
  double* chi2_out;                // n_pairs x 2
  int* iters_out;                  // n_pairs x 2
  int* n_inliers;                  // n_pairs
  unsigned char* inlier;           // match_ptr[n_pairs]: a match's level between the rounds, and the result
  // cs_sim3_pairs_linearize
  double* err;                     // match_ptr[n_pairs] x 4
  double* jac;                     // match_ptr[n_pairs] x 28
};

void sim3_pair_launch(const Sim3PairLaunch& a, hipStream_t st);
void sim3_pair_launch_linearize(const Sim3PairLaunch& a, hipStream_t st);

}  // namespace cs
