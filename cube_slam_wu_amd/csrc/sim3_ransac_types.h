// sim3_ransac_types.h -- what sim3_ransac_host.cpp hands to sim3_ransac_kernels.hip (Sim(3) RANSAC of keyframe pairs, include/cubeslam_hip.h: cs_sim3_ransac_*).
#pragma once
#include <hip/hip_runtime.h>

#include "cs_sim3_ransac.h"

namespace cs {

// SIM3_RANSAC_CHUNK: matches a wave stages at a time, one per lane
enum { SIM3_RANSAC_WAVES_PER_BLOCK = 4, SIM3_RANSAC_CHUNK = 64 };

struct Sim3RansacLaunch {
  int n_pairs;
  int min_inliers;
  int n_hyp;                       // the inspection form: hypotheses per pair, 1 .. SIM3_RANSAC_MAX_ITERATIONS
  const double* intr;              // n_pairs x 8: fx1 fy1 cx1 cy1 fx2 fy2 cx2 cy2
  const unsigned char* fix_scale;  // n_pairs
  const unsigned long long* seed;  // n_pairs
  const int* match_ptr;            // n_pairs + 1
  const int* max_its;              // n_pairs: sim3_ransac_budget, 0 = the pair is not run
  const double* rec;               // match_ptr[n_pairs] x SIM3_RANSAC_MATCH_DOUBLES (cs_sim3_ransac.h), behind a 256-byte aligned base
  // cs_sim3_ransac_pairs
  int* found;                      // n_pairs
  int* hyp;                        // n_pairs
  int* iterations;                 // n_pairs
  int* n_inliers;                  // n_pairs
  double* S_out;                   // n_pairs x 8
  unsigned char* inlier;           // match_ptr[n_pairs]
  // cs_sim3_ransac_hypotheses
  double* S_each;                  // n_pairs x n_hyp x 8
  int* count_each;                 // n_pairs x n_hyp
};

// inspect: every one of n_hyp hypotheses per pair to S_each / count_each, no selection
void sim3_ransac_launch(const Sim3RansacLaunch& a, bool inspect, hipStream_t st);

}  // namespace cs
