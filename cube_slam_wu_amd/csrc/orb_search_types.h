// orb_search_types.h -- what orb_search_host.cpp hands to orb_search_kernels.hip (guided ORB matching by projection, include/cubeslam_hip.h: cs_orb_search_*).
#pragma once
#include <hip/hip_runtime.h>

#include "cs_chunk.h"
#include "cs_orb_search.h"

namespace cs {

// ORB_CHUNK: queries of ONE job a wave handles, one per lane
enum { ORB_WAVES_PER_BLOCK = 4, ORB_CHUNK = 64 };

struct OrbLaunch {
  int n_chunks;
  OrbParams prm;
  // the resident frame set (cs_orb_search_set_frames)
  const OrbFrame* frame;           // n_frames (cs_orb_search.h: orb_frame_record)
  const int* start;                // every frame's cols rows + 1 cell starts, frame f's from frame[f].cell_first on
  const double* kp4;               // the sorted keypoints of all frames, ORB_KP_DOUBLES each, behind a 256-byte aligned base
  const int* orig;                 // ... their index in their frame
  const unsigned* desc;            // ... their ORB_DESC_WORDS words, behind a 256-byte aligned base
  // the call's
  const Chunk* chunk;              // n_chunks (cs_chunk.h; owner = the job), built by the host from query_ptr
  const OrbJob* job;               // n_jobs (orb_job_record)
  const double* q8;                // n_queries x ORB_QUERY_DOUBLES, behind a 256-byte aligned base
  const unsigned* qdesc;           // n_queries x ORB_DESC_WORDS, behind a 256-byte aligned base
  const unsigned char* skip;       // n_queries
  unsigned char* status;           // n_queries
  unsigned char* level;            // n_queries
  int* best_idx;                   // n_queries
  int* best_dist;                  // n_queries
  double* insp5;                   // cs_orb_search_inspect: n_queries x 5 (u v ur dist radius)
  int* n_window;                   // ... n_queries
  int* n_candidates;               // ... n_queries
};

// inspect: insp5, n_window and n_candidates are written too
void orb_search_launch(const OrbLaunch& a, bool inspect, hipStream_t st);

}  // namespace cs
