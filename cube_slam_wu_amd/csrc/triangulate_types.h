// triangulate_types.h -- what triangulate_host.cpp hands to triangulate_kernels.hip (two-view triangulation of new map points, include/cubeslam_hip.h: cs_triangulate_*).
#pragma once
#include <hip/hip_runtime.h>

#include "cs_chunk.h"
#include "cs_triangulate.h"

namespace cs {

// TRI_CHUNK: matches of ONE pair a wave handles, one per lane
enum { TRI_WAVES_PER_BLOCK = 4, TRI_CHUNK = 64 };

struct TriLaunch {
  int n_chunks;
  TriParams prm;
  const Chunk* chunk;              // n_chunks (cs_chunk.h; owner = the pair), built by the host from match_ptr
  const TriPair* pair;             // n_pairs (cs_triangulate.h: triangulate_pair_record)
  const double* rec;               // n_matches x TRI_MATCH_DOUBLES, behind a 256-byte aligned base
  double* out8;                    // n_matches x TRI_OUT_DOUBLES, behind a 256-byte aligned base
  unsigned char* status;           // n_matches
  unsigned char* route;            // n_matches
  double* cos3;                    // cs_triangulate_inspect: n_matches x 3 (cosRays cosS1 cosS2)
};

// inspect: cos3 is written too
void triangulate_launch(const TriLaunch& a, bool inspect, hipStream_t st);

}  // namespace cs
