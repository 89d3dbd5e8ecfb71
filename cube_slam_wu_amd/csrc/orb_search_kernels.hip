// orb_search_kernels.hip -- guided ORB matching by projection, many (map points -> keyframe) jobs per launch (include/cubeslam_hip.h: cs_orb_search_*).
//
// The arithmetic is cs_orb_search.h's (the ORBmatcher::Fuse / SearchBySim3 steps it restates are named there); this file gives it its wave:
// ONE LANE, ONE QUERY, and one wavefront per chunk of at most ORB_CHUNK = 64 queries of ONE job.  The host builds the chunk table (job,
// first query, count), so the job's record and its frame's record -- [R | t], s, th, the gates, intrinsics, bounds, the level table --
// sit behind wave-uniform addresses and are read by scalar loads.  A lane reads its 64-byte query as four aligned double2s and its
// descriptor as two uint4s (8 VGPRs for the whole walk), projects, and walks the cells of its window: the host has laid each frame's
// keypoints out sorted by cell, column-major, stable in their index, so one cell column of a window is ONE contiguous run of 32-byte
// keypoint records and the statement's walk order is ascending memory order.  The lane keeps (best distance, first seen) under a strict
// `<`: the tie rule needs nothing else.  A keypoint's descriptor (32 bytes, two uint4 loads, 8 XORs and popcounts) is read only when it
// has passed the window, level and reprojection gates.
//
// Keypoints and descriptors are read through L1 / L2, not staged in LDS: a lane touches the few cells of its own window -- a handful of
// keypoints of a frame's 2 000 -- and the 64 windows of a wave lie anywhere in the image, so staging would read the whole 64 KB of a
// frame's descriptors per wave to use a few hundred bytes of them (DESIGN.md has the measured figures).
//
// No LDS, no barrier, no atomic, no cross-lane traffic: a wave without a chunk leaves at once, lanes past the chunk's count leave, and
// the OK queries of a job are counted by the host from the downloaded status bytes.  A query's result does not depend on its lane, its
// wave or its batch.  FP64, -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "cs_wave.h"
#include "orb_search_types.h"

namespace cs {
namespace {

static_assert(ORB_CHUNK == 64, "one query per lane");
static_assert(sizeof(OrbFrame) % 16 == 0 && sizeof(OrbJob) % 16 == 0 && sizeof(Chunk) == 16, "records behind aligned addresses");

template <bool INSPECT>
__global__ void __launch_bounds__(64 * ORB_WAVES_PER_BLOCK) orb_search_kernel(const OrbLaunch a) {
  Chunk ch;
  int lane;
  if (!wave_chunk<ORB_WAVES_PER_BLOCK>(a.chunk, a.n_chunks, ch, lane)) return;      // (a whole wavefront, or a lane past the count: there is no barrier in this kernel)
  const OrbJob& J = a.job[ch.owner];                 // wave-uniform
  const OrbFrame& F = a.frame[J.frame];              // wave-uniform
  const size_t i = (size_t)ch.first + lane;

  double q[ORB_QUERY_DOUBLES];
  load_record<ORB_QUERY_DOUBLES>(a.q8 + i * ORB_QUERY_DOUBLES, q);
  unsigned qd[ORB_DESC_WORDS];
  {
    const uint4* p = reinterpret_cast<const uint4*>(a.qdesc + i * ORB_DESC_WORDS);
    const uint4 lo = p[0], hi = p[1];
    qd[0] = lo.x; qd[1] = lo.y; qd[2] = lo.z; qd[3] = lo.w; qd[4] = hi.x; qd[5] = hi.y; qd[6] = hi.z; qd[7] = hi.w;
  }
  const int kp_first = F.kp_first;
  OrbQueryOut o;
  orb_search_query(F, J, a.prm, a.start + F.cell_first, a.kp4 + (size_t)kp_first * ORB_KP_DOUBLES, a.orig + kp_first, a.desc + (size_t)kp_first * ORB_DESC_WORDS, q, qd,
                   a.skip[i] != 0, o);

  a.status[i] = (unsigned char)o.status;
  a.level[i] = (unsigned char)o.level;
  a.best_idx[i] = o.best_idx;
  a.best_dist[i] = o.best_dist;
  if (INSPECT) {
    double* p = a.insp5 + ORB_INSPECT_DOUBLES * i;
    p[0] = o.u; p[1] = o.v; p[2] = o.ur; p[3] = o.dist; p[4] = o.radius;
    a.n_window[i] = o.n_window;
    a.n_candidates[i] = o.n_candidates;
  }
}

}  // namespace

void orb_search_launch(const OrbLaunch& a, bool inspect, hipStream_t st) {
  if (a.n_chunks <= 0) return;
  const int blocks = (a.n_chunks + ORB_WAVES_PER_BLOCK - 1) / ORB_WAVES_PER_BLOCK;
  if (inspect) hipLaunchKernelGGL(orb_search_kernel<true>, dim3(blocks), dim3(64 * ORB_WAVES_PER_BLOCK), 0, st, a);
  else hipLaunchKernelGGL(orb_search_kernel<false>, dim3(blocks), dim3(64 * ORB_WAVES_PER_BLOCK), 0, st, a);
}

}  // namespace cs
