// triangulate_kernels.hip -- two-view triangulation of new map points, many keyframe pairs per launch (include/cubeslam_hip.h: cs_triangulate_*).
//
// The arithmetic is cs_triangulate.h's (the CreateNewMapPoints steps it restates are named there); this file gives it its wave: ONE LANE,
// ONE MATCH, and one wavefront per chunk of at most TRI_CHUNK = 64 matches of ONE pair.  The host builds the chunk table (pair, first
// match, count), so everything per pair -- both [R | t], both centres, both intrinsics, the ran flag -- sits behind a wave-uniform address
// and is read once per wave by scalar loads, not once per lane.  The pair's record is made once per pair on the host by
// triangulate_pair_record: a match's result does not depend on where its pair stands in a batch.  A lane reads its 96-byte match as six
// aligned double2s and writes its 64-byte result as four; status and route are a byte each.
//
// No LDS, no barrier, no atomic: a wave without a chunk leaves at once, lanes past the chunk's count leave, and the accepted matches of a
// pair are counted by the host from the downloaded status bytes.  The only loop is the Jacobi's 8 sweeps.  The routes diverge inside a wave
// (the linear triangulation runs under the mask of the lanes that take it).  FP64, -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "cs_wave.h"
#include "triangulate_types.h"

namespace cs {
namespace {

static_assert(TRI_CHUNK == 64, "one match per lane");
static_assert(sizeof(TriPair) % 16 == 0 && sizeof(Chunk) == 16, "records behind aligned addresses");

template <bool INSPECT>
__global__ void __launch_bounds__(64 * TRI_WAVES_PER_BLOCK) triangulate_kernel(const TriLaunch a) {
  Chunk ch;
  int lane;
  if (!wave_chunk<TRI_WAVES_PER_BLOCK>(a.chunk, a.n_chunks, ch, lane)) return;      // (a whole wavefront, or a lane past the count: there is no barrier in this kernel)
  const TriPair& P = a.pair[ch.owner];               // wave-uniform
  const size_t i = (size_t)ch.first + lane;

  double m[TRI_MATCH_DOUBLES];
  load_record<TRI_MATCH_DOUBLES>(a.rec + i * TRI_MATCH_DOUBLES, m);
  TriMatchOut o;
  triangulate_match(P, a.prm, m, o);

  double r[TRI_OUT_DOUBLES];
  triangulate_store(o, r);
  double2* dst = reinterpret_cast<double2*>(a.out8 + i * TRI_OUT_DOUBLES);
#pragma unroll
  for (int k = 0; k < TRI_OUT_DOUBLES / 2; k++) dst[k] = make_double2(r[2 * k], r[2 * k + 1]);
  a.status[i] = (unsigned char)o.status;
  a.route[i] = (unsigned char)o.route;
  if (INSPECT) {
    a.cos3[3 * i] = o.cosRays;
    a.cos3[3 * i + 1] = o.cosS1;
    a.cos3[3 * i + 2] = o.cosS2;
  }
}

}  // namespace

void triangulate_launch(const TriLaunch& a, bool inspect, hipStream_t st) {
  if (a.n_chunks <= 0) return;
  const int blocks = (a.n_chunks + TRI_WAVES_PER_BLOCK - 1) / TRI_WAVES_PER_BLOCK;
  if (inspect) hipLaunchKernelGGL(triangulate_kernel<true>, dim3(blocks), dim3(64 * TRI_WAVES_PER_BLOCK), 0, st, a);
  else hipLaunchKernelGGL(triangulate_kernel<false>, dim3(blocks), dim3(64 * TRI_WAVES_PER_BLOCK), 0, st, a);
}

}  // namespace cs
