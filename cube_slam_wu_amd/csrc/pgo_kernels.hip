// pgo_kernels.hip -- device side of the Sim(3) pose-graph optimisation (include/cubeslam_hip.h: cs_pgo_*; host: pgo_host.cpp).
//
//   pgo_edge_kernel            EdgeSim3 (types_seven_dof_expmap.h:99-126) with BaseBinaryEdge's numeric Jacobians (base_binary_edge.hpp:130-205):
//                              one edge on a half-wave -- lanes 0-13 the +delta evaluation of update coordinate d (0-6: vertex i, 7-13:
//                              vertex j), lanes 14-27 the -delta one, lane 28 the unperturbed error --, two edges per wavefront.  Writes e, J_i,
//                              J_j and the edge's terms of the quadratic form (base_binary_edge.hpp:55-120, no robust kernel).
//   pgo_error_kernel           e and e^T Omega e alone, a thread per edge (after a trial's update).
//   pgo_assemble_*_kernel      vertex-major gather of the diagonal blocks and b over a CSR of incident edges, in the CSR's order; every
//                              off-diagonal block has one edge.  Plain stores only: two runs give the same bits.
//   pgo_reduce_kernel<KIND>    chi2, the LM scale term, max |H_jj|: one workgroup, strided partial sums in index order, then a fixed LDS tree.
//   pgo_update_kernel          VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69).
//   pgo_se3_kernel, pgo_correct_points_kernel   what Optimizer::OptimizeEssentialGraph does with the result.
// Every index a kernel uses comes from arrays the host has validated (pgo_host.cpp); nothing is indexed by a computed value.
#include <hip/hip_runtime.h>

#include "cs_sim3.h"
#include "pgo_types.h"

namespace cs {

namespace {

// sum_c a[c] b[c], c ascending: the one order every product of this file uses
__device__ __forceinline__ double dot7(const double* a, const double* b) {
  double s = 0.0;
#pragma unroll
  for (int c = 0; c < 7; c++) s += a[c] * b[c];
  return s;
}

__global__ __launch_bounds__(64) void pgo_edge_kernel(PgoView v) {
  __shared__ double J[PGO_EDGES_PER_BLOCK][15][7];     // columns 0-13: d e / d update coordinate, column 14: e
  __shared__ double OJ[PGO_EDGES_PER_BLOCK][15][7];    // Omega times each of them
  __shared__ double W[PGO_EDGES_PER_BLOCK][49];
  const int tid = threadIdx.x, sub = tid >> 5, h = tid & 31;
  const int k = blockIdx.x * PGO_EDGES_PER_BLOCK + sub;
  const bool live = k < v.ne;
  const double delta = 1e-9, scalar = 1.0 / (2 * delta);
  double e[7] = {0, 0, 0, 0, 0, 0, 0};
  bool on = false;
  if (live) {
    const int vi = v.ei[k], vj = v.ej[k];
    Sim3 Si = sim3_load(v.est + 8 * (size_t)vi), Sj = sim3_load(v.est + 8 * (size_t)vj);
    const Sim3 M = sim3_load(v.meas + 8 * (size_t)k);
    const bool pert = h < 28;
    const int d = h < 14 ? h : h - 14;
    const bool side_j = d >= 7;
    const int c = side_j ? d - 7 : d;
    on = pert && v.vcol[side_j ? vj : vi] >= 0;        // (a fixed vertex gets no Jacobian)
    if (on) {
      const double step = h < 14 ? delta : -delta;
      double u[7];
#pragma unroll
      for (int i = 0; i < 7; i++) u[i] = i == c ? step : 0.0;
      const bool fs = v.fix_scale[side_j ? vj : vi] != 0;
      const Sim3 P = sim3_oplus(side_j ? Sj : Si, u, fs);
      if (side_j) Sj = P; else Si = P;
    }
    if (on || h == 28) sim3_edge_error(M, Si, Sj, e);
    for (int t = h; t < 49; t += 32) W[sub][t] = v.info[49 * (size_t)k + t];
  }
  // the -delta error of a column sits 14 lanes up (every lane takes part in the exchange)
  const int src = h < 14 ? tid + 14 : tid;
#pragma unroll
  for (int r = 0; r < 7; r++) {
    const double e2 = __shfl(e[r], src);
    if (live && h < 14) J[sub][h][r] = on ? scalar * (e[r] - e2) : 0.0;
    if (live && h == 28) J[sub][14][r] = e[r];
  }
  __syncthreads();
  if (live && h < 15) {
#pragma unroll
    for (int r = 0; r < 7; r++) OJ[sub][h][r] = dot7(&W[sub][7 * r], J[sub][h]);
  }
  __syncthreads();
  if (!live) return;
  const size_t k7 = 7 * (size_t)k, k49 = 49 * (size_t)k;
  for (int o = h; o < 162; o += 32) {
    if (o < 147) {
      const int blk = o / 49, t = o - 49 * blk, a = t / 7, b = t - 7 * a;
      const double s = dot7(J[sub][(blk == 2 ? 7 : 0) + a], OJ[sub][(blk == 0 ? 0 : 7) + b]);
      (blk == 0 ? v.Hii : (blk == 1 ? v.Hij : v.Hjj))[k49 + t] = s;
    } else if (o < 161) {
      const int a = o - 147;                             // omega_r = -Omega e (base_binary_edge.hpp:74)
      const double s = -dot7(J[sub][a], OJ[sub][14]);
      if (a < 7) v.bi[k7 + a] = s; else v.bj[k7 + a - 7] = s;
    } else {
      v.chi2_each[k] = dot7(J[sub][14], OJ[sub][14]);
    }
  }
  for (int o = h; o < 105; o += 32) {
    if (o < 98) {
      const int side = o / 49, t = o - 49 * side, r = t / 7, c = t - 7 * r;
      (side ? v.Jj : v.Ji)[k49 + t] = J[sub][7 * side + c][r];
    } else {
      v.err[k7 + o - 98] = J[sub][14][o - 98];
    }
  }
}

__global__ __launch_bounds__(64) void pgo_error_kernel(PgoView v) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= v.ne) return;
  double e[7], Oe[7];
  sim3_edge_error(sim3_load(v.meas + 8 * (size_t)k), sim3_load(v.est + 8 * (size_t)v.ei[k]), sim3_load(v.est + 8 * (size_t)v.ej[k]), e);
  const double* W = v.info + 49 * (size_t)k;
#pragma unroll
  for (int r = 0; r < 7; r++) { Oe[r] = dot7(W + 7 * r, e); v.err[7 * (size_t)k + r] = e[r]; }
  v.chi2_each[k] = dot7(e, Oe);
}

// a workgroup per vertex: threads 0-48 the diagonal block, 49-55 b
__global__ __launch_bounds__(64) void pgo_assemble_diag_kernel(PgoView v, double lambda) {
  const int vid = blockIdx.x, t = threadIdx.x;
  const int col = v.vcol[vid];
  if (col < 0 || t >= 56) return;
  double s = 0.0;
  for (int q = v.inc_ptr[vid]; q < v.inc_ptr[vid + 1]; q++) {
    const size_t k = (size_t)v.inc_edge[q];
    const bool is_j = v.inc_side[q] != 0;
    s += t < 49 ? (is_j ? v.Hjj : v.Hii)[49 * k + t] : (is_j ? v.bj : v.bi)[7 * k + t - 49];
  }
  if (t < 49) {
    const int r = t / 7, c = t - 7 * r;
    if (r == c) v.diag[col + r] = s;
    if (r >= c) v.S[(size_t)(col + r) * v.n + col + c] = r == c ? s + lambda : s;
  } else {
    v.b[col + t - 49] = s;
    v.x[col + t - 49] = s;
  }
}

// J_i^T Omega J_j is the block (rows of i, columns of j): into the lower triangle as it is, or transposed
__global__ __launch_bounds__(256) void pgo_assemble_offdiag_kernel(PgoView v) {
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= 49 * (size_t)v.ne) return;
  const int k = (int)(g / 49), t = (int)(g - 49 * (size_t)k), a = t / 7, b = t - 7 * a;
  const int ci = v.vcol[v.ei[k]], cj = v.vcol[v.ej[k]];
  if (ci < 0 || cj < 0) return;
  const double val = v.Hij[g];
  if (ci > cj) v.S[(size_t)(ci + a) * v.n + cj + b] = val;
  else v.S[(size_t)(cj + b) * v.n + ci + a] = val;
}

enum { RED_SUM = 0, RED_SCALE = 1, RED_MAXABS = 2 };
template <int KIND>
__global__ __launch_bounds__(PGO_REDUCE_T) void pgo_reduce_kernel(const double* __restrict__ a, const double* __restrict__ b, double lambda, int n, double* out) {
  __shared__ double red[PGO_REDUCE_T];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < n; i += PGO_REDUCE_T) {
    if (KIND == RED_SUM) s += a[i];
    else if (KIND == RED_SCALE) s += a[i] * (lambda * a[i] + b[i]);       // computeScale (optimization_algorithm_levenberg.cpp:182-189)
    else s = fmax(s, fabs(a[i]));
  }
  red[t] = s;
  __syncthreads();
  for (int w = PGO_REDUCE_T / 2; w > 0; w >>= 1) {
    if (t < w) red[t] = KIND == RED_MAXABS ? fmax(red[t], red[t + w]) : red[t] + red[t + w];
    __syncthreads();
  }
  if (t == 0) *out = red[0];
}

__global__ __launch_bounds__(64) void pgo_update_kernel(PgoView v) {
  const int vid = blockIdx.x * 64 + threadIdx.x;
  if (vid >= v.nv) return;
  const int col = v.vcol[vid];
  if (col < 0) return;
  double u[7];
#pragma unroll
  for (int i = 0; i < 7; i++) u[i] = v.x[col + i];
  sim3_store(sim3_oplus(sim3_load(v.est + 8 * (size_t)vid), u, v.fix_scale[vid] != 0), v.est + 8 * (size_t)vid);
}

// Optimizer::OptimizeEssentialGraph's recovery of an SE(3) pose: [sR t] -> [R t / s] (the rotation as SE3Quat holds it: normalised, w >= 0)
__global__ __launch_bounds__(64) void pgo_se3_kernel(const double* __restrict__ est, int nv, double* __restrict__ T7) {
  const int vid = blockIdx.x * 64 + threadIdx.x;
  if (vid >= nv) return;
  const Sim3 S = sim3_load(est + 8 * (size_t)vid);
  Pose p = sim3_quat(S);
  pose_normalize(p);
  const double f = 1. / S.s;
  for (int i = 0; i < 3; i++) p.t[i] = S.t[i] * f;
  pose_store(p, T7 + 7 * (size_t)vid);
}

// P' = S_opt[ref]^-1 .map( S_init[ref].map(P) )
__global__ __launch_bounds__(256) void pgo_correct_points_kernel(const double* __restrict__ est_init, const double* __restrict__ est, int n, const int* __restrict__ ref,
                                                                 const double* __restrict__ xyz_in, double* __restrict__ xyz_out) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const size_t r = (size_t)ref[p];
  const double X[3] = {xyz_in[3 * (size_t)p], xyz_in[3 * (size_t)p + 1], xyz_in[3 * (size_t)p + 2]};
  double Xc[3], Xw[3];
  sim3_map(sim3_load(est_init + 8 * r), X, Xc);
  sim3_map(sim3_inv(sim3_load(est + 8 * r)), Xc, Xw);
  for (int i = 0; i < 3; i++) xyz_out[3 * (size_t)p + i] = Xw[i];
}

}  // namespace

void pgo_launch_edges(const PgoView& v, hipStream_t st) {
  if (v.ne > 0) hipLaunchKernelGGL(pgo_edge_kernel, dim3((v.ne + PGO_EDGES_PER_BLOCK - 1) / PGO_EDGES_PER_BLOCK), dim3(64), 0, st, v);
}
void pgo_launch_errors(const PgoView& v, hipStream_t st) {
  if (v.ne > 0) hipLaunchKernelGGL(pgo_error_kernel, dim3((v.ne + 63) / 64), dim3(64), 0, st, v);
}
void pgo_launch_chi2(const PgoView& v, hipStream_t st) {
  hipLaunchKernelGGL(pgo_reduce_kernel<RED_SUM>, dim3(1), dim3(PGO_REDUCE_T), 0, st, v.chi2_each, (const double*)nullptr, 0.0, v.ne, v.rec);
}
void pgo_launch_assemble(const PgoView& v, double lambda, hipStream_t st) {
  if (v.n <= 0) return;
  hipLaunchKernelGGL(pgo_assemble_diag_kernel, dim3(v.nv), dim3(64), 0, st, v, lambda);
  hipLaunchKernelGGL(pgo_assemble_offdiag_kernel, dim3((unsigned)((49 * (size_t)v.ne + 255) / 256)), dim3(256), 0, st, v);
  hipLaunchKernelGGL(pgo_reduce_kernel<RED_MAXABS>, dim3(1), dim3(PGO_REDUCE_T), 0, st, v.diag, (const double*)nullptr, 0.0, v.n, v.rec + 2);
}
void pgo_launch_scale(const PgoView& v, double lambda, hipStream_t st) {
  hipLaunchKernelGGL(pgo_reduce_kernel<RED_SCALE>, dim3(1), dim3(PGO_REDUCE_T), 0, st, v.x, v.b, lambda, v.n, v.rec + 1);
}
void pgo_launch_update(const PgoView& v, hipStream_t st) {
  if (v.nv > 0) hipLaunchKernelGGL(pgo_update_kernel, dim3((v.nv + 63) / 64), dim3(64), 0, st, v);
}
void pgo_launch_se3(const double* est, int nv, double* Tcw7, hipStream_t st) {
  if (nv > 0) hipLaunchKernelGGL(pgo_se3_kernel, dim3((nv + 63) / 64), dim3(64), 0, st, est, nv, Tcw7);
}
void pgo_launch_correct_points(const double* est_init, const double* est, int n, const int* ref, const double* xyz_in, double* xyz_out, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(pgo_correct_points_kernel, dim3((n + 255) / 256), dim3(256), 0, st, est_init, est, n, ref, xyz_in, xyz_out);
}

}  // namespace cs
