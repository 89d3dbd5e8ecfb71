// ba_kernels.hip -- HIP kernels of the g2o bundle-adjustment iteration for gfx950 (MI355X).
//
// One LM linearisation = computeActiveErrors + buildSystem + Schur complement + back-substitution
// (object_slam/Thirdparty/g2o/g2o/core/sparse_optimizer.cpp:61-114, block_solver.hpp:353-560):
//   ba_chi2_*            residuals + (robust) chi2, fixed-shape block reduction (deterministic);
//   ba_lin_cam_kernel    one workgroup per camera: residual, analytic 2x6 Jacobian
//                        (types_six_dof_expmap.cpp:148-184), rho'-weighted J^T Omega J and -J^T Omega e
//                        accumulated per lane and reduced with wavefront shuffles -> A_ii (6x6), b_i;
//   ba_lin_pt_kernel     one lane per landmark over its (contiguous) edges: A_jj (3x3), b_j in registers, the
//                        6x3 H_pl block of every edge streamed out once;
//   ba_cub_edge_kernel / ba_odom_edge_kernel   numeric central-difference Jacobians, delta = 1e-9
//                        (base_binary_edge.hpp:130-205) through oplus + computeError, then the quadratic form
//                        (base_binary_edge.hpp:54-120) into per-edge blocks; ba_accum_pose_kernel gathers them;
//   ba_prep_kernel       D_j^-1 = (H_ll,j + lambda I)^-1, D^-1 b_l, W D^-1 per edge (block_solver.hpp:385-407);
//   ba_cam_rhs_kernel / ba_cub_scatter_kernel / ba_offdiag_kernel   reduced system S = H_pp (+lambda) and
//                        b_schur = b_p - sum W D^-1 b_l (:373-439);
//   ba_schur_kernel      one wavefront per covisible camera pair (i1 <= i2): S_{i1 i2} -= sum_j (W D^-1)_{i1 j} W_{i2 j}^T
//                        over the landmarks both cameras see (:409-431);
//   ba_schur_fused_kernel / ba_lin_schur_kernel / ba_schur_long_kernel / ba_schur_gather_kernel   the same product per segment of
//                        landmarks seen by one set of cameras, on the matrix cores (with the landmark side's linearisation fused in);
//   ba_cub_elim_kernel / ba_cub_backsub_kernel   the free cuboids eliminated like landmarks (BaView::elim);
//   ba_backsub_all_kernel   x_l = D^-1 (b_l - W^T x_p) (:457-482), the eliminated cuboids' increments in front of it;
//   ba_update_kernel / ba_scale_update_kernel   oplus on every vertex (sparse_optimizer.cpp:422-435), the LM scale term beside it;
//   ba_classify_kernel, ba_edge_chi_kernel, ba_*_widths_kernel   edge levels and outlier rounds; ba_ext_*   host-evaluated terms;
//   the launchers, with the small kernels of a trial's bookkeeping (ba_trial_prologue_kernel, ba_fail_flag_kernel, ba_sum2_*,
//   ba_multi_zero / ba_multi_copy), at the end.
// What solves the reduced system these kernels build is not here: band_kernels.hip (persistent banded Cholesky, the sharded solve's
// interiors and separators), bcr_kernels.hip (block cyclic reduction), sparse_kernels.hip (general sparse Cholesky); band_solver.h is the
// seam to the first two.
// All FP64.  No atomics on the data path except the (unique-pair) off-diagonal pose blocks.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include <utility>

#include "ba_proj_edge.h"
#include "ba_types.h"
#include "band_solver.h"
#include "cs_wave.h"

namespace cs {

// A projection edge -- its records, its plain chi2, its linearisation and the products of its quadratic form -- is stated in ba_proj_edge.h;
// the kernels below hold what is theirs: which edges a lane takes, where the sums go.  STEREO picks the 3-row form (ROWS) and the table's
// stereo arrays; there is no second wording of anything beside it.

// ---------------------------------------------------------------------------------------------------
// (device bodies with the block index / block count as arguments: ba_chi2_kernel below runs both kinds of block in ONE launch)
template <bool STEREO>
__device__ __forceinline__ void chi2_proj_block(const BaView& v, int bid, int nblocks, double* ws) {
  const ProjTable<STEREO> E(v, PointMajor{});
  double acc = 0;
  for (int k = bid * 256 + threadIdx.x; k < v.n_proj; k += nblocks * 256) {
    if (edge_off(E.width[k])) continue;      // level 1: no share in chi2, its error never formed
    double pc[3], rho0, rho1;
    const double c = proj_edge_chi(E, k, pc);
    proj_rho(E.rk, k, E.width[k], E.kernels_off(E.stereo(k)), c, rho0, rho1);
    acc += rho0;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) v.chi_partial[bid] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}

__device__ __forceinline__ double quad_form(const double* e, const double* info, int n) {
  double s = 0;
  for (int i = 0; i < n; i++) {
    double t = 0;
    for (int j = 0; j < n; j++) t += info[n * i + j] * e[j];
    s += e[i] * t;
  }
  return s;
}

// one lane per cuboid / odometry edge; partial sums appended after the projection partials
__device__ __forceinline__ void chi2_pose_edges_wave(const BaView& v, int partial_off, int bid, int lane) {
  int k = bid * 64 + lane;
  double c = 0;
  if (k < v.n_cub3) {
    double e[9];
    if (v.ce_active[k]) cuboid_edge_error(pose_load(v.cams + 7 * v.ce_cam[k]), cube_load(v.cubes + 10 * v.ce_cub[k]), cube_load(v.ce_meas + 10 * k), e);
    if (v.ce_active[k]) c = quad_form(e, v.ce_info + 81 * k, 9);
    if (v.ce_active[k] && v.ce_rk && v.ce_rk[k] && !(v.rk_off & RK_OFF_CUB3)) { double r1; robust_rho(v.ce_rk[k], v.ce_rdelta[k], c, c, r1); }
  } else if (k < v.n_cub) {
    const int q = k - v.n_cub3;
    double e[4];
    if (v.ce_active[k]) {
      cuboid_proj_error(pose_load(v.cams + 7 * v.ce_cam[k]), cube_load(v.cubes + 10 * v.ce_cub[k]), v.pe_K + 9 * (size_t)q, v.pe_meas + 4 * (size_t)q, e);
      c = quad_form(e, v.pe_info + 16 * (size_t)q, 4);
      if (v.ce_rk && v.ce_rk[k] && !(v.rk_off & RK_OFF_CPROJ)) { double r1; robust_rho(v.ce_rk[k], v.ce_rdelta[k], c, c, r1); }
    }
  } else if (k < v.n_cub + v.n_odom) {
    int q = k - v.n_cub;
    double e[6];
    if (v.oe_active[q]) {
      odom_edge_error(pose_load(v.cams + 7 * v.oe_i[q]), pose_load(v.cams + 7 * v.oe_j[q]), pose_load(v.oe_meas + 7 * q), e);
      c = quad_form(e, v.oe_info + 36 * q, 6);
      if (v.oe_rk && v.oe_rk[q] && !(v.rk_off & RK_OFF_ODOM)) { double r1; robust_rho(v.oe_rk[q], v.oe_rdelta[q], c, c, r1); }
    }
  }
  c = wave_sum(c);
  if (lane == 0) v.chi_partial[partial_off + bid] = c;
}
// chi2 of every active edge in one launch: the blocks of the cuboid / odometry edges FIRST (a wave per 64 edges: few, long -- four SE3 logs
// per cuboid edge), the projection edges' blocks behind them.  The partial sums keep their places: [0, nb_proj) projection blocks, then one
// per 64 pose edges -- the same values in the same slots as the two launches this replaces (round 6: one dispatch less on every trial's chain).
template <bool STEREO>
__global__ __launch_bounds__(256) void ba_chi2_kernel(BaView v, int nb_proj, int nb_pose) {
  __shared__ double ws[4];
  const int nb4 = (nb_pose + 3) / 4;
  if ((int)blockIdx.x < nb4) {
    const int pb = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (pb < nb_pose) chi2_pose_edges_wave(v, nb_proj, pb, threadIdx.x & 63);
    return;
  }
  chi2_proj_block<STEREO>(v, blockIdx.x - nb4, nb_proj, ws);
}

// x^T (lambda x + b) of the LM gain ratio (optimization_algorithm_levenberg.cpp:117-126, computeScale :182-189) over
// the pose increments (x in v.rhs, b in bcam / bcub) and the landmark increments (xl, bl); fixed-shape reduction:
// SCALE_BLOCKS partial sums, added up by the host in order.
enum { SCALE_BLOCKS = 256 };
__device__ __forceinline__ void scale_block(const BaView& v, const double* __restrict__ lamp, double* partial, int bid, double* ws) {
  const double lambda_lm = lamp[0], lambda_pose = lamp[1];     // (lambda of the trial, read from device memory: the launch sequence of a trial is a fixed graph)
  double acc = 0;
  const int n = v.np + v.nc + v.no;
  for (int i = bid * 256 + threadIdx.x; i < n; i += SCALE_BLOCKS * 256) {
    if (i < v.np) {
      if (v.pt_free[i])
#pragma unroll
        for (int d = 0; d < 3; d++) { const double x = v.xl[3 * (size_t)i + d]; acc += x * (lambda_lm * x + v.bl[3 * (size_t)i + d]); }
    } else if (i < v.np + v.nc) {
      const int c = i - v.np, col = v.cam_col[c];
      if (col >= 0)
#pragma unroll
        for (int d = 0; d < 6; d++) { const double x = v.rhs[col + d]; acc += x * (lambda_pose * x + v.bcam[6 * c + d]); }
    } else {
      const int o = i - v.np - v.nc, col = v.cub_col[o];
      if (col >= 0)
#pragma unroll
        for (int d = 0; d < 9; d++) { const double x = v.rhs[col + d]; acc += x * (lambda_pose * x + v.bcub[9 * o + d]); }
    }
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[bid] = (ws[0] + ws[1]) + (ws[2] + ws[3]);
}
__global__ __launch_bounds__(256) void ba_scale_kernel(BaView v, const double* __restrict__ lamp, double* partial) {
  __shared__ double ws[4];
  scale_block(v, lamp, partial, blockIdx.x, ws);
}

// ---------------------------------------------------------------------------------------------------
template <bool STEREO>
__global__ __launch_bounds__(256) void ba_lin_cam_kernel(BaView v) {
  int c = blockIdx.x;
  if (v.cam_col[c] < 0) return;
  __shared__ double red[4][27];
  Pose T = pose_load(v.cams + 7 * c);
  double R[9];
  pose_rotmat(T, R);
  double A[21], b[6];
#pragma unroll
  for (int i = 0; i < 21; i++) A[i] = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) b[i] = 0;
  int e0 = v.cam_ptr[c], e1 = v.cam_ptr[c + 1];
  const ProjTable<STEREO> E(v, CameraMajor{});
  for (int k = e0 + threadIdx.x; k < e1; k += 256) {
    ProjLinT<STEREO ? 3 : 2> L;
    proj_linearize(E, k, T, R, E.point_of(k), L);
    lin_cam_terms(L, A, b);
  }
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 21; i++) { double s = wave_sum(A[i]); if (lane == 0) red[w][i] = s; }
#pragma unroll
  for (int i = 0; i < 6; i++) { double s = wave_sum(b[i]); if (lane == 0) red[w][21 + i] = s; }
  __syncthreads();
  if (threadIdx.x < 27) {
    double s = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    if (threadIdx.x < 21) {
      // upper-triangular index -> (i, j)
      int t = threadIdx.x, i = 0;
      while (t >= 6 - i) { t -= 6 - i; i++; }
      int j = i + t;
      v.Hcam[36 * c + 6 * i + j] = s;
      v.Hcam[36 * c + 6 * j + i] = s;
    } else {
      v.bcam[6 * c + (threadIdx.x - 21)] = s;
    }
  }
}

// Landmark side of the projection edges: A_jj (3x3), b_j and the 6x3 H_pl block of every edge.  One LANE PER EDGE (edges are stored
// landmark-major, so a wavefront reads its 64 edge records -- uv, information, intrinsics, kernel width, camera id -- as coalesced
// streams; a lane per landmark read them 80-byte-strided and fetched every line ~3 times: 415 MB for 150 MB of records by PMC).
// A workgroup owns LIN_PT_GROUP consecutive landmarks = one contiguous run of edges; every edge's J_p^T W J_p / J_p^T r terms go to
// LDS and the landmark's first lane adds them up in edge order -- the order, and therefore every bit, of the sequential loop this
// replaces.  Groups with more than LIN_PT_CAP edges (landmarks with very long tracks) walk their edges per landmark instead.
enum { LIN_PT_GROUP = 48, LIN_PT_CAP = 512 };

template <bool STEREO>
__device__ __forceinline__ void lin_pt_edge(const BaView& v, int k, bool free_pt, double* H6, double* b3) {
  const int c = v.pm_cam[k];
  Pose T = pose_load(v.cams + 7 * c);
  double R[9];
  pose_rotmat(T, R);
  const ProjTable<STEREO> E(v, PointMajor{});
  ProjLinT<STEREO ? 3 : 2> L;
  proj_linearize(E, k, T, R, E.point_of(k), L);
  lin_point_terms(L, H6, b3);
  double* Wk = v.W + 18 * (size_t)k;
  lin_hpl(L, free_pt && v.cam_col[c] >= 0, [&](int i, int j) -> double& { return Wk[3 * i + j]; });
}

template <bool STEREO>
__global__ __launch_bounds__(256) void ba_lin_pt_kernel(BaView v) {
  __shared__ double part[9][LIN_PT_CAP];     // [term][edge of the group]: consecutive lanes, consecutive words
  const int p0 = blockIdx.x * LIN_PT_GROUP, p1 = min(v.np, p0 + LIN_PT_GROUP);
  if (p0 >= v.np) return;
  const int e0 = v.pt_ptr[p0], e1 = v.pt_ptr[p1];
  const bool staged = e1 - e0 <= LIN_PT_CAP;
  if (staged) {
    for (int k = e0 + threadIdx.x; k < e1; k += 256) {
      double H6[6], b3[3];
      lin_pt_edge<STEREO>(v, k, v.pt_free[v.pm_pt[k]] != 0, H6, b3);
#pragma unroll
      for (int i = 0; i < 6; i++) part[i][k - e0] = H6[i];
#pragma unroll
      for (int i = 0; i < 3; i++) part[6 + i][k - e0] = b3[i];
    }
    __syncthreads();
  }
  const int p = p0 + threadIdx.x;
  if (threadIdx.x >= LIN_PT_GROUP || p >= p1) return;
  double H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
  for (int k = v.pt_ptr[p]; k < v.pt_ptr[p + 1]; k++) {
    double H6[6], b3[3];
    if (staged) {
#pragma unroll
      for (int i = 0; i < 6; i++) H6[i] = part[i][k - e0];
#pragma unroll
      for (int i = 0; i < 3; i++) b3[i] = part[6 + i][k - e0];
    } else {
      lin_pt_edge<STEREO>(v, k, v.pt_free[p] != 0, H6, b3);
    }
#pragma unroll
    for (int i = 0; i < 6; i++) H[i] += H6[i];
#pragma unroll
    for (int i = 0; i < 3; i++) b[i] += b3[i];
  }
  double* Hp = v.Hll + 9 * (size_t)p;
  Hp[0] = H[0]; Hp[1] = H[1]; Hp[2] = H[2]; Hp[3] = H[1]; Hp[4] = H[3]; Hp[5] = H[4]; Hp[6] = H[2]; Hp[7] = H[4]; Hp[8] = H[5];
  v.bl[3 * p] = b[0]; v.bl[3 * p + 1] = b[1]; v.bl[3 * p + 2] = b[2];
}

// ---- numeric-Jacobian edges -------------------------------------------------------------------------
// One edge per 16 lanes: lane d evaluates the two perturbed errors of Jacobian column d (lane 15 the unperturbed
// error), the columns meet in LDS, and lane i then forms row i of J^T Omega J and of -J^T Omega e.
// NA / NB = tangent dimensions of the two vertices, D = error dimension; J is stored J[d][r] (column d, row r).
template <int D, int NA, int NB>
// w = rho' of the edge's robust kernel (1 without one: the products below are then exactly the unweighted ones): Omega is weighted
// entry by entry like robustInformation() (base_edge.h:96-102), which also weights b = -J^T (rho' Omega) e (base_binary_edge.hpp:99).
__device__ __forceinline__ void edge_rows_from_columns(const double (*J)[D], const double* e0, const double* __restrict__ info, int i,
                                                       double* Haa, double* Hbb, double* Hab, double* ba, double* bb, double w) {
  constexpr int N = NA + NB;
  if (i >= N) return;
  double t[D];   // t = J(:, i)^T (w Omega)
#pragma unroll
  for (int j = 0; j < D; j++) { double s = 0; for (int k = 0; k < D; k++) s = fma(J[i][k], w * info[D * k + j], s); t[j] = s; }
  double bi = 0;
#pragma unroll
  for (int k = 0; k < D; k++) bi = fma(t[k], e0[k], bi);
  if (i < NA) ba[i] = -bi; else bb[i - NA] = -bi;
  for (int j = 0; j < N; j++) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < D; k++) s = fma(t[k], J[j][k], s);
    if (i < NA) { if (j < NA) Haa[i * NA + j] = s; else Hab[i * NB + (j - NA)] = s; }
    else if (j >= NA) Hbb[(i - NA) * NB + (j - NA)] = s;
  }
}

// 32 lanes per edge: lane (d, s), d = column 0..14 (camera tangent 0-5, cuboid tangent 6-14), s = 0 / 1 evaluates the error at
// +delta / -delta of that column (lane (15, 0): the unperturbed error), so the two oplus + computeError chains of a column run side
// by side instead of one after the other; the pair meets through a lane exchange.
__device__ __forceinline__ double lane_xor16(double x) {
  const int lo = __shfl_xor(__double2loint(x), 16), hi = __shfl_xor(__double2hiint(x), 16);
  return __hiloint2double(hi, lo);
}

// (one instance per edge class -- IS3D: EdgeSE3Cuboid, the edges [0, n_cub3) of the combined list; else EdgeSE3CuboidProj, [n_cub3, n_cub) --
// so that the bounding-box path's eight unrolled corners do not set the register budget of the 9-dim path: 196 -> 168 VGPRs, three
// wavefronts per SIMD instead of two)
__device__ __forceinline__ void odom_edge_block(const BaView& v, int blk, int tid, double (*J)[16][6]);
// odom_blocks (IS3D instance only): that many workgroups IN FRONT of the cuboid edges' do the odometry edges instead, eight per workgroup (round 6,
// last: their ~250 short wavefronts used to be a launch of their own behind this one on the side stream -- 20-38 us that ba_accum_pose_kernel waited
// for; on a stream of their own they queue for wave slots behind this kernel's and the chi2 kernel's workgroups; as this launch's FIRST workgroups
// they are dispatched first and are done long before the cuboid edges)
template <bool IS3D>
__global__ __launch_bounds__(128, 3) void ba_cub_edge_kernel(BaView v, int odom_blocks) {
  __shared__ double Jbuf[2 * 4 * 16 * 6];      // the cuboid edges' [4][16][9] column store, or two odometry column stores of [4][16][6]
  static_assert(2 * 4 * 16 * 6 >= 4 * 16 * 9, "one buffer for both kinds of workgroup");
  if (IS3D && (int)blockIdx.x < odom_blocks) {
    odom_edge_block(v, 2 * blockIdx.x + (threadIdx.x >> 6), threadIdx.x & 63, reinterpret_cast<double (*)[16][6]>(Jbuf + 4 * 16 * 6 * (threadIdx.x >> 6)));
    return;
  }
  double (*J)[16][9] = reinterpret_cast<double (*)[16][9]>(Jbuf);    // [edge in block][column d (15 = e0)][row]
  const int sub = threadIdx.x >> 5, h = threadIdx.x & 31, d = h & 15, sgn = h >> 4;
  const int k = (IS3D ? 0 : v.n_cub3) + ((int)blockIdx.x - (IS3D ? odom_blocks : 0)) * 4 + sub;
  const bool live = k < (IS3D ? v.n_cub3 : v.n_cub);
  const double delta = 1e-9, scalar = 1.0 / (2 * delta);
  const double step = sgn ? -delta : delta;
  constexpr bool is3d = IS3D;
  double (*Jq)[4] = reinterpret_cast<double (*)[4]>(&J[sub][0][0]);   // the 4-row view of this edge's column store
  if (!IS3D && live) {
    const int q = k - v.n_cub3;
    Pose T = pose_load(v.cams + 7 * v.ce_cam[k]);
    Cube cube = cube_load(v.cubes + 10 * v.ce_cub[k]);
    const double* K = v.pe_K + 9 * (size_t)q;
    const double* meas = v.pe_meas + 4 * (size_t)q;
    const bool act = v.ce_active[k] != 0;
    const bool fa = act && v.cam_col[v.ce_cam[k]] >= 0, fb = act && v.cub_col[v.ce_cub[k]] >= 0;
    double e1[4] = {0, 0, 0, 0};
    if (d == 15) {
      if (sgn == 0) cuboid_proj_error(T, cube, K, meas, e1);
    } else if (d < 6) {
      double add[6] = {0, 0, 0, 0, 0, 0};
      add[d] = step;
      if (fa) cuboid_proj_error(cam_oplus(T, add), cube, K, meas, e1);
    } else {
      double add[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      add[d - 6] = step;
      if (fb) cuboid_proj_error(T, cube_oplus(cube, add), K, meas, e1);
    }
    const bool on = d < 6 ? fa : fb;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const double e2 = lane_xor16(e1[r]);      // the partner's error: -delta for the s = 0 lanes
      if (sgn == 0) Jq[d][r] = d == 15 ? (act ? e1[r] : 0.0) : (on ? scalar * (e1[r] - e2) : 0.0);
    }
  }
  if (IS3D && live) {
    Pose T = pose_load(v.cams + 7 * v.ce_cam[k]);
    Cube cube = cube_load(v.cubes + 10 * v.ce_cub[k]);
    Cube meas = cube_load(v.ce_meas + 10 * k);
    const bool act = v.ce_active[k] != 0;  // sharded BA: the edge belongs to another rank -> zero blocks
    const bool fa = act && v.cam_col[v.ce_cam[k]] >= 0, fb = act && v.cub_col[v.ce_cub[k]] >= 0;
    double e1[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    // Two phases.  (1) The unperturbed error: min_log_error's four yaw candidates on four lanes (h = 0 .. 3) instead of a loop on one;
    // the norms meet through lane exchanges, the winner by the reference's rule (first minimum, strict <; g2o_Object.h:76-114).
    // (2) The 30 perturbed evaluations: a 1e-9 step moves a candidate's norm by ~1e-7 at most, so where the winner leads the runner-up
    // by more than CUBE_CLEAR_LEAD (1e-3) (1 + norm) every perturbed evaluation has the same winner and computes THAT candidate only -- the same
    // instructions on the same operands as the loop would run for it, hence the same bits; otherwise (a near tie: yaw near 45 degrees
    // off with a square footprint) the full loop.  Two candidate evaluations per wavefront instead of four: 135 -> ~80 us at C4.
    Cube esti0;
    esti0.pose = pose_mul(pose_inv(T), meas.pose);
    esti0.scale[0] = meas.scale[0]; esti0.scale[1] = meas.scale[1]; esti0.scale[2] = meas.scale[2];
    double ec[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    double nc = 0.0;
    if (h < 4) nc = cube_log_error_candidate(cube, esti0, h, ec);
    const int gbase = threadIdx.x & 32;          // first lane of this edge's 32 within the wavefront
    double n4[4];
#pragma unroll
    for (int i = 0; i < 4; i++) { const int lo = __shfl(__double2loint(nc), gbase + i), hi = __shfl(__double2hiint(nc), gbase + i); n4[i] = __hiloint2double(hi, lo); }
    int win = 0;
    double best_n = n4[0];
#pragma unroll
    for (int i = 1; i < 4; i++) if (n4[i] < best_n) { best_n = n4[i]; win = i; }
    bool clear = best_n == best_n;               // (a NaN leader: the loop decides)
#pragma unroll
    for (int i = 0; i < 4; i++) if (i != win && !(n4[i] - best_n > CUBE_CLEAR_LEAD * (1.0 + best_n))) clear = false;
    // the unperturbed error: the winner's, fetched from the lane that holds it (every lane takes part in the exchange: an inactive
    // source lane would read as zero)
#pragma unroll
    for (int r = 0; r < 9; r++) {
      const int lo = __shfl(__double2loint(ec[r]), gbase + win), hi = __shfl(__double2hiint(ec[r]), gbase + win);
      if (d == 15) e1[r] = __hiloint2double(hi, lo);
    }
    if (d < 6) {
      double add[6] = {0, 0, 0, 0, 0, 0};
      add[d] = step;
      if (fa) {
        const Pose Tp = cam_oplus(T, add);
        if (clear) { Cube es; es.pose = pose_mul(pose_inv(Tp), meas.pose); es.scale[0] = meas.scale[0]; es.scale[1] = meas.scale[1]; es.scale[2] = meas.scale[2]; cube_log_error_candidate(cube, es, win, e1); }
        else cuboid_edge_error(Tp, cube, meas, e1);
      }
    } else if (d < 15) {
      double add[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      add[d - 6] = step;
      if (fb) {
        if (clear) cube_log_error_candidate(cube_oplus(cube, add), esti0, win, e1);
        else cuboid_edge_error(T, cube_oplus(cube, add), meas, e1);
      }
    }
    const bool on = d < 6 ? fa : fb;
#pragma unroll
    for (int r = 0; r < 9; r++) {
      const double e2 = lane_xor16(e1[r]);
      if (sgn == 0) J[sub][d][r] = d == 15 ? (act ? e1[r] : 0.0) : (on ? scalar * (e1[r] - e2) : 0.0);
    }
  }
  __syncthreads();
  double w = 1.0;      // rho' of the edge's kernel at its chi2 (every lane of the edge computes the same value)
  if (live && sgn == 0 && v.ce_rk && v.ce_rk[k] && !(v.rk_off & (is3d ? RK_OFF_CUB3 : RK_OFF_CPROJ))) {
    const double c = is3d ? quad_form(J[sub][15], v.ce_info + 81 * (size_t)k, 9) : quad_form(Jq[15], v.pe_info + 16 * (size_t)(k - v.n_cub3), 4);
    double r0;
    robust_rho(v.ce_rk[k], v.ce_rdelta[k], c, r0, w);
  }
  if (live && is3d && sgn == 0)
    edge_rows_from_columns<9, 6, 9>(J[sub], J[sub][15], v.ce_info + 81 * (size_t)k, d, v.ce_Hcc + 36 * (size_t)k, v.ce_Hoo + 81 * (size_t)k,
                                    v.ce_Hco + 54 * (size_t)k, v.ce_bc + 6 * (size_t)k, v.ce_bo + 9 * (size_t)k, w);
  if (live && !is3d && sgn == 0)
    edge_rows_from_columns<4, 6, 9>(Jq, Jq[15], v.pe_info + 16 * (size_t)(k - v.n_cub3), d, v.ce_Hcc + 36 * (size_t)k, v.ce_Hoo + 81 * (size_t)k,
                                    v.ce_Hco + 54 * (size_t)k, v.ce_bc + 6 * (size_t)k, v.ce_bo + 9 * (size_t)k, w);
}

// (four odometry edges per 64 threads; blk = which four, tid = 0 .. 63, J: the four edges' column store.  Every thread of the workgroup reaches the barrier.)
__device__ __forceinline__ void odom_edge_block(const BaView& v, int blk, int tid, double (*J)[16][6]) {
  const int sub = tid >> 4, d = tid & 15;
  const int k = blk * 4 + sub;
  const bool live = k < v.n_odom;
  const double delta = 1e-9, scalar = 1.0 / (2 * delta);
  if (live) {
    Pose T1 = pose_load(v.cams + 7 * v.oe_i[k]), T2 = pose_load(v.cams + 7 * v.oe_j[k]), M = pose_load(v.oe_meas + 7 * k);
    const bool act = v.oe_active[k] != 0;
    const bool fa = act && v.cam_col[v.oe_i[k]] >= 0, fb = act && v.cam_col[v.oe_j[k]] >= 0;
    double e1[6], e2[6], add[6] = {0, 0, 0, 0, 0, 0};
    if (d == 15) {
      odom_edge_error(T1, T2, M, e1);
      for (int r = 0; r < 6; r++) J[sub][15][r] = act ? e1[r] : 0.0;
    } else if (d < 6) {
      if (fa) {
        add[d] = delta; odom_edge_error(cam_oplus(T1, add), T2, M, e1);
        add[d] = -delta; odom_edge_error(cam_oplus(T1, add), T2, M, e2);
      }
      for (int r = 0; r < 6; r++) J[sub][d][r] = fa ? scalar * (e1[r] - e2[r]) : 0.0;
    } else if (d < 12) {
      if (fb) {
        add[d - 6] = delta; odom_edge_error(T1, cam_oplus(T2, add), M, e1);
        add[d - 6] = -delta; odom_edge_error(T1, cam_oplus(T2, add), M, e2);
      }
      for (int r = 0; r < 6; r++) J[sub][d][r] = fb ? scalar * (e1[r] - e2[r]) : 0.0;
    }
  }
  __syncthreads();
  if (live) {
    double w = 1.0;
    if (v.oe_rk && v.oe_rk[k] && !(v.rk_off & RK_OFF_ODOM)) { double r0; robust_rho(v.oe_rk[k], v.oe_rdelta[k], quad_form(J[sub][15], v.oe_info + 36 * (size_t)k, 6), r0, w); }
    edge_rows_from_columns<6, 6, 6>(J[sub], J[sub][15], v.oe_info + 36 * (size_t)k, d, v.oe_Hii + 36 * (size_t)k, v.oe_Hjj + 36 * (size_t)k,
                                    v.oe_Hij + 36 * (size_t)k, v.oe_bi + 6 * (size_t)k, v.oe_bj + 6 * (size_t)k, w);
  }
}

__global__ __launch_bounds__(64) void ba_odom_edge_kernel(BaView v) {
  __shared__ double J[4][16][6];
  odom_edge_block(v, blockIdx.x, threadIdx.x, J);
}

// gather the numeric-edge blocks into the pose vertices' A_ii / b_i (fixed order: deterministic)
__global__ __launch_bounds__(128) void ba_accum_pose_kernel(BaView v, int zero_cam_first) {
  int vid = blockIdx.x, t = threadIdx.x;
  if (vid < v.nc) {
    int c = vid;
    if (v.cam_col[c] < 0 || t >= 42) return;
    double s = zero_cam_first ? 0.0 : ((t < 36) ? v.Hcam[36 * c + t] : v.bcam[6 * c + t - 36]);
    for (int q = v.cam_ce_ptr[c]; q < v.cam_ce_ptr[c + 1]; q++) { int k = v.cam_ce_idx[q]; s += (t < 36) ? v.ce_Hcc[36 * (size_t)k + t] : v.ce_bc[6 * (size_t)k + t - 36]; }
    for (int q = v.cam_oei_ptr[c]; q < v.cam_oei_ptr[c + 1]; q++) { int k = v.cam_oei_idx[q]; s += (t < 36) ? v.oe_Hii[36 * (size_t)k + t] : v.oe_bi[6 * (size_t)k + t - 36]; }
    for (int q = v.cam_oej_ptr[c]; q < v.cam_oej_ptr[c + 1]; q++) { int k = v.cam_oej_idx[q]; s += (t < 36) ? v.oe_Hjj[36 * (size_t)k + t] : v.oe_bj[6 * (size_t)k + t - 36]; }
    if (t < 36) v.Hcam[36 * c + t] = s; else v.bcam[6 * c + t - 36] = s;
  } else {
    int o = vid - v.nc;
    if (o >= v.no || v.cub_col[o] < 0 || t >= 90) return;
    double s = 0;
    for (int q = v.cub_ce_ptr[o]; q < v.cub_ce_ptr[o + 1]; q++) { int k = v.cub_ce_idx[q]; s += (t < 81) ? v.ce_Hoo[81 * (size_t)k + t] : v.ce_bo[9 * (size_t)k + t - 81]; }
    if (t < 81) v.Hcub[81 * o + t] = s; else v.bcub[9 * o + t - 81] = s;
  }
}

// ---- Schur complement ---------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ba_prep_kernel(BaView v, const double* __restrict__ lamp) {
  const double lambda = lamp[0];
  int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= v.np) return;
  double D[9], Di[9];
  // a landmark without edges on this rank (sharded BA: it lives elsewhere) gets a zero increment
  bool free_pt = v.pt_free[p] != 0 && v.pt_ptr[p + 1] > v.pt_ptr[p];
  if (free_pt) {
#pragma unroll
    for (int i = 0; i < 9; i++) D[i] = v.Hll[9 * (size_t)p + i];
    D[0] += lambda; D[4] += lambda; D[8] += lambda;
    inv3x3(D, Di);
  } else {
#pragma unroll
    for (int i = 0; i < 9; i++) Di[i] = 0;
  }
#pragma unroll
  for (int i = 0; i < 9; i++) v.Dinv[9 * (size_t)p + i] = Di[i];
  double b[3] = {v.bl[3 * p], v.bl[3 * p + 1], v.bl[3 * p + 2]}, db[3];
  mat3_vec(Di, b, db);
  v.dbl[3 * p] = db[0]; v.dbl[3 * p + 1] = db[1]; v.dbl[3 * p + 2] = db[2];
}

// WD = W D^-1, one thread per (projection edge, row of its 6 x 3 block): reads and writes are contiguous across the wave
__global__ __launch_bounds__(256) void ba_wd_kernel(BaView v) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= 6 * (size_t)v.n_proj) return;
  const int k = (int)(t / 6);
  const double* Di = v.Dinv + 9 * (size_t)v.pm_pt[k];
  const double w0 = v.W[3 * t], w1 = v.W[3 * t + 1], w2 = v.W[3 * t + 2];
#pragma unroll
  for (int c = 0; c < 3; c++) v.WD[3 * t + c] = w0 * Di[c] + w1 * Di[3 + c] + w2 * Di[6 + c];
}

// camera part of the reduced system: S_cc = A_cc + lambda I, b_schur,c = b_c - sum_e W_e (D^-1 b_l)
__global__ __launch_bounds__(256) void ba_cam_rhs_kernel(BaView v, const double* __restrict__ lamp) {
  const double lambda = lamp[0];
  int c = blockIdx.x;
  int col = v.cam_col[c];
  if (col < 0) return;
  __shared__ double red[4][6];
  double acc[6] = {0, 0, 0, 0, 0, 0};
  for (int k = v.cam_ptr[c] + threadIdx.x; k < v.cam_ptr[c + 1]; k += 256) {
    int pm = v.cm_pm[k];
    const double* Wk = v.W + 18 * (size_t)pm;
    const double* db = v.dbl + 3 * v.cm_pt[k];
#pragma unroll
    for (int r = 0; r < 6; r++) acc[r] += Wk[3 * r] * db[0] + Wk[3 * r + 1] * db[1] + Wk[3 * r + 2] * db[2];
  }
  int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
  for (int r = 0; r < 6; r++) { double s = wave_sum(acc[r]); if (lane == 0) red[w][r] = s; }
  __syncthreads();
  if (threadIdx.x < 6) {
    double s = (red[0][threadIdx.x] + red[1][threadIdx.x]) + (red[2][threadIdx.x] + red[3][threadIdx.x]);
    v.rhs[col + threadIdx.x] = v.bcam[6 * c + threadIdx.x] - s;
  }
  if (threadIdx.x < 36) {
    int i = threadIdx.x / 6, j = threadIdx.x % 6;
    if (i >= j) *ba_S_at(v, col + i, col + j) = v.Hcam[36 * c + threadIdx.x] + ((i == j && col >= v.lam_lo && col < v.lam_hi) ? lambda : 0.0);
  }
}

__global__ __launch_bounds__(128) void ba_cub_scatter_kernel(BaView v, const double* __restrict__ lamp) {
  const double lambda = lamp[0];
  int o = blockIdx.x, t = threadIdx.x;
  int col = v.cub_col[o];
  if (col < 0) return;
  if (t < 81) {
    int i = t / 9, j = t % 9;
    if (i >= j) *ba_S_at(v, col + i, col + j) = v.Hcub[81 * o + t] + ((i == j && col >= v.lam_lo && col < v.lam_hi) ? lambda : 0.0);
  } else if (t < 90) {
    v.rhs[col + t - 81] = v.bcub[9 * o + t - 81];
  }
}

// off-diagonal pose blocks: camera-cuboid (6x9) per cuboid edge, camera-camera (6x6) per odometry edge
__device__ __forceinline__ void ba_offdiag_body(const BaView& v, int k, int t) {
  if (k < v.n_cub) {
    if (v.elim) return;       // the cuboids are not part of the reduced system
    int ca = v.cam_col[v.ce_cam[k]], cb = v.cub_col[v.ce_cub[k]];
    if (ca < 0 || cb < 0 || t >= 54) return;
    int i = t / 9, j = t % 9;
    double val = v.ce_Hco[54 * (size_t)k + t];
    // block (ca+i, cb+j): stored in the lower triangle, whichever vertex comes later in the ordering
    if (cb > ca) atomicAdd(ba_S_at(v, cb + j, ca + i), val); else atomicAdd(ba_S_at(v, ca + i, cb + j), val);
  } else {
    int q = k - v.n_cub;
    if (q >= v.n_odom) return;
    int ca = v.cam_col[v.oe_i[q]], cb = v.cam_col[v.oe_j[q]];
    if (ca < 0 || cb < 0 || t >= 36) return;
    int i = t / 6, j = t % 6;
    double val = v.oe_Hij[36 * (size_t)q + t];
    if (cb > ca) atomicAdd(ba_S_at(v, cb + j, ca + i), val); else atomicAdd(ba_S_at(v, ca + i, cb + j), val);
  }
}
__global__ __launch_bounds__(64) void ba_offdiag_kernel(BaView v) { ba_offdiag_body(v, blockIdx.x, threadIdx.x); }

// One wavefront per covisible camera pair.  Every lane walks its own landmarks of the pair (entries q0 + lane,
// + 64, ...), accumulating the whole 6 x 6 block W_a D^-1 W_b^T in registers (each lane streams two contiguous
// 144-byte records per entry); the 64 partial blocks are summed through an LDS tile in a fixed order.
__global__ __launch_bounds__(128) void ba_schur_kernel(BaView v) {
  __shared__ double red[2][64][37];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int pair = blockIdx.x * 2 + wv;
  if (pair < v.n_pairs) {
    const int q0 = v.pair_ptr[pair], q1 = v.pair_ptr[pair + 1];
    double acc[36];
#pragma unroll
    for (int o = 0; o < 36; o++) acc[o] = 0.0;
    for (int q = q0 + lane; q < q1; q += 64) {
      const double* x = v.WD + 18 * (size_t)v.ent_a[q];
      const double* y = v.W + 18 * (size_t)v.ent_b[q];
      double xv[18], yv[18];
#pragma unroll
      for (int i = 0; i < 18; i++) { xv[i] = x[i]; yv[i] = y[i]; }
#pragma unroll
      for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c < 6; c++) acc[6 * r + c] = fma(xv[3 * r + 2], yv[3 * c + 2], fma(xv[3 * r + 1], yv[3 * c + 1], fma(xv[3 * r], yv[3 * c], acc[6 * r + c])));
    }
#pragma unroll
    for (int o = 0; o < 36; o++) red[wv][lane][o] = acc[o];
  }
  __syncthreads();
  if (pair < v.n_pairs && lane < 36) {
    double s = 0;
#pragma unroll 8
    for (int j = 0; j < 64; j++) s += red[wv][j][lane];
    const int r = lane / 6, c = lane % 6;
    const int i1 = v.pair_i1[pair], i2 = v.pair_i2[pair];
    // element (i1 + r, i2 + c) of the symmetric S, i1 <= i2: its lower-triangle home is (i2 + c, i1 + r)
    if (i1 != i2 || c >= r) *ba_S_at(v, i2 + c, i1 + r) -= s;
  }
}

// ---- fused Schur product on the matrix cores ----------------------------------------------------------------------------
// block_solver.hpp:385-431 for one segment of landmarks that are seen by the same k cameras.  Their Hpl blocks form, per
// landmark j, a (6k x 3) matrix W_j (rows: camera slot a, row r of its 6 x 3 block; contiguous in the point-major W array), and
//     sum_j W_j D_j^-1 W_j^T   (6k x 6k)       sum_j W_j D_j^-1 b_l,j   (6k)
// is ONE matrix product whose contraction index runs over (landmark, landmark coordinate): A = [W_j D_j^-1]_j (6k x 3m),
// B = [W_j | b_l,j]_j^T (3m x (6k + 1)).  v_mfma_f64_16x16x4_f64 takes the K = 3 coordinates of one landmark (padded to 4) per
// issue; a wavefront walks its segment, keeping the upper block triangle of the product in accumulator registers
// (MT x MT tiles of 16 x 16), i.e. the cross-landmark reduction happens inside the matrix core, not through LDS or atomics.
// Operand lane map of the f64 16x16x4 form: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15],
// D[row = (lane >> 4) + 4 reg][col = lane & 15].
// Every W record is read from HBM exactly once (the pair-major kernel re-read it once per camera pair), D^-1 is written once for
// the back-substitution, and W D^-1 never exists in memory.  (ba_v4d, the accumulator type: cs_wave.h)

template <int MT>
struct BaSegOperands {
  double Dm[9];        // H_ll of the landmark (lambda not yet added)
  double w[MT][3];     // W row 16 t + i
  double bcol[MT];     // B operand of N-tile u
  int p;
};

// all loads unconditional (clamped addresses, values selected afterwards): no exec-masked branches, so the compiler can count
// the loads in flight and the prefetch of the next landmark really overlaps this one's products
template <int MT>
__device__ __forceinline__ void ba_seg_load(const BaView& v, int p, int e0, int rows, int i, int kk, BaSegOperands<MT>& o) {
  o.p = p;
  const double* H = v.Hll + 9 * (size_t)p;
#pragma unroll
  for (int q = 0; q < 9; q++) o.Dm[q] = H[q];
  const double* Wp = v.W + 18 * (size_t)e0;
  const int k3 = kk < 3 ? kk : 0;
  const double blv = v.bl[3 * (size_t)p + k3];
#pragma unroll
  for (int t = 0; t < MT; t++) {
    const int row = 16 * t + i;
    const bool in = row < rows;
    const double* wr = Wp + 3 * (in ? row : rows - 1);
    const double w0 = wr[0], w1 = wr[1], w2 = wr[2];
    o.w[t][0] = in ? w0 : 0.0; o.w[t][1] = in ? w1 : 0.0; o.w[t][2] = in ? w2 : 0.0;
    // B: column `row` of [W_j^T | b_l]: W(row, kk) below `rows`, the right-hand-side column at `rows`
    const double wk = k3 == 0 ? w0 : (k3 == 1 ? w1 : w2);
    o.bcol[t] = kk < 3 ? (in ? wk : (row == rows ? blv : 0.0)) : 0.0;
  }
}

template <int MT>
__device__ __forceinline__ void ba_schur_segment(const BaView& v, double lambda, int seg, int k) {
  const int lane = threadIdx.x & 63, i = lane & 15, kk = lane >> 4, rows = 6 * k;
  const int q0 = v.seg_ptr[seg], q1 = v.seg_ptr[seg + 1];
  // the segment's landmark ids and first-edge slots, one per lane, broadcast with readlane inside the loop (no dependent
  // scalar loads on the chain)
  int my_p = 0, my_e0 = 0;
  if (q0 + lane < q1) { my_p = v.run_lm[q0 + lane]; my_e0 = v.pt_ptr[my_p]; }
  ba_v4d acc[MT][MT];
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int u = 0; u < MT; u++) acc[t][u] = ba_v4d{0.0, 0.0, 0.0, 0.0};
  // ping-pong operand buffers: while landmark q is multiplied, the loads of landmark q + 1 are in flight
  BaSegOperands<MT> bufA, bufB;
  const int n = q1 - q0;
  auto load = [&](BaSegOperands<MT>& o, int q) {
    const int qq = q < n ? q : n - 1;            // past the end: re-load the last landmark (harmless, keeps the loop branch-free)
    ba_seg_load<MT>(v, __builtin_amdgcn_readlane(my_p, qq), __builtin_amdgcn_readlane(my_e0, qq), rows, i, kk, o);
  };
  auto product = [&](const BaSegOperands<MT>& o) {
    double D[9], Di[9];
#pragma unroll
    for (int e = 0; e < 9; e++) D[e] = o.Dm[e];
    D[0] += lambda; D[4] += lambda; D[8] += lambda;
    inv3x3(D, Di);
    if (lane < 9) v.Dinv[9 * (size_t)o.p + lane] = Di[lane];       // for the back-substitution (block_solver.hpp:457-482)
    const int k3 = kk < 3 ? kk : 0;
    double a[MT];
#pragma unroll
    for (int t = 0; t < MT; t++) {
      const double wd = o.w[t][0] * Di[k3] + o.w[t][1] * Di[3 + k3] + o.w[t][2] * Di[6 + k3];   // (W D^-1)(row, kk), as ba_wd_kernel
      a[t] = kk < 3 ? wd : 0.0;
    }
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
      for (int u = t; u < MT; u++) acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], o.bcol[u], acc[t][u], 0, 0, 0);
  };
  load(bufA, 0);
  for (int q = 0; q < n; q += 2) {
    load(bufB, q + 1);
    product(bufA);
    if (q + 1 < n) {            // wave-uniform
      load(bufA, q + 2);
      product(bufB);
    }
  }
  // flush: the k (k + 1) / 2 blocks (a <= b; diagonal blocks: upper triangle c >= r, what the reduced system stores) and
  // the k coefficient vectors
  const int tile0 = v.seg_tile[seg], slot0 = v.seg_slot[seg];
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int u = t; u < MT; u++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const int R = 16 * t + (lane >> 4) + 4 * g, Cc = 16 * u + (lane & 15);
        if (R >= rows) continue;
        const int sa = R / 6, r = R - 6 * sa;
        const double val = acc[t][u][g];
        if (Cc < rows) {
          const int sb = Cc / 6, c = Cc - 6 * sb;
          if (sa < sb || (sa == sb && c >= r)) v.part_tiles[36 * (size_t)(tile0 + sa * k - sa * (sa - 1) / 2 + (sb - sa)) + 6 * r + c] = val;
        } else if (Cc == rows) {
          v.part_coef[6 * (size_t)(slot0 + sa) + r] = val;
        }
      }
}

// one instantiation per tile count (the segments are sorted by k, so each launch covers a contiguous range): MT = 1 for k <= 2
// (12 rows + the right-hand-side column), 2 for k <= 5 (30 + 1), 3 for k <= 7 (42 + 1), 4 for k <= 10 (60 + 1), 5 for k <= BA_FUSED_KMAX = 13 (78 + 1)
template <int MT>
__global__ __launch_bounds__(256) void ba_schur_fused_kernel(BaView v, const double* __restrict__ lamp, int seg_begin, int seg_end) {
  const double lambda = lamp[0];
  const int seg = __builtin_amdgcn_readfirstlane(seg_begin + blockIdx.x * 4 + (threadIdx.x >> 6));   // wave-uniform: scalar loads below
  if (seg >= seg_end) return;
  ba_schur_segment<MT>(v, lambda, seg, v.seg_k[seg]);
}

// ---- linearisation + Schur product in one pass over the projection edges (round 5) ------------------------------------------------
// ba_lin_pt_kernel wrote every edge's H_pl block (163 MB at C4) for ba_schur_fused_kernel to read back two kernels later, and spent
// 70-140 us of the linearisation phase doing so.  Here the segment's wavefront linearises its own edges -- a lane per edge, a chunk of
// floor(64 / k) landmarks at a time (types_six_dof_expmap.cpp:148-184, base_binary_edge.hpp:54-120: the same proj_linearize and the
// same products as ba_lin_pt_kernel, hence the same bits) -- keeps the blocks in LDS as the matrix-core operands, sums H_ll / b_l per
// landmark in edge order, inverts the damped block once per landmark (not once per lane) and runs ba_schur_segment's products.  H_pl,
// H_ll, b_l and D^-1 are still written, once, for the back-substitution (block_solver.hpp:457-482); nothing is read back.  A lane's
// camera is its slot's -- the same for every landmark of the segment -- so its pose and rotation matrix are loaded and formed once.
// Used by cs_ba_optimize from the second iteration on (the first needs H_ll for lambda's initial value before any trial), on unsharded
// graphs without long tracks or host-evaluated edges; the classic pair of kernels serves everything else and the inspection entries.
enum { LS_PLANES = 18, LS_DCOLS = 16, LS_WAVE_DOUBLES = LS_PLANES * 64 + 12 * LS_DCOLS };   // 10.75 KB per wavefront: three workgroups per CU
template <int MT, bool STEREO>
__device__ __forceinline__ void ba_lin_schur_segment(const BaView& v, double lambda, int seg, int k, double* lds) {
  const int lane = threadIdx.x & 63, i = lane & 15, kk = lane >> 4, rows = 6 * k;
  const int q0 = v.seg_ptr[seg], q1 = v.seg_ptr[seg + 1], n = q1 - q0;
  double (*Wl)[64] = reinterpret_cast<double (*)[64]>(lds);                  // [18][edge of the chunk]
  double (*Dl)[LS_DCOLS] = reinterpret_cast<double (*)[LS_DCOLS]>(lds + LS_PLANES * 64);   // [12][landmark of the chunk]: D^-1 (9), b_l (3)
  // (round 6: the run entry's first edge and the slot's camera come from tables of their own -- run_e0 = pt_ptr[run_lm], seg_cam = pm_cam of the
  // segment's first landmark -- so that the head of a segment is three dependent round trips (segment scalars -> these -> pose / records)
  // instead of five; with three waves per SIMD the kernel is those round trips)
  int my_p = 0, my_e0 = 0;
  if (q0 + lane < q1) { my_p = v.run_lm[q0 + lane]; my_e0 = v.run_e0[q0 + lane]; }
  ba_v4d acc[MT][MT];
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int u = 0; u < MT; u++) acc[t][u] = ba_v4d{0.0, 0.0, 0.0, 0.0};
  const int C = min((int)LS_DCOLS, 64 / k);             // landmarks per chunk
  const int lc = lane / k, sa_l = lane - lc * k;        // this lane's (landmark of the chunk, camera slot)
  // the slot's camera (the same for every landmark of the segment)
  const int cam = v.seg_cam[v.seg_slot[seg] + (lc < C ? sa_l : 0)];
  const Pose T = pose_load(v.cams + 7 * cam);
  double R[9];
  pose_rotmat(T, R);
  const bool cam_free = v.cam_col[cam] >= 0;
  // operand rows of this lane, per 16-row tile: row = 16 t + i = 6 a + r
  int w_off[MT]; bool w_in[MT];
#pragma unroll
  for (int t = 0; t < MT; t++) {
    const int row = 16 * t + i;
    w_in[t] = row < rows;
    const int rr = w_in[t] ? row : 0, a = rr / 6, r = rr - 6 * a;
    w_off[t] = (3 * r) * 64 + a;                        // plane 3 r (+ c), edge a (+ l k)
  }
  const int k3 = kk < 3 ? kk : 0;
  // an edge's record (point, measurement, information, intrinsics, kernel width): requested one chunk ahead, with clamped
  // indices -- every load unconditional, so that the requests of the next chunk are in flight under this chunk's products
  // (a stereo graph's record adds the edge's kind and u_right; the 3 x 3 information and bf are read where a stereo lane linearises -- ten more
  // doubles in the record would be held across the chunk's products by every lane, mono ones included)
  struct EdgeRec { double X[3], uv[2], info[4], intr[4], huber; int p, e; double ur; int kind; };
  const ProjTable<STEREO> E(v, PointMajor{});
  auto fetch = [&](int c0) {
    EdgeRec r;
    const int ncl = min(C, n - c0);
    const int src = (c0 < n && lc < ncl) ? c0 + lc : 0;
    r.p = __shfl(my_p, src); r.e = __shfl(my_e0, src) + ((c0 < n && lc < ncl) ? sa_l : 0);
#pragma unroll
    for (int q = 0; q < 3; q++) r.X[q] = v.points[3 * (size_t)r.p + q];
#pragma unroll
    for (int q = 0; q < 2; q++) r.uv[q] = v.pm_uv[2 * (size_t)r.e + q];
#pragma unroll
    for (int q = 0; q < 4; q++) { r.info[q] = E.info_at(r.e, q); r.intr[q] = E.intr_at(r.e, q); }
    r.huber = v.pm_huber[r.e];
    r.ur = E.ur(r.e); r.kind = E.kind_of(r.e);
    return r;
  };
  EdgeRec rec = fetch(0);
  for (int c0 = 0; c0 < n; c0 += C) {
    const int ncl = min(C, n - c0);
    // ---- the chunk's edges, a lane each
    double h9[9];          // this edge's J_p^T W J_p (upper triangle, 6) and J_p^T r (3)
    const int p_edge = rec.p;
    {
      const int p = rec.p, e = rec.e;
#pragma unroll
      for (int q = 0; q < 9; q++) h9[q] = 0.0;
      if (lc < ncl) {
        ProjLinT<STEREO ? 3 : 2> L;
        proj_linearize(T, R, rec.X, rec.uv, rec.info, rec.intr, rec.huber, E.rk, e, E.rk_off, rec.kind != 0, rec.ur, E.srec(e), L);
        // (H_pl goes out as 18 eight-byte stores per lane.  Round 5 measured the alternative -- the chunk's records through LDS as runs of 18 k
        // contiguous doubles, 64 consecutive doubles per store instruction --: the same HBM traffic by the counters (251 MB read, 227 MB written per
        // launch at C4: L2 merges the partial lines either way) and a kernel 7 % slower for the index arithmetic; dropped.  What the kernel
        // over-fetches is its INPUT: a landmark's k edge records are 80 / 160 bytes in a stream ordered by landmark id, and the landmarks of a
        // segment are not neighbours in it.)
        // Round 6: H_pl does not go to memory at all here (231 MB written per launch at C4, 259 MB read back by the back-substitution): the only
        // reader behind this kernel, x_l = D^-1 (b_l - H_pl^T x_p), forms the blocks again from the same state with the same arithmetic
        // (backsub_lin_point) -- 20 bytes of edge record instead of a 144-byte block per edge, the same bits.
        const bool both = cam_free && v.pt_free[p] != 0;
#pragma unroll
        for (int q = 0; q < 6; q++) {
          double h3[3];
          lin_hpl_row(L, q, h3);
#pragma unroll
          for (int j = 0; j < 3; j++) {
            const double w = both ? h3[j] : 0.0;
            Wl[3 * q + j][lane] = w;
          }
        }
        // (behind the H_pl rows, not in front of them: in front, the 2-row form's <5> instance needs 137 registers beside its 120 accumulator
        // registers -- one more than two wavefronts per SIMD allow; here 131)
        lin_point_terms(L, h9, h9 + 6);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    // ---- per landmark: H_ll, b_l summed in edge order (the landmark's first lane collects its k edges' terms through lane exchanges:
    // 0 + h_0 + h_1 + ..., the order and the bits of ba_lin_pt_kernel's loop); the damped block's inverse
    {
      double H[6], b[3];
#pragma unroll
      for (int q = 0; q < 6; q++) H[q] = h9[q];
#pragma unroll
      for (int q = 0; q < 3; q++) b[q] = h9[6 + q];
      for (int a = 1; a < k; a++) {
        const int from = (lane + a) & 63;
#pragma unroll
        for (int q = 0; q < 9; q++) {
          const int lo = __shfl(__double2loint(h9[q]), from), hi = __shfl(__double2hiint(h9[q]), from);
          const double t = __hiloint2double(hi, lo);
          if (q < 6) H[q] += t; else b[q - 6] += t;
        }
      }
      if (sa_l == 0 && lc < ncl) {
        double* Hp = v.Hll + 9 * (size_t)p_edge;
        Hp[0] = H[0]; Hp[1] = H[1]; Hp[2] = H[2]; Hp[3] = H[1]; Hp[4] = H[3]; Hp[5] = H[4]; Hp[6] = H[2]; Hp[7] = H[4]; Hp[8] = H[5];
        v.bl[3 * (size_t)p_edge] = b[0]; v.bl[3 * (size_t)p_edge + 1] = b[1]; v.bl[3 * (size_t)p_edge + 2] = b[2];
        double D[9] = {H[0], H[1], H[2], H[1], H[3], H[4], H[2], H[4], H[5]}, Di[9];
        D[0] += lambda; D[4] += lambda; D[8] += lambda;
        inv3x3(D, Di);
#pragma unroll
        for (int q = 0; q < 9; q++) { v.Dinv[9 * (size_t)p_edge + q] = Di[q]; Dl[q][lc] = Di[q]; }
#pragma unroll
        for (int q = 0; q < 3; q++) Dl[9 + q][lc] = b[q];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    rec = fetch(c0 + C);
    // ---- the products, landmark by landmark (ba_schur_segment's, operands out of LDS)
    for (int l = 0; l < ncl; l++) {
      double Di[9];
#pragma unroll
      for (int q = 0; q < 9; q++) Di[q] = Dl[q][l];
      const double blv = Dl[9 + k3][l];
      double a[MT], bcol[MT];
#pragma unroll
      for (int t = 0; t < MT; t++) {
        const double* wp = lds + w_off[t] + l * k;
        const double x0 = wp[0], x1 = wp[64], x2 = wp[128];
        const double w0 = w_in[t] ? x0 : 0.0, w1 = w_in[t] ? x1 : 0.0, w2 = w_in[t] ? x2 : 0.0;
        const double wd = w0 * Di[k3] + w1 * Di[3 + k3] + w2 * Di[6 + k3];
        a[t] = kk < 3 ? wd : 0.0;
        const double wk = k3 == 0 ? w0 : (k3 == 1 ? w1 : w2);
        bcol[t] = kk < 3 ? (w_in[t] ? wk : (16 * t + i == rows ? blv : 0.0)) : 0.0;
      }
#pragma unroll
      for (int t = 0; t < MT; t++)
#pragma unroll
        for (int u = t; u < MT; u++) acc[t][u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[t], bcol[u], acc[t][u], 0, 0, 0);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
  }
  // flush: as ba_schur_segment
  const int tile0 = v.seg_tile[seg], slot0 = v.seg_slot[seg];
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int u = t; u < MT; u++)
#pragma unroll
      for (int g = 0; g < 4; g++) {
        const int Rr = 16 * t + (lane >> 4) + 4 * g, Cc = 16 * u + (lane & 15);
        if (Rr >= rows) continue;
        const int sa = Rr / 6, r = Rr - 6 * sa;
        const double val = acc[t][u][g];
        if (Cc < rows) {
          const int sb = Cc / 6, c = Cc - 6 * sb;
          if (sa < sb || (sa == sb && c >= r)) v.part_tiles[36 * (size_t)(tile0 + sa * k - sa * (sa - 1) / 2 + (sb - sa)) + 6 * r + c] = val;
        } else if (Cc == rows) {
          v.part_coef[6 * (size_t)(slot0 + sa) + r] = val;
        }
      }
}
template <int MT, bool STEREO>
__global__ __launch_bounds__(256) void ba_lin_schur_kernel(BaView v, const double* __restrict__ lamp, int seg_begin, int seg_end, double lam_val) {
  __shared__ double lds[4][LS_WAVE_DOUBLES];
  const double lambda = lamp ? lamp[0] : lam_val;      // (by value: the trial's prologue runs beside this kernel, BaSidePrologue)
  const int seg = __builtin_amdgcn_readfirstlane(seg_begin + blockIdx.x * 4 + (threadIdx.x >> 6));
  if (seg >= seg_end) return;
  ba_lin_schur_segment<MT, STEREO>(v, lambda, seg, v.seg_k[seg], lds[threadIdx.x >> 6]);
}

// Long tracks (BA_FUSED_KMAX < k <= BA_LONG_KMAX cameras: the tail of a real map, landmarks seen from dozens of key frames): the same
// segment, the same partial blocks and vectors for the destination schedule, formed with plain multiply-adds -- a wavefront per
// segment, its landmarks one after the other (such landmarks rarely share their camera set: usually one), W and W D^-1 of the landmark
// in LDS, the k (k + 1) / 2 blocks spread over the lanes.  Without it ONE such landmark sent the whole problem to the pair-major path.
__global__ __launch_bounds__(256) void ba_schur_long_kernel(BaView v, const double* __restrict__ lamp, int seg_begin, int seg_end) {
  __shared__ double Wl[4][6 * BA_LONG_KMAX * 3], WDl[4][6 * BA_LONG_KMAX * 3];
  const double lambda = lamp[0];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int seg = __builtin_amdgcn_readfirstlane(seg_begin + blockIdx.x * 4 + wv);
  if (seg >= seg_end) return;
  const int k = v.seg_k[seg], rows = 6 * k, q0 = v.seg_ptr[seg], q1 = v.seg_ptr[seg + 1], tile0 = v.seg_tile[seg], slot0 = v.seg_slot[seg];
  const int npair = k * (k + 1) / 2;
  double* W = Wl[wv];
  double* WD = WDl[wv];
  for (int q = q0; q < q1; q++) {
    const int p = v.run_lm[q], e0 = v.pt_ptr[p];
    double D[9], Di[9];
#pragma unroll
    for (int e = 0; e < 9; e++) D[e] = v.Hll[9 * (size_t)p + e];
    D[0] += lambda; D[4] += lambda; D[8] += lambda;
    inv3x3(D, Di);
    if (lane < 9) v.Dinv[9 * (size_t)p + lane] = Di[lane];
    const double bl0 = v.bl[3 * (size_t)p], bl1 = v.bl[3 * (size_t)p + 1], bl2 = v.bl[3 * (size_t)p + 2];
    const double* Wp = v.W + 18 * (size_t)e0;            // the landmark's k edges, camera slots ascending: row 6 a + r at Wp + 3 (6 a + r)
    __builtin_amdgcn_wave_barrier();
    for (int row = lane; row < rows; row += 64) {
      const double w0 = Wp[3 * row], w1 = Wp[3 * row + 1], w2 = Wp[3 * row + 2];
      W[3 * row] = w0; W[3 * row + 1] = w1; W[3 * row + 2] = w2;
#pragma unroll
      for (int m = 0; m < 3; m++) WD[3 * row + m] = w0 * Di[m] + w1 * Di[3 + m] + w2 * Di[6 + m];       // (W D^-1)(row, m), as ba_wd_kernel
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const bool first = q == q0;
    // an item = one row of one block: (pair of slots, r) -> the six entries (r, 0 .. 5), 48 contiguous bytes of the tile
    for (int item = lane; item < 6 * npair; item += 64) {
      const int pi = item / 6, r = item - 6 * pi;
      // pair index -> (sa, sb), sa <= sb: pi = sa k - sa (sa - 1) / 2 + (sb - sa)
      const float tk = (float)(2 * k + 1);
      int sa = (int)((tk - __builtin_sqrtf(tk * tk - 8.0f * (float)pi)) * 0.5f);
      sa = max(0, min(k - 1, sa));
      while (sa > 0 && sa * k - sa * (sa - 1) / 2 > pi) sa--;
      while ((sa + 1) * k - (sa + 1) * sa / 2 <= pi) sa++;
      const int sb = sa + (pi - (sa * k - sa * (sa - 1) / 2));
      const double* x = WD + 3 * (6 * sa + r);
      const double x0 = x[0], x1 = x[1], x2 = x[2];
      const double* y = W + 18 * sb;
      double* dst = v.part_tiles + 36 * (size_t)(tile0 + pi) + 6 * r;
      double val[6];
#pragma unroll
      for (int c = 0; c < 6; c++) val[c] = fma(x2, y[3 * c + 2], fma(x1, y[3 * c + 1], x0 * y[3 * c]));
      const int c_lo = sa == sb ? r : 0;                 // (diagonal blocks: the upper triangle is what the reduced system stores)
      if (first) {                                       // (wave-uniform: the segment's first landmark stores, the others add -- no load before a plain store)
#pragma unroll
        for (int c = 0; c < 6; c++) if (c >= c_lo) dst[c] = val[c];
      } else {
#pragma unroll
        for (int c = 0; c < 6; c++) if (c >= c_lo) dst[c] += val[c];
      }
    }
    for (int row = lane; row < rows; row += 64) {
      const double val = fma(WD[3 * row + 2], bl2, fma(WD[3 * row + 1], bl1, WD[3 * row] * bl0));
      double* dst = v.part_coef + 6 * (size_t)slot0 + row;
      if (first) *dst = val; else *dst += val;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  }
}

// destination schedule, blocks: one wavefront per block of the reduced system sums the partial blocks written for it, in the
// order of the segments (fixed: the result does not depend on scheduling), and subtracts the sum (block_solver.hpp:409-431)
__global__ __launch_bounds__(256) void ba_schur_gather_kernel(BaView v) {
  const int pair = __builtin_amdgcn_readfirstlane(blockIdx.x * 4 + (threadIdx.x >> 6)), lane = threadIdx.x & 63;
  if (pair >= v.n_gpairs) return;
  // (round 5: the partial blocks' indices are fetched 64 at a time, one per lane, and the blocks eight at a time -- all requests of a
  // batch in flight together; the additions stay in the schedule's order.  One index load + one block load per term, each waiting for
  // the one before, made this kernel 55 us of pure latency at C4.)
  const int q0 = v.gpair_ptr[pair], nq = v.gpair_ptr[pair + 1] - q0;
  const int l36 = lane < 36 ? lane : 0;
  double s = 0;
  for (int base = 0; base < nq; base += 64) {
    const int cnt = min(64, nq - base);
    const int my_t = v.gtile[q0 + base + (lane < cnt ? lane : 0)];
    for (int j = 0; j < cnt; j += 8) {
      double x[8];
#pragma unroll
      for (int u = 0; u < 8; u++) {
        const int tq = __builtin_amdgcn_readlane(my_t, min(j + u, cnt - 1));
        x[u] = v.part_tiles[36 * (size_t)tq + l36];
      }
#pragma unroll
      for (int u = 0; u < 8; u++) if (j + u < cnt) s += x[u];
    }
  }
  if (lane >= 36) return;
  const int r = lane / 6, c = lane % 6;
  const int i1 = v.gpair_i1[pair], i2 = v.gpair_i2[pair];
  if (i1 != i2 || c >= r) *ba_S_at(v, i2 + c, i1 + r) -= s;
}

// destination schedule, right-hand side: S_cc = A_cc + lambda I and b_schur,c = b_c - sum of the camera's partial W D^-1 b_l
__device__ __forceinline__ void ba_cam_rhs_fused_body(const BaView& v, const double* __restrict__ lamp, int c, int t) {
  const double lambda = lamp[0];
  const int col = v.cam_col[c];
  if (col < 0) return;
  {
    const int q0 = v.gcam_ptr[c], nq = v.gcam_ptr[c + 1] - q0;
    const int t6 = t < 6 ? t : 0;
    double s = 0;
    for (int base = 0; base < nq; base += 64) {       // (as ba_schur_gather_kernel: indices 64 at a time, vectors eight at a time, sums in order)
      const int cnt = min(64, nq - base);
      const int my_s = v.gslot[q0 + base + (t < cnt ? t : 0)];
      for (int j = 0; j < cnt; j += 8) {
        double x[8];
#pragma unroll
        for (int u = 0; u < 8; u++) x[u] = v.part_coef[6 * (size_t)__builtin_amdgcn_readlane(my_s, min(j + u, cnt - 1)) + t6];
#pragma unroll
        for (int u = 0; u < 8; u++) if (j + u < cnt) s += x[u];
      }
    }
    if (t < 6) v.rhs[col + t] = v.bcam[6 * c + t] - s;
  }
  if (t < 36) {
    const int i = t / 6, j = t % 6;
    if (i >= j) *ba_S_at(v, col + i, col + j) = v.Hcam[36 * c + t] + ((i == j && col >= v.lam_lo && col < v.lam_hi) ? lambda : 0.0);
  }
}
__global__ __launch_bounds__(64) void ba_cam_rhs_fused_kernel(BaView v, const double* __restrict__ lamp) { ba_cam_rhs_fused_body(v, lamp, blockIdx.x, threadIdx.x); }
// ... and the off-diagonal pose blocks in the same launch (round 6: the cameras' diagonal blocks / right-hand sides and the pose edges' off-diagonal
// blocks touch disjoint entries of S; two 5-7 us launches in a row on every trial's chain were one launch boundary too many)
__global__ __launch_bounds__(64) void ba_cam_rhs_offdiag_kernel(BaView v, const double* __restrict__ lamp) {
  if ((int)blockIdx.x < v.nc) ba_cam_rhs_fused_body(v, lamp, blockIdx.x, threadIdx.x);
  else ba_offdiag_body(v, (int)blockIdx.x - v.nc, threadIdx.x);
}

// ---- elimination of the cuboids (BaView::elim) ------------------------------------------------------------------------------
// A free cuboid is coupled to the cameras that observe it and to nothing else, so it leaves the reduced system exactly like a landmark
// (block_solver.hpp:385-431 with a 9 x 9 block): D_oo^-1 = (H_oo + lambda I)^-1, S(c_a, c_b) -= M_a D_oo^-1 M_b^T for every pair of
// observing cameras, b_schur(c_a) -= M_a D_oo^-1 b_o, with M_a = the 6 x 9 camera-cuboid block summed over the edges of slot a (a
// camera may hold an EdgeSE3Cuboid and an EdgeSE3CuboidProj to the same cuboid).  One wavefront per cuboid; the blocks and vectors go
// to the same partial arrays as the landmark segments' and are summed by the same destination schedule.
__global__ __launch_bounds__(256) void ba_cub_elim_kernel(BaView v, const double* __restrict__ lamp) {
  const double lambda = lamp[0];
  // M, G: 54 doubles per slot of the graph's widest cuboid (dynamic: sized for BA_ELIM_MAX_SLOTS = 64 slots they took 55 KB of a CU's LDS from the
  // landmark segments' kernel that runs beside this one; a C4 cuboid has ~20 observing cameras)
  extern __shared__ double elim_lds[];
  double (*M)[54] = reinterpret_cast<double (*)[54]>(elim_lds);
  double (*G)[54] = reinterpret_cast<double (*)[54]>(elim_lds + 54 * (size_t)v.elim_max_slots);
  __shared__ double A[9][9], Di[9][9], bo[9];
  const int o = blockIdx.x, t = threadIdx.x;
  if (v.cub_col[o] < 0 || !v.cub_mine[o]) return;      // another rank's cuboid: its partial blocks, M and D^-1 stay zero here
  const int s0 = v.cubS_ptr[o], ns = v.cubS_ptr[o + 1] - s0;
  // M_s: one thread per (slot, element), the slot's edges in edge order
  for (int e = t; e < ns * 54; e += 256) {
    const int sl = e / 54, el = e - 54 * sl;
    double sv = 0;
    for (int q = v.slotE_ptr[s0 + sl]; q < v.slotE_ptr[s0 + sl + 1]; q++) sv += v.ce_Hco[54 * (size_t)v.slotE_idx[q] + el];
    M[sl][el] = sv;
    v.cub_M[54 * (size_t)(s0 + sl) + el] = sv;
  }
  for (int e = t; e < 81; e += 256) A[e / 9][e % 9] = v.Hcub[81 * (size_t)o + e] + ((e / 9 == e % 9) ? lambda : 0.0);
  __syncthreads();
  // Cholesky A = L L^T, then Di = L^-T L^-1 (9 x 9).  Round 6: on the lanes of the first wave with L and X in LDS -- as one lane with L and X
  // as local arrays (dynamic indices: 1.3 KB of scratch per lane) it was ~1 500 dependent scratch accesses, most of the kernel's 80-95 us.
  // Every entry is formed by the same operations in the same order as before (a column of L by the lanes of its rows, a column of L^-1 by
  // one lane, an entry of Di by one lane): the same bits.
  __shared__ double Lm[9][9], Xm[9][9];
  if (t < 64) {
    bool fail = false;
    for (int j = 0; j < 9; j++) {
      double d = A[j][j];
      for (int k = 0; k < j; k++) d -= Lm[j][k] * Lm[j][k];
      if (!(d > 0.0)) { fail = true; d = 1.0; }
      const double r = sqrt(d);
      if (t == j) Lm[j][j] = r;
      if (t > j && t < 9) {
        double sv = A[t][j];
        for (int k = 0; k < j; k++) sv -= Lm[t][k] * Lm[j][k];
        Lm[t][j] = sv / r;
      }
      __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      __builtin_amdgcn_wave_barrier();
    }
    if (t < 9) {         // X = L^-1 (lower triangular): lane c forms column c
      const int c = t;
      for (int i = 0; i < 9; i++) {
        double sv = (i == c) ? 1.0 : 0.0;
        for (int k = c; k < i; k++) sv -= Lm[i][k] * Xm[k][c];
        Xm[i][c] = (i >= c) ? sv / Lm[i][i] : 0.0;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    for (int e = t; e < 81; e += 64) {
      const int i = e / 9, j = e - 9 * i;
      double sv = 0;
      for (int k = (i > j ? i : j); k < 9; k++) sv += Xm[k][i] * Xm[k][j];
      Di[i][j] = sv;
    }
    if (fail && t == 0) atomicExch(v.elim_fail, 1);
  }
  __syncthreads();
  for (int e = t; e < 81; e += 256) v.cub_Dinv[81 * (size_t)o + e] = Di[e / 9][e % 9];
  if (t < 9) { double sv = 0; for (int k = 0; k < 9; k++) sv += Di[t][k] * v.bcub[9 * (size_t)o + k]; bo[t] = sv; }
  __syncthreads();
  // G_s = M_s D^-1, the slot's share of the right-hand side
  for (int e = t; e < ns * 54; e += 256) {
    const int sl = e / 54, r = (e % 54) / 9, c = e % 9;
    double sv = 0;
    for (int k = 0; k < 9; k++) sv += M[sl][9 * r + k] * Di[k][c];
    G[sl][9 * r + c] = sv;
  }
  for (int e = t; e < ns * 6; e += 256) {
    const int sl = e / 6, r = e % 6;
    double sv = 0;
    for (int k = 0; k < 9; k++) sv += M[sl][9 * r + k] * bo[k];
    v.part_coef[6 * (size_t)(v.cub_coef[o] + sl) + r] = sv;
  }
  __syncthreads();
  // the slot pairs a <= b (slots are sorted by column): block(r, c) = sum_m G_a(r, m) M_b(c, m)
  const int npair = ns * (ns + 1) / 2;
  for (int e = t; e < npair * 36; e += 256) {
    const int pr = e / 36, rc = e % 36, r = rc / 6, c = rc % 6;
    // pair index -> (a, b), a <= b: pr = a ns - a (a - 1) / 2 + (b - a)  (closed form + correction, as ba_schur_long_kernel; the walk over
    // the rows it replaces was up to ns steps for every one of the block's 36 entries)
    const float tk = (float)(2 * ns + 1);
    int a = (int)((tk - __builtin_sqrtf(tk * tk - 8.0f * (float)pr)) * 0.5f);
    a = max(0, min(ns - 1, a));
    while (a > 0 && a * ns - a * (a - 1) / 2 > pr) a--;
    while ((a + 1) * ns - (a + 1) * a / 2 <= pr) a++;
    const int b = a + (pr - (a * ns - a * (a - 1) / 2));
    double sv = 0;
    for (int m = 0; m < 9; m++) sv += G[a][9 * r + m] * M[b][9 * c + m];
    v.part_tiles[36 * (size_t)(v.cub_tile[o] + pr) + rc] = sv;
  }
}

// x_o = D_oo^-1 (b_o - sum_s M_s^T x_cam(s))   (block_solver.hpp:457-482 for the cuboid blocks)
__device__ __forceinline__ void cub_backsub_wave(const BaView& v, int o, int t, double* cl) {     // one wavefront; cl: 9 doubles of LDS of its own
  const int col = v.cub_col[o];
  if (col < 0) return;
  if (t < 9) {
    double acc = v.bcub[9 * (size_t)o + t];
    for (int sl = v.cubS_ptr[o]; sl < v.cubS_ptr[o + 1]; sl++) {
      const double* Ms = v.cub_M + 54 * (size_t)sl;
      const double* xp = v.rhs + v.cam_col[v.cubS_cam[sl]];
      double sv = 0;
      for (int r = 0; r < 6; r++) sv += Ms[9 * r + t] * (-xp[r]);
      acc += sv;
    }
    cl[t] = acc;
  }
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  __builtin_amdgcn_wave_barrier();
  if (t < 9) {
    double sv = 0;
    for (int k = 0; k < 9; k++) sv += v.cub_Dinv[81 * (size_t)o + 9 * t + k] * cl[k];
    v.rhs[col + t] = sv;
  }
}
__global__ __launch_bounds__(64) void ba_cub_backsub_kernel(BaView v) {
  __shared__ double cl[9];
  cub_backsub_wave(v, blockIdx.x, threadIdx.x, cl);
}

// (Round 5 tried the H_pl records as one coalesced stream through LDS, a lane per edge, the landmark's lane summing in edge order: 84 us
// against 80 at C4 -- the 163 MB read is not what this kernel waits for -- and was dropped.)
__device__ __forceinline__ void backsub_point(const BaView& v, int p) {
  if (p >= v.np) return;
  double cl[3] = {v.bl[3 * p], v.bl[3 * p + 1], v.bl[3 * p + 2]};
  for (int k = v.pt_ptr[p]; k < v.pt_ptr[p + 1]; k++) {
    int col = v.cam_col[v.pm_cam[k]];
    if (col < 0) continue;
    const double* Wk = v.W + 18 * (size_t)k;
    const double* xp = v.rhs + col;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      double s = 0;
#pragma unroll
      for (int r = 0; r < 6; r++) s += Wk[3 * r + c] * (-xp[r]);
      cl[c] += s;
    }
  }
  double x[3];
  mat3_vec(v.Dinv + 9 * (size_t)p, cl, x);
  v.xl[3 * p] = x[0]; v.xl[3 * p + 1] = x[1]; v.xl[3 * p + 2] = x[2];
}

// The same with H_pl formed on the spot (the fused linearise-in-Schur trials, which never write it): per edge the camera, the point, the
// measurement -- the proj_linearize and the lin_hpl that ba_lin_schur_segment / lin_pt_edge call (ba_proj_edge.h), then the same
// sums in the same order as the kernel above: the same x_l bit for bit (tests/test_ba_gpu.py holds the LM run to the classic pair).
template <bool STEREO>
__device__ __forceinline__ void backsub_lin_point(const BaView& v, int p) {
  if (p >= v.np) return;
  const ProjTable<STEREO> E(v, PointMajor{});
  double cl[3] = {v.bl[3 * p], v.bl[3 * p + 1], v.bl[3 * p + 2]};
  const bool free_pt = v.pt_free[p] != 0;
  const double X[3] = {v.points[3 * (size_t)p], v.points[3 * (size_t)p + 1], v.points[3 * (size_t)p + 2]};
  for (int k = v.pt_ptr[p]; k < v.pt_ptr[p + 1]; k++) {
    const int c = v.pm_cam[k];
    int col = v.cam_col[c];
    if (col < 0) continue;
    Pose T = pose_load(v.cams + 7 * c);
    double R[9];
    pose_rotmat(T, R);
    double Wk[18];
    ProjLinT<STEREO ? 3 : 2> L;
    proj_linearize(E, k, T, R, X, L);
    lin_hpl(L, free_pt, [&](int q, int j) -> double& { return Wk[3 * q + j]; });      // (the camera is free here)
    const double* xp = v.rhs + col;
#pragma unroll
    for (int cc = 0; cc < 3; cc++) {
      double s = 0;
#pragma unroll
      for (int r = 0; r < 6; r++) s += Wk[3 * r + cc] * (-xp[r]);
      cl[cc] += s;
    }
  }
  double x[3];
  mat3_vec(v.Dinv + 9 * (size_t)p, cl, x);
  v.xl[3 * p] = x[0]; v.xl[3 * p + 1] = x[1]; v.xl[3 * p + 2] = x[2];
}

// Both back-substitutions of a trial in ONE launch: the eliminated cuboids' blocks first (a wave per cuboid: x_o from the cameras' x_p), the
// landmarks' behind them -- the two read the cameras' increments only and write disjoint outputs.  LIN: H_pl formed on the spot (above).
template <bool LIN, bool STEREO>
__global__ __launch_bounds__(256) void ba_backsub_all_kernel(BaView v, int n_cub_blocks) {
  __shared__ double cl[4][9];
  if ((int)blockIdx.x < n_cub_blocks) {
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o < v.no) cub_backsub_wave(v, o, threadIdx.x & 63, cl[threadIdx.x >> 6]);
    return;
  }
  const int p = (blockIdx.x - n_cub_blocks) * 256 + threadIdx.x;
  if (LIN) backsub_lin_point<STEREO>(v, p); else backsub_point(v, p);
}

// bak_*: non-null = the push of the LM trial rides along (OptimizableGraph::push before the update, optimization_algorithm_levenberg.cpp:104-
// 113): every vertex's estimate goes to its backup slot before it is changed -- three device-to-device copies of the whole state per trial
// (~50 us at C4) become a few more stores of a kernel that reads the state anyway
__device__ __forceinline__ void update_vertex(const BaView& v, int i, double* bak_cams, double* bak_points, double* bak_cubes) {
  if (i < v.np) {
    if (bak_points) { bak_points[3 * i] = v.points[3 * i]; bak_points[3 * i + 1] = v.points[3 * i + 1]; bak_points[3 * i + 2] = v.points[3 * i + 2]; }
    if (v.pt_free[i]) { v.points[3 * i] += v.xl[3 * i]; v.points[3 * i + 1] += v.xl[3 * i + 1]; v.points[3 * i + 2] += v.xl[3 * i + 2]; }
    return;
  }
  i -= v.np;
  if (i < v.nc) {
    if (bak_cams) for (int q = 0; q < 7; q++) bak_cams[7 * i + q] = v.cams[7 * i + q];
    int col = v.cam_col[i];
    if (col >= 0) pose_store(cam_oplus(pose_load(v.cams + 7 * i), v.rhs + col), v.cams + 7 * i);
    return;
  }
  i -= v.nc;
  if (i < v.no) {
    if (bak_cubes) for (int q = 0; q < 10; q++) bak_cubes[10 * i + q] = v.cubes[10 * i + q];
    int col = v.cub_col[i];
    if (col >= 0) cube_store(cube_oplus(cube_load(v.cubes + 10 * i), v.rhs + col), v.cubes + 10 * i);
  }
}
__global__ __launch_bounds__(256) void ba_update_kernel(BaView v, double* bak_cams, double* bak_points, double* bak_cubes) {
  update_vertex(v, blockIdx.x * 256 + threadIdx.x, bak_cams, bak_points, bak_cubes);
}
// the LM scale term and the update of a trial in ONE launch: x^T (lambda x + b) reads the increments and the right-hand sides, the update reads
// the increments and writes the estimates -- independent; the SCALE_BLOCKS partial sums keep their places
__global__ __launch_bounds__(256) void ba_scale_update_kernel(BaView v, const double* __restrict__ lamp, double* partial, double* bak_cams, double* bak_points, double* bak_cubes) {
  __shared__ double ws[4];
  if (blockIdx.x < SCALE_BLOCKS) { scale_block(v, lamp, partial, blockIdx.x, ws); return; }
  update_vertex(v, (blockIdx.x - SCALE_BLOCKS) * 256 + threadIdx.x, bak_cams, bak_points, bak_cubes);
}

// status words of a trial -> one double (0 = fine), so that the flag can ride in the scalar all-reduce of the trial
__global__ void ba_fail_flag_kernel(const int* a, const int* b, const int* c, double* out) {
  if (threadIdx.x == 0) *out = ((a && *a) || (b && *b) || (c && *c)) ? 1.0 : 0.0;
}

void ba_launch_fail_flag(const int* a, const int* b, const int* c, double* out, hipStream_t st) {
  hipLaunchKernelGGL(ba_fail_flag_kernel, dim3(1), dim3(64), 0, st, a, b, c, out);
}

// ---------------------------------------------------------------------------------------- launchers --
// dst[r][0..width) = src[idx[r]][0..width): the structure phase's edge tables are permuted on the device (point-major order from
// the caller's order, camera-major from point-major) instead of on the host + a second upload
__global__ __launch_bounds__(256) void ba_gather_rows_kernel(const double* __restrict__ src, const int* __restrict__ idx, long long total, int width, double* __restrict__ dst) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long long r = t / width;
  const int c = (int)(t - r * width);
  dst[t] = src[(long long)idx[r] * width + c];
}
// dst[r][0..4) = the same four doubles for every row: the per-edge information / intrinsics records of a graph whose edges all shared one
// record, written out when an appended edge brings another (cs_ba_append_edges_proj) -- such a graph never uploads the records themselves
__global__ __launch_bounds__(256) void ba_fill_rows4_kernel(double* __restrict__ dst, double a, double b, double c, double d, long long total) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int q = (int)(t & 3);
  dst[t] = q == 0 ? a : (q == 1 ? b : (q == 2 ? c : d));
}
void ba_launch_fill_rows4(double* dst, const double* rec4, long long rows, hipStream_t st) {
  if (rows <= 0) return;
  hipLaunchKernelGGL(ba_fill_rows4_kernel, dim3((unsigned)((4 * rows + 255) / 256)), dim3(256), 0, st, dst, rec4[0], rec4[1], rec4[2], rec4[3], 4 * rows);
}
void ba_launch_gather_rows(const double* src, const int* idx, int n, int width, double* dst, hipStream_t st) {
  const long long total = (long long)n * width;
  if (total <= 0) return;
  hipLaunchKernelGGL(ba_gather_rows_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, src, idx, total, width, dst);
}

int ba_chi2_blocks(int n_proj) { int nb = (n_proj + 255) / 256; return nb < 1 ? 1 : (nb > 2048 ? 2048 : nb); }

// which instantiation of a projection-edge kernel a graph runs: f(std::true_type) where it holds a stereo edge, f(std::false_type) where not
template <class F>
static void with_edge_kinds(const BaView& v, F&& f) { if (v.pm_kind) f(std::true_type{}); else f(std::false_type{}); }

void ba_launch_chi2(const BaView& v, int nb_proj, hipStream_t st) {
  const int ne = v.n_cub + v.n_odom, nb_pose = (ne + 63) / 64;
  with_edge_kinds(v, [&](auto stereo) { hipLaunchKernelGGL(ba_chi2_kernel<decltype(stereo)::value>, dim3(nb_proj + (nb_pose + 3) / 4), dim3(256), 0, st, v, nb_proj, nb_pose); });
}
// the numeric-Jacobian edges (cuboid, odometry: few edges, long dependent chains) run beside the projection edges (many edges, short
// chains) on a second stream; ba_accum_pose_kernel needs both
// Three streams: the camera kernel is one workgroup per camera (1000 at C4: a fraction of the CUs), so the landmark kernel runs
// beside it on st3 and the numeric-Jacobian edges (cuboid, odometry) on st2; all meet before the per-vertex accumulation.
// ev_pre (optional): an event ALREADY recorded on st at the point from which the state no longer changes -- the side streams then start from
// there instead of from this call (a speculated linearisation: the numeric-Jacobian edges run beside the chi2 kernels of the trial before it)
void ba_launch_linearize(const BaView& v, hipStream_t st, hipStream_t st2, hipEvent_t ev_fork, hipEvent_t ev_join, hipStream_t st3, hipEvent_t ev_join3, hipEvent_t ev_pre) {
  const bool side = v.n_cub > 0;
  const bool lin_pt = v.np > 0 && !v.fuse_lin;       // (fuse_lin: the Schur kernels of this iteration's trials linearise the landmark side themselves)
  const bool side3 = lin_pt && (v.n_proj > 0 || v.nc > 0);
  hipStream_t se = side ? st2 : st;
  if ((side || side3) && !ev_pre) (void)hipEventRecord(ev_fork, st);
  if (ev_pre) ev_fork = ev_pre;
  if (side) (void)hipStreamWaitEvent(st2, ev_fork, 0);
  const int ob = (v.n_cub3 > 0 && v.n_odom > 0) ? (v.n_odom + 7) / 8 : 0;      // the odometry edges as the cuboid launch's first workgroups
  if (v.n_cub3 > 0) hipLaunchKernelGGL(ba_cub_edge_kernel<true>, dim3((v.n_cub3 + 3) / 4 + ob), dim3(128), 0, se, v, ob);
  if (v.n_cub > v.n_cub3) hipLaunchKernelGGL(ba_cub_edge_kernel<false>, dim3((v.n_cub - v.n_cub3 + 3) / 4), dim3(128), 0, se, v, 0);
  // (the odometry edges: a single short wave per four edges, 38 us of latency -- beside the cuboid edges on the main stream, not behind
  // them on the side stream, whose 135 us are the phase's critical path)
  // (the odometry edges behind the cuboid edges on the side stream: ~250 short wavefronts, 35 us; in front of the camera sums on the main
  // stream -- rounds 3-4 -- they waited for wave slots beside the cuboid edges for 112 us, behind them they lengthen the main stream's chain)
  if (v.n_odom > 0 && ob == 0) hipLaunchKernelGGL(ba_odom_edge_kernel, dim3((v.n_odom + 3) / 4), dim3(64), 0, se, v);
  if (side) (void)hipEventRecord(ev_join, st2);
  auto launch_lin_pt = [&](hipStream_t s) {
    with_edge_kinds(v, [&](auto stereo) { hipLaunchKernelGGL(ba_lin_pt_kernel<decltype(stereo)::value>, dim3((v.np + LIN_PT_GROUP - 1) / LIN_PT_GROUP), dim3(256), 0, s, v); });
  };
  if (side3) {
    (void)hipStreamWaitEvent(st3, ev_fork, 0);
    launch_lin_pt(st3);
    (void)hipEventRecord(ev_join3, st3);
  }
  if (v.n_proj > 0 || v.nc > 0) with_edge_kinds(v, [&](auto stereo) { hipLaunchKernelGGL(ba_lin_cam_kernel<decltype(stereo)::value>, dim3(v.nc), dim3(256), 0, st, v); });
  if (!side3 && lin_pt) launch_lin_pt(st);
  if (side) (void)hipStreamWaitEvent(st, ev_join, 0);
  if (side3) (void)hipStreamWaitEvent(st, ev_join3, 0);
  hipLaunchKernelGGL(ba_accum_pose_kernel, dim3(v.nc + v.no), dim3(128), 0, st, v, 0);
}
void ba_launch_reduce(const BaView& v, const double* lambda, hipStream_t st, hipStream_t st2, hipEvent_t ev_fork, hipEvent_t ev_join, const BaSidePrologue* sp) {   // lambda: device, [lambda, lambda of the pose diagonals in the scale term]
  // sp (optional): the trial's prologue has NOT been launched yet -- it goes to the side stream when there is one and the landmark segments can take
  // lambda by value (the fused-linearisation kernels, no long-track segments), else in front of everything on the main stream
  const bool side0 = v.fused && v.elim && v.no > 0 && st2 != nullptr;
  const bool sp_side = sp && side0 && v.fuse_lin && v.n_seg <= max(max(max(v.seg_class[0], v.seg_class[1]), max(v.seg_class[2], v.seg_class[3])), v.seg_class[4]);
  if (sp && !sp_side) ba_launch_trial_prologue(sp->d_lam, sp->lam0, sp->lam1, sp->info24, sp->elim_fail, sp->S, sp->n_clear, st);
  const double* lin_lamp = sp_side ? nullptr : lambda;
  const double lin_lam = sp_side ? sp->lam0 : 0.0;
  if (v.fused) {
    // the cuboid elimination (one workgroup per cuboid, latency-bound) runs beside the landmark segments on a second stream; both
    // write disjoint ranges of the partial arrays and meet before the destination schedule reads them
    const bool side = v.elim && v.no > 0 && st2 != nullptr;
    if (side) {
      (void)hipEventRecord(ev_fork, st);
      (void)hipStreamWaitEvent(st2, ev_fork, 0);
      if (sp_side) ba_launch_trial_prologue(sp->d_lam, sp->lam0, sp->lam1, sp->info24, sp->elim_fail, sp->S, sp->n_clear, st2);
      hipLaunchKernelGGL(ba_cub_elim_kernel, dim3(v.no), dim3(256), 2 * 54 * sizeof(double) * (size_t)v.elim_max_slots, st2, v, lambda);
    }
    // (the cuboid elimination must be dispatched BEFORE the bulk of the segments fills the device: started 18 us ahead -- behind the short
    // kernel of the one- and two-camera segments below -- its 500 workgroups run 90 us beside the bulk; started together with it they
    // queue for slots and take 200 us, whatever the stream priority.  Measured in round 5 by moving that short kernel to this stream.)
    if (side) (void)hipEventRecord(ev_join, st2);
    // the diagonal blocks / right-hand side of the cameras need the segments' partial vectors; the gather of the blocks runs last
    // (it subtracts from entries the vertex kernels have written)
    {
      // (class boundaries are cumulative: a class without segments repeats the boundary before it)
      int c0 = v.seg_class[0], c1 = max(c0, v.seg_class[1]), c2 = max(c1, v.seg_class[2]), c3 = max(c2, v.seg_class[3]);
      const int c4 = max(c3, v.seg_class[4]);
      if (v.fuse_lin) {
        // (round 6: the one- and two-camera segments ride in the <2> launch -- the same products on the same operands, their second tile idle --
        // instead of a 17 us launch of their own in front of it: the two kernels never overlapped; C4 1 312-1 324 -> 1 336-1 342 LM it/s)
        if (c1 > c0) c0 = 0;
        const int cb[6] = {0, c0, c1, c2, c3, c4};
        auto launch = [&](auto kern, int lo, int hi) { if (hi > lo) hipLaunchKernelGGL(kern, dim3((hi - lo + 3) / 4), dim3(256), 0, st, v, lin_lamp, lo, hi, lin_lam); };
        with_edge_kinds(v, [&](auto stereo) {
          constexpr bool S = decltype(stereo)::value;
          launch(ba_lin_schur_kernel<1, S>, cb[0], cb[1]); launch(ba_lin_schur_kernel<2, S>, cb[1], cb[2]); launch(ba_lin_schur_kernel<3, S>, cb[2], cb[3]);
          launch(ba_lin_schur_kernel<4, S>, cb[3], cb[4]); launch(ba_lin_schur_kernel<5, S>, cb[4], cb[5]);
        });
      } else {
        if (c0 > 0) hipLaunchKernelGGL(ba_schur_fused_kernel<1>, dim3((c0 + 3) / 4), dim3(256), 0, st, v, lambda, 0, c0);
        if (c1 > c0) hipLaunchKernelGGL(ba_schur_fused_kernel<2>, dim3((c1 - c0 + 3) / 4), dim3(256), 0, st, v, lambda, c0, c1);
        if (c2 > c1) hipLaunchKernelGGL(ba_schur_fused_kernel<3>, dim3((c2 - c1 + 3) / 4), dim3(256), 0, st, v, lambda, c1, c2);
        if (c3 > c2) hipLaunchKernelGGL(ba_schur_fused_kernel<4>, dim3((c3 - c2 + 3) / 4), dim3(256), 0, st, v, lambda, c2, c3);
        if (c4 > c3) hipLaunchKernelGGL(ba_schur_fused_kernel<5>, dim3((c4 - c3 + 3) / 4), dim3(256), 0, st, v, lambda, c3, c4);
      }
      if (v.n_seg > c4) hipLaunchKernelGGL(ba_schur_long_kernel, dim3((v.n_seg - c4 + 3) / 4), dim3(256), 0, st, v, lambda, c4, v.n_seg);
    }
    if (side) (void)hipStreamWaitEvent(st, ev_join, 0);
    else if (v.elim && v.no > 0) hipLaunchKernelGGL(ba_cub_elim_kernel, dim3(v.no), dim3(256), 2 * 54 * sizeof(double) * (size_t)v.elim_max_slots, st, v, lambda);
    hipLaunchKernelGGL(ba_cam_rhs_offdiag_kernel, dim3(v.nc + v.n_cub + v.n_odom), dim3(64), 0, st, v, lambda);
    if (!v.elim && v.no > 0) hipLaunchKernelGGL(ba_cub_scatter_kernel, dim3(v.no), dim3(128), 0, st, v, lambda);
    if (v.n_gpairs > 0) hipLaunchKernelGGL(ba_schur_gather_kernel, dim3((v.n_gpairs + 3) / 4), dim3(256), 0, st, v);
    return;
  }
  if (v.np > 0) hipLaunchKernelGGL(ba_prep_kernel, dim3((v.np + 255) / 256), dim3(256), 0, st, v, lambda);
  if (v.n_proj > 0) hipLaunchKernelGGL(ba_wd_kernel, dim3((unsigned)((6 * (size_t)v.n_proj + 255) / 256)), dim3(256), 0, st, v);
  hipLaunchKernelGGL(ba_cam_rhs_kernel, dim3(v.nc), dim3(256), 0, st, v, lambda);
  if (v.no > 0) hipLaunchKernelGGL(ba_cub_scatter_kernel, dim3(v.no), dim3(128), 0, st, v, lambda);
  if (v.n_cub + v.n_odom > 0) hipLaunchKernelGGL(ba_offdiag_kernel, dim3(v.n_cub + v.n_odom), dim3(64), 0, st, v);
  if (v.n_pairs > 0) hipLaunchKernelGGL(ba_schur_kernel, dim3((v.n_pairs + 1) / 2), dim3(128), 0, st, v);
}
// ---- debug: NaN / Inf scan (cs_ba_check_finite, CS_BA_DEBUG_NAN) -------------------------------------------------------------------
// g2o's debug builds look for NaNs where they are born: in the errors (SparseOptimizer::computeActiveErrors, sparse_optimizer.cpp:78-86)
// and in the Jacobians of every edge (BlockSolver::buildSystem, block_solver.hpp:533-544).  Here the errors and Jacobians never reach
// memory, so the scan covers what they turn into -- the edges' squared errors, every block of the linear system, the increments and
// the estimates -- and names the first offending entry of each array.  out[2 t] = number of non-finite entries of array t,
// out[2 t + 1] = smallest offending index + 1.
__global__ __launch_bounds__(256) void ba_scan_finite_kernel(const double* p, long long n, int* out) {
  int bad = 0;
  long long first = -1;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    const double x = p[i];
    if (!(x - x == 0.0)) { bad++; if (first < 0) first = i; }     // NaN and +-Inf
  }
  if (bad) { atomicAdd(out, bad); atomicMin((unsigned*)(out + 1), (unsigned)min(first + 1, 0x7ffffffeLL)); }
}
void ba_launch_scan_finite(const double* p, long long n, int* out, hipStream_t st) {
  if (n <= 0 || !p) return;
  const long long nb = (n + 255) / 256;
  hipLaunchKernelGGL(ba_scan_finite_kernel, dim3((unsigned)(nb > 2048 ? 2048 : nb)), dim3(256), 0, st, p, n, out);
}
// the edges' (un-robustified) squared errors e^T Omega e, one double per edge: projection edges (point-major order), then the
// camera-cuboid and the odometry edges -- what a NaN in an error vector turns into
// (a level-1 edge is not evaluated and reads as 0: projection edges by their width record's sign, the others through lvl_ce / lvl_oe, nullptr
// while none of them is at level 1)
template <bool STEREO>
__global__ __launch_bounds__(256) void ba_edge_chi_kernel(BaView v, double* out, const unsigned char* lvl_ce, const unsigned char* lvl_oe) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < v.n_proj) {
    if (edge_off(v.pm_huber[k])) { out[k] = 0.0; return; }
    double pc[3];
    out[k] = proj_edge_chi(ProjTable<STEREO>(v, PointMajor{}), k, pc);
    return;
  }
  const int q = k - v.n_proj;
  if (q < v.n_cub ? (lvl_ce && lvl_ce[q]) : (q < v.n_cub + v.n_odom && lvl_oe && lvl_oe[q - v.n_cub])) { out[k] = 0.0; return; }
  if (q < v.n_cub3) {
    double e[9];
    cuboid_edge_error(pose_load(v.cams + 7 * v.ce_cam[q]), cube_load(v.cubes + 10 * v.ce_cub[q]), cube_load(v.ce_meas + 10 * q), e);
    out[k] = quad_form(e, v.ce_info + 81 * q, 9);
  } else if (q < v.n_cub) {
    const int r = q - v.n_cub3;
    double e[4];
    cuboid_proj_error(pose_load(v.cams + 7 * v.ce_cam[q]), cube_load(v.cubes + 10 * v.ce_cub[q]), v.pe_K + 9 * (size_t)r, v.pe_meas + 4 * (size_t)r, e);
    out[k] = quad_form(e, v.pe_info + 16 * (size_t)r, 4);
  } else if (q < v.n_cub + v.n_odom) {
    const int r = q - v.n_cub;
    double e[6];
    odom_edge_error(pose_load(v.cams + 7 * v.oe_i[r]), pose_load(v.cams + 7 * v.oe_j[r]), pose_load(v.oe_meas + 7 * r), e);
    out[k] = quad_form(e, v.oe_info + 36 * r, 6);
  }
}
void ba_launch_edge_chi(const BaView& v, double* out, hipStream_t st, const unsigned char* lvl_ce, const unsigned char* lvl_oe) {
  const int n = v.n_proj + v.n_cub + v.n_odom;
  if (n <= 0) return;
  with_edge_kinds(v, [&](auto stereo) { hipLaunchKernelGGL(ba_edge_chi_kernel<decltype(stereo)::value>, dim3((n + 255) / 256), dim3(256), 0, st, v, out, lvl_ce, lvl_oe); });
}

// ---- edge levels (OptimizableGraph::Edge::setLevel) of the projection edges: see edge_off ------------------------------------------------
// The structure phase's gather of the width records, point-major from the caller's order: a width <= 0 (no kernel) becomes +0.0, so that the sign
// bit is free for the level; lvl (caller's order, nullptr: every edge at level 0) sets it.  src == nullptr: no edge has a width.
__global__ __launch_bounds__(256) void ba_gather_widths_kernel(const double* __restrict__ src, const int* __restrict__ idx, const unsigned char* __restrict__ lvl, int n, double* __restrict__ dst) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int s = idx[k];
  const double h = src ? src[s] : 0.0;
  const double w = h > 0 ? h : 0.0;
  dst[k] = (lvl && lvl[s]) ? -w : w;
}
void ba_launch_gather_widths(const double* src, const int* idx, const unsigned char* lvl, int n, double* dst, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ba_gather_widths_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, src, idx, lvl, n, dst);
}
// new levels into the point-major width records of a finished structure (cs_ba_set_edge_levels): the widths stay, the signs follow lvl
__global__ __launch_bounds__(256) void ba_relabel_widths_kernel(double* __restrict__ pm_huber, const int* __restrict__ idx, const unsigned char* __restrict__ lvl, int n) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const double w = fabs(pm_huber[k]);
  pm_huber[k] = lvl[idx[k]] ? -w : w;
}
void ba_launch_relabel_widths(double* pm_huber, const int* idx, const unsigned char* lvl, int n, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ba_relabel_widths_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pm_huber, idx, lvl, n);
}
__global__ __launch_bounds__(256) void ba_invert_perm_kernel(const int* __restrict__ perm, int n, int* __restrict__ inv) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k < n) inv[perm[k]] = k;
}
void ba_launch_invert_perm(const int* perm, int n, int* inv, hipStream_t st) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ba_invert_perm_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, perm, n, inv);
}
// cs_ba_classify_edges: ORB-SLAM2's outlier test between the rounds of LocalBundleAdjustment / BundleAdjustment (e->chi2() > 5.991 / 7.815 ||
// !e->isDepthPositive() -> setLevel(1)), one lane per projection edge over the point-major list at the current estimates.  Plain chi2 = e^T Omega e
// (the stereo error with its single-precision invz / bf: stereo_proj_error); depth = (T.map(X)).z, the test `not > 0` so that a NaN depth is out.
// sticky: a level-1 edge is not tested (and not evaluated unless its chi2 is asked for).  A changed level is written to the width record's sign
// in both edge orders and to the caller-order byte array; per class the lanes at level 1 afterwards are counted by ballot, one atomic per wavefront.
template <bool STEREO>
__global__ __launch_bounds__(256) void ba_classify_kernel(BaView v, BaClassify a) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  const ProjTable<STEREO> E(v, PointMajor{});
  bool stereo = false, out = false;
  if (k < v.n_proj) {
    stereo = E.stereo(k);
    const double h = a.pm_huber[k], thr = stereo ? a.thr_stereo : a.thr_mono;
    const bool was = edge_off(h), test = thr > 0 && !(a.sticky && was);
    out = was;
    if (test || a.chi_out) {
      double pc[3];
      const double chi = proj_edge_chi(E, k, pc);
      const int s = a.src[k];
      if (a.chi_out) a.chi_out[s] = chi;
      if (test) {
        out = chi > thr || (a.depth_positive && !(pc[2] > 0));
        if (out != was) {
          const double w = fabs(h), hn = out ? -w : w;
          a.pm_huber[k] = hn;
          a.cm_huber[a.pm_cm[k]] = hn;
        }
        a.lvl[s] = out ? 1 : 0;
      }
    }
  }
  const unsigned long long bm = __ballot(out && !stereo), bs = __ballot(out && stereo);
  if ((threadIdx.x & 63) == 0) {
    if (bm) atomicAdd(a.counts, __popcll(bm));
    if (bs) atomicAdd(a.counts + 1, __popcll(bs));
  }
}
void ba_launch_classify(const BaView& v, const BaClassify& a, hipStream_t st) {
  if (v.n_proj <= 0) return;
  with_edge_kinds(v, [&](auto stereo) { hipLaunchKernelGGL(ba_classify_kernel<decltype(stereo)::value>, dim3((unsigned)((v.n_proj + 255) / 256)), dim3(256), 0, st, v, a); });
}

// ---- external (host-evaluated) edges: cs_ba_set_external_edges / cs_ba_set_external_terms ---------------------------------------
// Edges of types the library does not evaluate go through their own linearizeOplus + constructQuadraticForm on the host
// (core/base_binary_edge.hpp:54-205, core/base_unary_edge.hpp:42-123); what those accumulate -- A_ii / b_i of the vertices, the
// off-diagonal block of a binary edge -- is added here to the blocks the device built from its own edges.
__global__ __launch_bounds__(256) void ba_ext_add_kernel(BaView v, const double* cam36, const double* cam6, const double* cub81, const double* cub9, const double* pt9, const double* pt3) {
  const long long nCam = (long long)v.nc * 42, nCub = (long long)v.no * 90, nPt = (long long)v.np * 12;
  long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t < nCam) {
    const int c = (int)(t / 42), e = (int)(t % 42);
    if (!cam36 || v.cam_col[c] < 0) return;
    if (e < 36) v.Hcam[36 * (size_t)c + e] += cam36[36 * (size_t)c + e]; else v.bcam[6 * (size_t)c + e - 36] += cam6[6 * (size_t)c + e - 36];
    return;
  }
  t -= nCam;
  if (t < nCub) {
    const int o = (int)(t / 90), e = (int)(t % 90);
    if (!cub81 || v.cub_col[o] < 0) return;
    if (e < 81) v.Hcub[81 * (size_t)o + e] += cub81[81 * (size_t)o + e]; else v.bcub[9 * (size_t)o + e - 81] += cub9[9 * (size_t)o + e - 81];
    return;
  }
  t -= nCub;
  if (t < nPt) {
    const int p = (int)(t / 12), e = (int)(t % 12);
    if (!pt9 || !v.pt_free[p]) return;
    if (e < 9) v.Hll[9 * (size_t)p + e] += pt9[9 * (size_t)p + e]; else v.bl[3 * (size_t)p + e - 9] += pt3[3 * (size_t)p + e - 9];
  }
}
// e4: (class_i, idx_i, class_j, idx_j) per edge, class 0 = camera (6), 1 = cuboid (9); Hij: 81 per edge, row-major dim_i x dim_j.
// A binary edge between two free pose vertices adds its block to the reduced system like an odometry edge's (ba_offdiag_kernel).
// One workgroup per destination pair of vertices (gptr / order: the edges grouped by unordered pair on the host, in the caller's order inside
// a group): its edges are added one after the other with plain read-modify-writes -- several edges on one pair, in either orientation, sum in
// a fixed order, like every other sum of the reduced system (no atomics: a trial's S does not depend on scheduling).
__global__ __launch_bounds__(128) void ba_ext_offdiag_kernel(BaView v, int n_groups, const int* gptr, const int* order, const int* e4, const double* Hij) {
  const int g = blockIdx.x, t = threadIdx.x;
  if (g >= n_groups) return;
  for (int q = gptr[g]; q < gptr[g + 1]; q++) {
    const int k = order[q];
    const int ci = e4[4 * k], ii = e4[4 * k + 1], cj = e4[4 * k + 2], ij = e4[4 * k + 3];
    if (ij < 0 || ci > 1 || cj > 1) continue;               // unary edge: diagonal terms only   (uniform over the workgroup)
    const int ca = ci ? v.cub_col[ii] : v.cam_col[ii], cb = cj ? v.cub_col[ij] : v.cam_col[ij];
    const int di = ci ? 9 : 6, dj = cj ? 9 : 6;
    if (ca < 0 || cb < 0 || ca >= v.n_red || cb >= v.n_red) continue;
    if (t < di * dj) {
      const int i = t / dj, j = t % dj;
      double* dst = cb > ca ? ba_S_at(v, cb + j, ca + i) : ba_S_at(v, ca + i, cb + j);
      *dst += Hij[81 * (size_t)k + t];
    }
    __syncthreads();     // (the next edge of the pair may be stored the other way round: another thread's element)
  }
}
void ba_launch_ext_add(const BaView& v, const double* cam36, const double* cam6, const double* cub81, const double* cub9, const double* pt9, const double* pt3, hipStream_t st) {
  const long long total = (long long)v.nc * 42 + (long long)v.no * 90 + (long long)v.np * 12;
  if (total > 0) hipLaunchKernelGGL(ba_ext_add_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, v, cam36, cam6, cub81, cub9, pt9, pt3);
}
void ba_launch_ext_offdiag(const BaView& v, int n_groups, const int* gptr, const int* order, const int* e4, const double* Hij, hipStream_t st) {
  if (n_groups > 0) hipLaunchKernelGGL(ba_ext_offdiag_kernel, dim3(n_groups), dim3(128), 0, st, v, n_groups, gptr, order, e4, Hij);
}
int ba_scale_blocks() { return SCALE_BLOCKS; }
// out[0] = sum of a[0 .. na), out[1] = sum of b[0 .. nb): fixed-shape tree (one workgroup), so the value does not depend on
// scheduling; lets chi2 and the LM scale term stay on the device until the one read-back (and RCCL all-reduce) of a trial
__global__ __launch_bounds__(256) void ba_sum2_kernel(const double* a, int na, const double* b, int nb, double* out) {
  __shared__ double ws[2][4];
  double sa = 0, sb = 0;
  for (int i = threadIdx.x; i < na; i += 256) sa += a[i];
  for (int i = threadIdx.x; i < nb; i += 256) sb += b[i];
  sa = wave_sum(sa); sb = wave_sum(sb);
  if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = sa; ws[1][threadIdx.x >> 6] = sb; }
  __syncthreads();
  if (threadIdx.x == 0) { out[0] = (ws[0][0] + ws[0][1]) + (ws[0][2] + ws[0][3]); out[1] = (ws[1][0] + ws[1][1]) + (ws[1][2] + ws[1][3]); }
}
void ba_launch_sum2(const double* a, int na, const double* b, int nb, double* out, hipStream_t st) {
  hipLaunchKernelGGL(ba_sum2_kernel, dim3(1), dim3(256), 0, st, a, na, b, nb, out);
}
// the same with the trial's failure flag in out[2] (ba_fail_flag_kernel's job, one launch fewer at the end of a trial)
// host_out (optional): the pinned mirror of the trial's scalars -- the three values and, behind a system-scope fence, the trial's sequence
// number, which the host polls: no copy command, no event, no signal between the last kernel of a trial and the host's decision
__global__ __launch_bounds__(256) void ba_sum2_flag_kernel(const double* a, int na, const double* b, int nb, const int* f0, const int* f1, double* out, double* host_out, double seq) {
  __shared__ double ws[2][4];
  double sa = 0, sb = 0;
  for (int i = threadIdx.x; i < na; i += 256) sa += a[i];
  for (int i = threadIdx.x; i < nb; i += 256) sb += b[i];
  sa = wave_sum(sa); sb = wave_sum(sb);
  if ((threadIdx.x & 63) == 0) { ws[0][threadIdx.x >> 6] = sa; ws[1][threadIdx.x >> 6] = sb; }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = (ws[0][0] + ws[0][1]) + (ws[0][2] + ws[0][3]); out[1] = (ws[1][0] + ws[1][1]) + (ws[1][2] + ws[1][3]);
    out[2] = ((f0 && *f0) || (f1 && *f1)) ? 1.0 : 0.0;
    if (host_out) {
      host_out[0] = out[0]; host_out[1] = out[1]; host_out[2] = out[2];
      __threadfence_system();
      __hip_atomic_store(host_out + 3, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}
void ba_launch_sum2_flag(const double* a, int na, const double* b, int nb, const int* f0, const int* f1, double* out, hipStream_t st, double* host_out, double seq) {
  hipLaunchKernelGGL(ba_sum2_flag_kernel, dim3(1), dim3(256), 0, st, a, na, b, nb, f0, f1, out, host_out, seq);
}
// computeLambdaInit (optimization_algorithm_levenberg.cpp:166-180): max |H_jj| over every non-fixed vertex -- cameras, cuboids, landmarks -- on the
// device (the maximum is exact whatever the order; non-negative doubles order like their bit patterns).  out[0] must be zero on entry.
__global__ __launch_bounds__(256) void ba_max_diag_kernel(BaView v, unsigned long long* out) {
  const long long nCam = 6ll * v.nc, nCub = 9ll * v.no, nPt = 3ll * v.np;
  double m = 0.0;
  for (long long t = (long long)blockIdx.x * 256 + threadIdx.x; t < nCam + nCub + nPt; t += (long long)gridDim.x * 256) {
    double x = 0.0;
    if (t < nCam) { const int i = (int)(t / 6), d = (int)(t % 6); if (v.cam_col[i] >= 0) x = v.Hcam[36 * (size_t)i + 7 * d]; }
    else if (t < nCam + nCub) { const long long q = t - nCam; const int i = (int)(q / 9), d = (int)(q % 9); if (v.cub_col[i] >= 0) x = v.Hcub[81 * (size_t)i + 10 * d]; }
    else { const long long q = t - nCam - nCub; const int i = (int)(q / 3), d = (int)(q % 3); if (v.pt_free[i]) x = v.Hll[9 * (size_t)i + 4 * d]; }
    x = fabs(x);
    if (x > m) m = x;      // (a NaN never wins, as in the reference's std::max(fabs(x), m) chain once a later entry follows it)
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) { const double y = __shfl_xor(m, o); if (y > m) m = y; }
  __shared__ double wm[4];
  if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {      // one atomic per workgroup (4096 wavefronts on one address took 50 us)
    const double a = wm[0] > wm[1] ? wm[0] : wm[1], b = wm[2] > wm[3] ? wm[2] : wm[3], mm = a > b ? a : b;
    if (mm > 0.0) atomicMax(out, (unsigned long long)__double_as_longlong(mm));
  }
}
void ba_launch_max_diag(const BaView& v, double* out, hipStream_t st) {
  const long long n = 6ll * v.nc + 9ll * v.no + 3ll * v.np;
  if (n <= 0) return;
  const long long nb = (n + 255) / 256;
  hipLaunchKernelGGL(ba_max_diag_kernel, dim3((unsigned)(nb > 512 ? 512 : nb)), dim3(256), 0, st, v, reinterpret_cast<unsigned long long*>(out));
}
// up to 48 buffers zeroed by one launch (the structure phase's allocations): blockIdx.y = buffer, 4-byte words
struct BaZeroList { unsigned* p[48]; unsigned long long words[48]; };
__global__ __launch_bounds__(256) void ba_multi_zero_kernel(BaZeroList L) {
  unsigned* __restrict__ p = L.p[blockIdx.y];
  const unsigned long long n = L.words[blockIdx.y];
  // 16 bytes per thread and step where the buffer allows it (hipMalloc aligns to 256 bytes)
  const unsigned long long n4 = n / 4;
  uint4* __restrict__ p4 = reinterpret_cast<uint4*>(p);
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (unsigned long long)gridDim.x * 256) p4[i] = make_uint4(0u, 0u, 0u, 0u);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3ull)) p[4 * n4 + threadIdx.x] = 0u;
}
void ba_launch_multi_zero(const std::pair<void*, size_t>* list, int n, hipStream_t st) {
  if (n <= 0) return;
  BaZeroList L;
  unsigned long long mx = 0;
  for (int i = 0; i < 48; i++) {
    const int q = i < n ? i : 0;
    L.p[i] = static_cast<unsigned*>(list[q].first);
    L.words[i] = i < n ? (list[q].second + 3) / 4 : 0;          // (every buffer's size is a multiple of 4 bytes: int and double elements)
    if (L.words[i] > mx) mx = L.words[i];
  }
  unsigned gx = (unsigned)std::min<unsigned long long>(512, (mx / 4 + 255) / 256 + 1);
  hipLaunchKernelGGL(ba_multi_zero_kernel, dim3(gx, n), dim3(256), 0, st, L);
}
// up to 48 small uploads by one launch: the sources sit in the structure phase's pinned staging arena (host memory the device reads over
// the link), the destinations are the handle's tables.  One hipMemcpyAsync per table was ~80 copies of a few KB in an appended frame's
// structure phase: 5 us of host time and a blit of its own on the stream apiece.  blockIdx.y = table, 4-byte words, 16-byte steps.
struct BaCopyList { unsigned* dst[48]; const unsigned* src[48]; unsigned long long words[48]; };
__global__ __launch_bounds__(256) void ba_multi_copy_kernel(BaCopyList L) {
  unsigned* __restrict__ d = L.dst[blockIdx.y];
  const unsigned* __restrict__ s = L.src[blockIdx.y];
  const unsigned long long n = L.words[blockIdx.y], n4 = n / 4;
  uint4* __restrict__ d4 = reinterpret_cast<uint4*>(d);
  const uint4* __restrict__ s4 = reinterpret_cast<const uint4*>(s);      // (arena offsets are multiples of 64 bytes, hipMalloc aligns to 256)
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (unsigned long long)gridDim.x * 256) d4[i] = s4[i];
  if (blockIdx.x == 0 && threadIdx.x < (n & 3ull)) d[4 * n4 + threadIdx.x] = s[4 * n4 + threadIdx.x];
}
void ba_launch_multi_copy(const BaCopyItem* list, int n, hipStream_t st) {
  if (n <= 0) return;
  BaCopyList L;
  unsigned long long mx = 0;
  for (int i = 0; i < 48; i++) {
    const int q = i < n ? i : 0;
    L.dst[i] = static_cast<unsigned*>(list[q].dst); L.src[i] = static_cast<const unsigned*>(list[q].src);
    L.words[i] = i < n ? list[q].bytes / 4 : 0;                   // (int and double elements: a multiple of 4 bytes)
    if (L.words[i] > mx) mx = L.words[i];
  }
  unsigned gx = (unsigned)std::min<unsigned long long>(64, (mx / 4 + 255) / 256 + 1);
  hipLaunchKernelGGL(ba_multi_copy_kernel, dim3(gx, n), dim3(256), 0, st, L);
}
// Head of a trial on the banded path: lambda into device memory (the kernels read it from there), the factorisation's status words,
// the cuboid elimination's failure word and the reduced system's right-hand side cleared -- one launch instead of a copy and three fills.
__global__ __launch_bounds__(256) void ba_trial_prologue_kernel(double* d_lam, double lam0, double lam1, int* info24, int* elim_fail, double* S, size_t n_clear) {
  // [S | rhs] cleared (16 bytes per thread and step: hipMalloc aligns to 256 bytes), the status words, lambda
  double2* __restrict__ S2 = reinterpret_cast<double2*>(S);
  const size_t n2 = n_clear / 2;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (size_t)gridDim.x * 256) S2[i] = make_double2(0.0, 0.0);
  if (blockIdx.x == 0) {
    if ((n_clear & 1) && threadIdx.x == BAND_INFO_WORDS + 3) S[n_clear - 1] = 0.0;
    if (threadIdx.x < BAND_INFO_WORDS) info24[threadIdx.x] = 0;
    if (threadIdx.x == BAND_INFO_WORDS) *elim_fail = 0;
    if (threadIdx.x == BAND_INFO_WORDS + 1) d_lam[0] = lam0;
    if (threadIdx.x == BAND_INFO_WORDS + 2) d_lam[1] = lam1;
  }
}
// S: the reduced system's buffer, n_clear = its doubles + the right-hand side's behind them (one buffer)
void ba_launch_trial_prologue(double* d_lam, double lam0, double lam1, int* info24, int* elim_fail, double* S, size_t n_clear, hipStream_t st) {
  const unsigned blocks = (unsigned)std::min<size_t>(1024, (n_clear / 2 + 255) / 256 + 1);
  hipLaunchKernelGGL(ba_trial_prologue_kernel, dim3(blocks), dim3(256), 0, st, d_lam, lam0, lam1, info24, elim_fail, S, n_clear);
}
void ba_launch_scale(const BaView& v, const double* lambda, double* partial, hipStream_t st) {
  hipLaunchKernelGGL(ba_scale_kernel, dim3(SCALE_BLOCKS), dim3(256), 0, st, v, lambda, partial);
}
void ba_launch_backsub(const BaView& v, hipStream_t st) {
  const int ncb = (v.elim && v.no > 0) ? (v.no + 3) / 4 : 0, npb = (v.np + 255) / 256;
  if (ncb + npb <= 0) return;
  if (!v.fuse_lin) hipLaunchKernelGGL((ba_backsub_all_kernel<false, false>), dim3(ncb + npb), dim3(256), 0, st, v, ncb);
  else with_edge_kinds(v, [&](auto stereo) { hipLaunchKernelGGL((ba_backsub_all_kernel<true, decltype(stereo)::value>), dim3(ncb + npb), dim3(256), 0, st, v, ncb); });      // (the trial's Schur kernels did not write H_pl)
}
void ba_launch_scale_update(const BaView& v, const double* lambda, double* partial, hipStream_t st, double* bak_cams, double* bak_points, double* bak_cubes) {
  const int n = v.np + v.nc + v.no;
  hipLaunchKernelGGL(ba_scale_update_kernel, dim3(SCALE_BLOCKS + (n + 255) / 256), dim3(256), 0, st, v, lambda, partial, bak_cams, bak_points, bak_cubes);
}
void ba_launch_update(const BaView& v, hipStream_t st, double* bak_cams, double* bak_points, double* bak_cubes) {
  int n = v.np + v.nc + v.no;
  if (n > 0) hipLaunchKernelGGL(ba_update_kernel, dim3((n + 255) / 256), dim3(256), 0, st, v, bak_cams, bak_points, bak_cubes);
}

}  // namespace cs
