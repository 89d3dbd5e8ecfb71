// ba_proj_edge.h -- the projection edge of the bundle adjustment (EdgeSE3ProjectXYZ, EdgeStereoSE3ProjectXYZ), stated once for
// every kernel of ba_kernels.hip that evaluates one, and for the host (tools/hostonly/ba_proj_edge_check.cpp):
//   ProjTable         a view of one of the two edge tables of a BaView (point-major / camera-major) whose accessors hide the
//                     uniform-or-per-edge choice of the records;
//   proj_edge_chi     the plain chi2 e^T Omega e of an edge of either kind;
//   proj_linearize    error, analytic Jacobians (types_six_dof_expmap.cpp:148-184, :240-279) and the weights of constructQuadraticForm
//                     (base_binary_edge.hpp:54-120) as a ProjLinT<2> (mono graphs) or a ProjLinT<3> (graphs that hold a stereo edge);
//   lin_cam_terms / lin_point_terms / lin_hpl_row   the products J_c^T W J_c, J_c^T r, J_p^T W J_p, J_p^T r, J_c^T W J_p of either form.
// The classic pair of kernels, the fused linearise-in-Schur kernels and the back-substitution that forms H_pl again all call THESE
// functions, so the bits they have to share are shared by construction.  All FP64, compiled with -ffp-contract=off: a row sum is
// a0 b0 + a1 b1 for two rows and (a0 b0 + a1 b1) + a2 b2 for three, in that order.
#pragma once
#include <string.h>

#include "ba_types.h"

#ifndef CS_HD_MEMBER      // (CS_HD is `static inline` on the host, which a member function cannot be)
#if defined(__HIPCC__)
#define CS_HD_MEMBER __host__ __device__ __forceinline__
#else
#define CS_HD_MEMBER inline
#endif
#endif

namespace cs {

// rho, rho' of a projection edge's squared error (cs_robust.h): Huber-or-none from the delta alone, any kernel through the kind array
// (off: the class's kernels are switched off in place, cs_ba_set_kernels_enabled -- the RK_NONE branch, whatever the records hold)
CS_HD void proj_rho(const int* rk, size_t k, double delta, bool off, double e, double& rho0, double& rho1) {
  if (off) { rho0 = e; rho1 = 1.0; }
  else if (rk) robust_rho(rk[k], delta, e, rho0, rho1);
  else huber_rho(e, delta, rho0, rho1);
}
// An edge's level (OptimizableGraph::Edge::setLevel, core/optimizable_graph.h) rides in the SIGN BIT of its kernel-width record (pm_huber /
// cm_huber, widths are >= +0.0 otherwise): the kernels already read that record, so a graph without a level-1 edge reads nothing more and computes
// what it always did.  A level-1 edge is outside the active set: every site that evaluates an edge SELECTS zeros for it before the projection is
// used -- its point may sit at depth 0 or behind the camera, and 0 * inf must not reach a sum.
CS_HD bool edge_off(double width_record) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __double2hiint(width_record) < 0;
#else
  long long bits;
  memcpy(&bits, &width_record, sizeof bits);
  return bits < 0;
#endif
}
// The select of the linearising sites (proj_linearize): a level-1 edge's camera-frame point is replaced by (0, 0, 1) BEFORE it is
// projected, so its error and Jacobians are finite whatever the estimates are, and its rho' and chi2 are then selected to zero -- Omega and -Omega e are
// weighted by an exact 0 and every product the callers form from the ProjLinT is an exact (signed) zero.  Selects, not an early return with a zeroed
// ProjLinT: a second exit made the compiler keep the camera-frame point in scratch memory in every kernel that inlines these functions, and zeroing the
// error as well cost ba_lin_schur_kernel<1, true> and <5, false> a wavefront of occupancy (169 and 257 registers against the steps at 168 and 256).
CS_HD void level1_point(bool off, double* pc) { if (off) { pc[0] = 0.0; pc[1] = 0.0; pc[2] = 1.0; } }

// ---- one of a BaView's two tables of projection edges ---------------------------------------------------------------------------------
// Every kernel that evaluates a projection edge has a STEREO instantiation, launched for graphs that hold a stereo edge (v.pm_kind != nullptr);
// a graph without one runs the STEREO = false code, which never names the stereo arrays (they are nullptr there).
struct PointMajor {};
struct CameraMajor {};
template <bool STEREO>
struct ProjTable {
  const double* cams; const double* points;
  const int* pt; const int* cam;            // cam: nullptr in the camera-major table (an edge's camera is the run it sits in)
  const double* uv;
  const double* info; const double* info_u; // 2 x 2 information: per edge, or the graph's one record
  const double* intr; const double* intr_u; // fx fy cx cy: likewise
  const double* width;                      // kernel width, the level in its sign
  const int* kind; const double* ur_;       // stereo graphs: 1 = stereo edge; u_right
  const double* sinfo; const double* sinfo_u;   // a stereo edge's record beyond the mono one: 3 x 3 information + bf, the edge's own or the graph's one
  const int* rk; int rk_off;
  CS_HD_MEMBER ProjTable(const BaView& v, PointMajor)
      : cams(v.cams), points(v.points), pt(v.pm_pt), cam(v.pm_cam), uv(v.pm_uv), info(v.pm_info), info_u(v.info_u), intr(v.pm_intr), intr_u(v.intr_u), width(v.pm_huber),
        kind(v.pm_kind), ur_(v.pm_ur), sinfo(v.pm_sinfo), sinfo_u(v.sinfo_u), rk(v.pm_rk), rk_off(v.rk_off) {}
  CS_HD_MEMBER ProjTable(const BaView& v, CameraMajor)
      : cams(v.cams), points(v.points), pt(v.cm_pt), cam(nullptr), uv(v.cm_uv), info(v.cm_info), info_u(v.info_u), intr(v.cm_intr), intr_u(v.intr_u), width(v.cm_huber),
        kind(v.cm_kind), ur_(v.cm_ur), sinfo(v.cm_sinfo), sinfo_u(v.sinfo_u), rk(v.cm_rk), rk_off(v.rk_off) {}
  CS_HD_MEMBER const double* point_of(size_t k) const { return points + 3 * (size_t)pt[k]; }
  CS_HD_MEMBER const double* uv_of(size_t k) const { return uv + 2 * k; }
  CS_HD_MEMBER const double* info_of(size_t k) const { return info_u ? info_u : info + 4 * k; }
  CS_HD_MEMBER const double* intr_of(size_t k) const { return intr_u ? intr_u : intr + 4 * k; }
  CS_HD_MEMBER double info_at(size_t k, int q) const { return info_u ? info_u[q] : info[4 * k + q]; }     // (a load, for the sites that prefetch a record)
  CS_HD_MEMBER double intr_at(size_t k, int q) const { return intr_u ? intr_u[q] : intr[4 * k + q]; }
  CS_HD_MEMBER bool stereo(size_t k) const { if constexpr (STEREO) return kind[k] != 0; else return false; }
  CS_HD_MEMBER int kind_of(size_t k) const { if constexpr (STEREO) return kind[k]; else return 0; }
  CS_HD_MEMBER double ur(size_t k) const { if constexpr (STEREO) return ur_[k]; else return 0.0; }
  CS_HD_MEMBER const double* srec(size_t k) const { if constexpr (STEREO) return sinfo_u ? sinfo_u : sinfo + 10 * k; else return nullptr; }
  CS_HD_MEMBER bool kernels_off(bool stereo_edge) const { return (rk_off & (stereo_edge ? RK_OFF_STEREO : RK_OFF_MONO)) != 0; }
};

// e^T Omega e, row sums left to right
CS_HD double quad2(const double* e, const double* info) { return e[0] * (info[0] * e[0] + info[1] * e[1]) + e[1] * (info[2] * e[0] + info[3] * e[1]); }
CS_HD double quad3(const double* e, const double* info) {
  return e[0] * ((info[0] * e[0] + info[1] * e[1]) + info[2] * e[2]) + e[1] * ((info[3] * e[0] + info[4] * e[1]) + info[5] * e[2]) + e[2] * ((info[6] * e[0] + info[7] * e[1]) + info[8] * e[2]);
}
// The plain (un-robustified) chi2 of edge k of the point-major table at the current estimates, pc = the point in the camera frame.  A stereo
// edge's error has the reference's single-precision invz / bf (stereo_proj_error, cs_se3.h).  The edge's level is the caller's business.
template <bool STEREO>
CS_HD double proj_edge_chi(const ProjTable<STEREO>& E, size_t k, double* pc) {
  const Pose T = pose_load(E.cams + 7 * E.cam[k]);
  const double* intr = E.intr_of(k);
  if (E.stereo(k)) {
    double e3[3];
    const double* srec = E.srec(k);
    stereo_proj_error(T, E.point_of(k), E.uv_of(k), E.ur(k), intr, srec[9], e3, pc);
    return quad3(e3, srec);
  }
  double e[2];
  proj_error(T, E.point_of(k), E.uv_of(k), intr, e, pc);
  return quad2(e, E.info_of(k));
}

// ---- linearisation --------------------------------------------------------------------------------------------------------------------
template <int ROWS>
struct ProjLinT {
  double e[ROWS];          // error (u, v; a stereo graph's third row: u_right)
  double Jp[3 * ROWS];     // ROWS x 3  d e / d point
  double Jc[6 * ROWS];     // ROWS x 6  d e / d camera (rot 0..2, trans 3..5)
  double Wm[ROWS * ROWS];  // rho' * Omega
  double r[ROWS];          // -rho' * Omega e
  double chi;              // rho0
};
// what both kinds of edge and both forms share: rows 0 and 1 of the camera Jacobian, which both linearizeOplus write alike
// (types_six_dof_expmap.cpp:171-183, :259-271)
CS_HD void proj_cam_rows01(double x, double y, double z, double fx, double fy, double* Jc) {
  const double z_2 = z * z;
  Jc[0] = x * y / z_2 * fx; Jc[1] = -(1 + (x * x / z_2)) * fx; Jc[2] = y / z * fx; Jc[3] = -1. / z * fx; Jc[4] = 0; Jc[5] = x / z_2 * fx;
  Jc[6] = (1 + y * y / z_2) * fy; Jc[7] = -x * y / z_2 * fy; Jc[8] = -x / z * fy; Jc[9] = 0; Jc[10] = -1. / z * fy; Jc[11] = y / z_2 * fy;
}
// a mono edge's error (proj_error's arithmetic on the camera-frame point) and its point Jacobian -1/z * tmp * R (:150-169)
CS_HD void proj_mono_rows(double x, double y, double z, const double* uv, const double* intr, const double* R, double* e, double* jp) {
  const double fx = intr[0], fy = intr[1];
  e[0] = uv[0] - (x / z * fx + intr[2]);
  e[1] = uv[1] - (y / z * fy + intr[3]);
  const double tmp[6] = {fx, 0, -x / z * fx, 0, fy, -y / z * fy};
#pragma unroll
  for (int i = 0; i < 2; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double s = 0;
#pragma unroll
      for (int q = 0; q < 3; q++) s += (-1. / z * tmp[3 * i + q]) * R[3 * q + j];
      jp[3 * i + j] = s;
    }
}
// The 2-row form: a mono edge of a graph without a stereo edge (stereo, ur, srec: not read).  R = the rotation matrix of T.
CS_HD void proj_linearize(const Pose& T, const double* R, const double* X, const double* uv, const double* info, const double* intr, double huber, const int* rk, size_t k, int rk_off,
                          bool, double, const double*, ProjLinT<2>& L) {
  double pc[3];
  pose_map(T, X, pc);
  const bool off = edge_off(huber);
  level1_point(off, pc);
  proj_mono_rows(pc[0], pc[1], pc[2], uv, intr, R, L.e, L.Jp);
  proj_cam_rows01(pc[0], pc[1], pc[2], intr[0], intr[1], L.Jc);
  const double c = quad2(L.e, info);
  double rho1;
  proj_rho(rk, k, huber, (rk_off & RK_OFF_MONO) != 0, c, L.chi, rho1);
  if (off) { rho1 = 0.0; L.chi = 0.0; }
#pragma unroll
  for (int i = 0; i < 4; i++) L.Wm[i] = rho1 * info[i];
  L.r[0] = -(info[0] * L.e[0] + info[1] * L.e[1]) * rho1;
  L.r[1] = -(info[2] * L.e[0] + info[3] * L.e[1]) * rho1;
}
// The 3-row form: either kind of edge of a stereo graph, from the fields both kinds have (uv, info: the mono edge's 2 x 2; intr) and the
// stereo ones (u_right; srec = 3 x 3 information, bf).  A lane branches on its edge's kind while it linearises; both kinds then share one set of
// 3-row products -- a mono edge fills rows 0 and 1 and leaves row 2 (error, Jacobians, information) zero, which adds exact zeros to the sums the
// 2-row form makes.  What the two kinds share is formed once, in front of the per-lane branch: the camera-frame point and rows 0 and 1 of
// the camera Jacobian.  Stereo: the error with its single-precision invz / bf (cs_se3.h), the point Jacobian in ITS form (:247-257:
// -fx R(0,j) / z + fx x R(2,j) / z^2, not the mono edge's -1/z * tmp * R), row 2 of both Jacobians (:255-257, :273-278), all double.  Mono: the
// 2-row form's rows, row 2 zero.
CS_HD void proj_linearize(const Pose& T, const double* R, const double* X, const double* uv, const double* info, const double* intr, double huber, const int* rk, size_t k, int rk_off,
                          bool stereo, double ur, const double* srec, ProjLinT<3>& L) {
  double pc[3];
  pose_map(T, X, pc);
  const bool off = edge_off(huber);
  level1_point(off, pc);
  const double x = pc[0], y = pc[1], z = pc[2], z_2 = z * z, fx = intr[0], fy = intr[1];
  proj_cam_rows01(x, y, z, fx, fy, L.Jc);
  double e[3], W[9], jp[9], jc2[6];
  if (stereo) {
    const double bf = srec[9];
    stereo_cam_project_error(pc, uv, ur, intr, bf, e);
#pragma unroll
    for (int j = 0; j < 3; j++) {
      jp[j] = -fx * R[j] / z + fx * x * R[6 + j] / z_2;
      jp[3 + j] = -fy * R[3 + j] / z + fy * y * R[6 + j] / z_2;
      jp[6 + j] = jp[j] - bf * R[6 + j] / z_2;
    }
    jc2[0] = L.Jc[0] - bf * y / z_2; jc2[1] = L.Jc[1] + bf * x / z_2; jc2[2] = L.Jc[2]; jc2[3] = L.Jc[3]; jc2[4] = 0; jc2[5] = L.Jc[5] - bf / z_2;
#pragma unroll
    for (int i = 0; i < 9; i++) W[i] = srec[i];
  } else {
    proj_mono_rows(x, y, z, uv, intr, R, e, jp);
    e[2] = 0;
    jp[6] = 0; jp[7] = 0; jp[8] = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) jc2[i] = 0;
    W[0] = info[0]; W[1] = info[1]; W[2] = 0; W[3] = info[2]; W[4] = info[3]; W[5] = 0; W[6] = 0; W[7] = 0; W[8] = 0;
  }
#pragma unroll
  for (int i = 0; i < 3; i++) L.e[i] = e[i];
#pragma unroll
  for (int i = 0; i < 9; i++) L.Jp[i] = jp[i];
#pragma unroll
  for (int i = 0; i < 6; i++) L.Jc[12 + i] = jc2[i];
  // (a mono edge: the zeros of row / column 2 add nothing -- e^T Omega e, rho' Omega and -rho' Omega e are the 2 x 2 ones)
  const double c = quad3(L.e, W);
  double rho1;
  proj_rho(rk, k, huber, (rk_off & (stereo ? RK_OFF_STEREO : RK_OFF_MONO)) != 0, c, L.chi, rho1);
  if (off) { rho1 = 0.0; L.chi = 0.0; }
#pragma unroll
  for (int i = 0; i < 9; i++) L.Wm[i] = rho1 * W[i];
#pragma unroll
  for (int i = 0; i < 3; i++) L.r[i] = -((W[3 * i] * L.e[0] + W[3 * i + 1] * L.e[1]) + W[3 * i + 2] * L.e[2]) * rho1;
}
// edge k of a table, with the camera (pose T, rotation matrix R) and the point X its caller already holds
template <bool STEREO>
CS_HD void proj_linearize(const ProjTable<STEREO>& E, size_t k, const Pose& T, const double* R, const double* X, ProjLinT<STEREO ? 3 : 2>& L) {
  proj_linearize(T, R, X, E.uv_of(k), E.info_of(k), E.intr_of(k), E.width[k], E.rk, k, E.rk_off, E.stereo(k), E.ur(k), E.srec(k), L);
}

// ---- the products of constructQuadraticForm -------------------------------------------------------------------------------------------
// sum over the rows of a (stride sa) times b (stride sb), left to right
template <int ROWS>
CS_HD double row_sum(const double* a, int sa, const double* b, int sb) {
  const double s = a[0] * b[0] + a[sa] * b[sb];
  if constexpr (ROWS == 3) return s + a[2 * sa] * b[2 * sb];
  else return s;
}
template <int ROWS>
CS_HD void lin_cam_terms(const ProjLinT<ROWS>& L, double* A21, double* b6) {   // A_ii (upper triangle) += J_c^T W J_c, b_i += J_c^T r
  int q = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double jw[ROWS];   // row i of J_c^T W
#pragma unroll
    for (int d = 0; d < ROWS; d++) jw[d] = row_sum<ROWS>(L.Jc + i, 6, L.Wm + d, ROWS);
#pragma unroll
    for (int j = i; j < 6; j++) A21[q++] += row_sum<ROWS>(jw, 1, L.Jc + j, 6);
    b6[i] += row_sum<ROWS>(L.Jc + i, 6, L.r, 1);
  }
}
template <int ROWS>
CS_HD void lin_point_terms(const ProjLinT<ROWS>& L, double* H6, double* b3) {   // J_p^T W J_p (upper triangle), J_p^T r
  double pw[3 * ROWS];  // J_p^T W (3 x ROWS)
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int d = 0; d < ROWS; d++) pw[ROWS * i + d] = row_sum<ROWS>(L.Jp + i, 3, L.Wm + d, ROWS);
  int q = 0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = i; j < 3; j++) H6[q++] = row_sum<ROWS>(pw + ROWS * i, 1, L.Jp + j, 3);
    b3[i] = row_sum<ROWS>(L.Jp + i, 3, L.r, 1);
  }
}
template <int ROWS>
CS_HD void lin_hpl_row(const ProjLinT<ROWS>& L, int i, double* h3) {   // row i of H_pl = J_c^T W J_p (6 x 3), J_c^T W formed once per row
  double jw[ROWS];
#pragma unroll
  for (int d = 0; d < ROWS; d++) jw[d] = row_sum<ROWS>(L.Jc + i, 6, L.Wm + d, ROWS);
#pragma unroll
  for (int j = 0; j < 3; j++) h3[j] = row_sum<ROWS>(jw, 1, L.Jp + j, 3);
}
// the whole block, or zeros where one of the edge's vertices is fixed; out(i, j) = the destination of entry (i, j)
template <int ROWS, class Out>
CS_HD void lin_hpl(const ProjLinT<ROWS>& L, bool both_free, Out out) {
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double h3[3];
    lin_hpl_row(L, i, h3);
#pragma unroll
    for (int j = 0; j < 3; j++) out(i, j) = both_free ? h3[j] : 0.0;
  }
}

}  // namespace cs
