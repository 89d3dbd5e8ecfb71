// cs_triangulate.h -- two-view triangulation of the matches between the current keyframe and its neighbours, for host and device
// (include/cubeslam_hip.h: cs_triangulate_*).
//
// What an ORB-SLAM2-derived local mapper runs on every keyframe between its matcher and local bundle adjustment:
// LocalMapping::CreateNewMapPoints with KeyFrame::UnprojectStereo, and MapPoint::UpdateNormalAndDepth for the two observations a new
// point has, NOT IN THE REFERENCE.  ORB-SLAM2 computes this in float32 with OpenCV's SVD; this statement is FP64.  Keyframe 1 is the
// current keyframe, keyframe 2 the neighbour.  The statement:
//
//   per pair       Tcw_i: 7 doubles x y z qx qy qz qw (SE3Quat::toVector); R_i = the rotation matrix of q_i / |q_i|, t_i = x y z;
//                  cam_i = fx fy cx cy bf b (b: the stereo baseline in metres).  Camera centres O_i = -R_i^T t_i,
//                  baseline = |O2 - O1|.  median_depth2 > 0: the monocular rule, the pair is not run when
//                  baseline / median_depth2 < min_baseline_ratio; median_depth2 <= 0: the stereo rule, not run when baseline < b2.
//                  Every match of a pair that is not run has status PAIR_NOT_RUN.  (triangulate_pair_record, once per pair.)
//   per match      for each side i: u_i v_i ur_i depth_i sigma2_i scale_i; ur_i < 0: no right-image coordinate, depth_i is not read.
//                  The first test that fails gives the status.
//   1 rays         xn_i = ((u_i - cx_i) / fx_i, (v_i - cy_i) / fy_i, 1), ray_i = R_i^T xn_i, cosRays = ray1 . ray2 / (|ray1| |ray2|);
//                  stereo_i = ur_i >= 0; cosS1 = cosS2 = cosRays + 1; if stereo1: cosS1 = (d1^2 - b1^2 / 4) / (d1^2 + b1^2 / 4), which
//                  is cos(2 atan2(b / 2, d)) without libm; ELSE if stereo2: the same for side 2.  The else is ORB-SLAM2's own: when
//                  side 1 is stereo, side 2's value stays cosRays + 1 even if side 2 is stereo too.  cosS = min(cosS1, cosS2).
//   2 route        cosRays < cosS && cosRays > 0 && (stereo1 || stereo2 || cosRays < max_cos_parallax): TRIANGULATED.  The 4 x 4 A has
//                  the rows xn1.x T1[2] - T1[0], xn1.y T1[2] - T1[1], xn2.x T2[2] - T2[0], xn2.y T2[2] - T2[1], T = [R | t]; the
//                  homogeneous point is the right singular vector of its smallest singular value by a ONE-SIDED (Hestenes) Jacobi on
//                  the columns of A: pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), 8 sweeps; for columns p, q: alpha = |a_p|^2,
//                  beta = |a_q|^2, gamma = a_p . a_q, zeta = (beta - alpha) / (2 gamma), t = sign(zeta) / (|zeta| + sqrt(zeta^2 + 1)),
//                  c = 1 / sqrt(t^2 + 1), s = t c, (a_p, a_q) <- (c a_p - s a_q, s a_p + c a_q), the same on the columns of V (which
//                  starts as the identity); gamma exactly 0: the identity, by selects, no lane branches.  The vector is V's column of
//                  the smallest |a_k|^2, the first of equals.  (A^T A is never formed: that would square the condition number.)
//                  w == 0 or a coordinate of xyz / w not finite: W_ZERO.  X = xyz / w; the vector's sign cancels.
//                  Otherwise stereo1 && cosS1 < cosS2: X = R1^T ((u1 - cx1) d1 / fx1, (v1 - cy1) d1 / fy1, d1) + O1, STEREO1.
//                  Otherwise stereo2 && cosS2 < cosS1: the same from camera 2, STEREO2.  Otherwise LOW_PARALLAX, route NONE.
//   3 depths       z1 = (R1 X + t1).z <= 0: DEPTH1; z2 <= 0: DEPTH2.
//   4 reprojection side 1, then side 2: u = fx x / z + cx, v = fy y / z + cy; mono: (u - u_i)^2 + (v - v_i)^2 > chi2_mono sigma2_i;
//                  stereo: + (u - bf / z - ur_i)^2, against chi2_stereo sigma2_i: REPROJ1 / REPROJ2.  A NaN error is a rejection.
//   5 scale        dist_i = |X - O_i|; either one zero: ZERO_DIST.  ratioDist = dist2 / dist1, ratioOctave = scale1 / scale2;
//                  ratioDist ratio_factor < ratioOctave || ratioDist > ratioOctave ratio_factor: SCALE.
//   6 accepted     OK: normal = ((X - O1) / dist1 + (X - O2) / dist2) / 2, NOT renormalised (as ORB-SLAM2 leaves it),
//                  max_distance = dist1 scale1, min_distance = max_distance / scale_range.
//   outputs        X, normal, min_distance, max_distance, status, route; a match that is not accepted still hands out X when one was
//                  computed (status DEPTH1 and later), and zeros otherwise.
//
// Every sum is taken left to right as written below.  triangulate_pair_serial runs one pair match after match
// (tools/hostonly/triangulate_host_check.cpp); triangulate_kernels.hip runs one match per lane from the same routines.
// FP64, -ffp-contract=off.
#pragma once
#include <float.h>
#include <math.h>

#include "cs_dense_lm.h"      // CS_HD, CS_UNROLL, CS_NOUNROLL
#include "cs_se3.h"           // quat_rotmat

namespace cs {

// A match as the host packs it: 12 doubles = 96 bytes   [0..5] u1 v1 ur1 depth1 sigma2_1 scale1   [6..11] the same of side 2
// What a match hands out: 8 doubles                      [0..2] X   [3..5] normal   [6] min_distance   [7] max_distance
enum { TRI_MATCH_DOUBLES = 12, TRI_OUT_DOUBLES = 8, TRI_JACOBI_SWEEPS = 8, TRI_CAM_DOUBLES = 6 };

// (the values of cs_triangulate_status / cs_triangulate_route of include/cubeslam_hip.h; triangulate_host.cpp asserts that they agree)
enum { TRI_OK = 0, TRI_PAIR_NOT_RUN = 1, TRI_LOW_PARALLAX = 2, TRI_W_ZERO = 3, TRI_DEPTH1 = 4, TRI_DEPTH2 = 5, TRI_REPROJ1 = 6, TRI_REPROJ2 = 7,
       TRI_ZERO_DIST = 8, TRI_SCALE = 9 };
enum { TRI_ROUTE_NONE = 0, TRI_ROUTE_TRIANGULATED = 1, TRI_ROUTE_STEREO1 = 2, TRI_ROUTE_STEREO2 = 3 };

struct TriParams {
  double min_baseline_ratio, max_cos_parallax, chi2_mono, chi2_stereo, ratio_factor, scale_range;
};

// What is the same for every match of a pair: 44 doubles, made once per pair by triangulate_pair_record.  R row-major.
struct TriPair {
  double R1[9], t1[3], O1[3], cam1[TRI_CAM_DOUBLES];
  double R2[9], t2[3], O2[3], cam2[TRI_CAM_DOUBLES];
  double ran, baseline;      // ran: 1.0 or 0.0
};

struct TriMatchOut {
  double X[3], normal[3], min_distance, max_distance;
  double cosRays, cosS1, cosS2;      // the inspection form's
  int status, route;
};

CS_HD bool tri_finite(double x) { return fabs(x) <= DBL_MAX; }      // (a NaN compares false)

// R (row-major) of q / |q|, t and O = -R^T t from 7 doubles x y z qx qy qz qw
CS_HD void triangulate_camera(const double* Tcw, double* R, double* t, double* O) {
  const double n = sqrt(Tcw[3] * Tcw[3] + Tcw[4] * Tcw[4] + Tcw[5] * Tcw[5] + Tcw[6] * Tcw[6]);
  quat_rotmat(Tcw[6] / n, Tcw[3] / n, Tcw[4] / n, Tcw[5] / n, R);
  CS_UNROLL
  for (int i = 0; i < 3; i++) t[i] = Tcw[i];
  CS_UNROLL
  for (int i = 0; i < 3; i++) O[i] = -(R[i] * t[0] + R[3 + i] * t[1] + R[6 + i] * t[2]);
}

CS_HD void triangulate_pair_record(const double* Tcw1, const double* Tcw2, const double* cam1, const double* cam2, double median_depth2, double min_baseline_ratio,
                                   TriPair& P) {
  triangulate_camera(Tcw1, P.R1, P.t1, P.O1);
  triangulate_camera(Tcw2, P.R2, P.t2, P.O2);
  CS_UNROLL
  for (int k = 0; k < TRI_CAM_DOUBLES; k++) { P.cam1[k] = cam1[k]; P.cam2[k] = cam2[k]; }
  const double d0 = P.O2[0] - P.O1[0], d1 = P.O2[1] - P.O1[1], d2 = P.O2[2] - P.O1[2];
  P.baseline = sqrt(d0 * d0 + d1 * d1 + d2 * d2);
  const bool skip = (median_depth2 > 0.0) ? (P.baseline / median_depth2 < min_baseline_ratio) : (P.baseline < cam2[5]);
  P.ran = skip ? 0.0 : 1.0;
}

// R^T x
CS_HD void tri_rotate_back(const double* R, const double* x, double* o) {
  CS_UNROLL
  for (int i = 0; i < 3; i++) o[i] = R[i] * x[0] + R[3 + i] * x[1] + R[6 + i] * x[2];
}

// R X + t
CS_HD void tri_to_camera(const double* R, const double* t, const double* X, double* o) {
  CS_UNROLL
  for (int i = 0; i < 3; i++) o[i] = (R[3 * i] * X[0] + R[3 * i + 1] * X[1] + R[3 * i + 2] * X[2]) + t[i];
}

CS_HD double tri_cos_stereo(double d, double b) {
  const double q = (b * b) * 0.25;
  return (d * d - q) / (d * d + q);
}

// One Hestenes rotation of the columns P, Q of a, accumulated into v.  P and Q are template arguments: every index is a constant, nothing
// is addressed, and a lane whose columns are already orthogonal rotates by the identity (c = 1, s = 0) instead of branching.
template <int P, int Q>
CS_HD void tri_jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
  const double alpha = a[0][P] * a[0][P] + a[1][P] * a[1][P] + a[2][P] * a[2][P] + a[3][P] * a[3][P];
  const double beta = a[0][Q] * a[0][Q] + a[1][Q] * a[1][Q] + a[2][Q] * a[2][Q] + a[3][Q] * a[3][Q];
  const double gamma = a[0][P] * a[0][Q] + a[1][P] * a[1][Q] + a[2][P] * a[2][Q] + a[3][P] * a[3][Q];
  const bool skip = (gamma == 0.0);
  const double zeta = (beta - alpha) / (skip ? 1.0 : 2.0 * gamma);
  const double r = 1.0 / (fabs(zeta) + sqrt(zeta * zeta + 1.0));      // (zeta^2 = inf: r = 0)
  const double t = skip ? 0.0 : (zeta < 0.0 ? -r : r);
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  CS_UNROLL
  for (int k = 0; k < 4; k++) {
    const double g = a[k][P], h = a[k][Q];
    a[k][P] = c * g - s * h;
    a[k][Q] = s * g + c * h;
  }
  CS_UNROLL
  for (int k = 0; k < 4; k++) {
    const double g = v[k][P], h = v[k][Q];
    v[k][P] = c * g - s * h;
    v[k][Q] = s * g + c * h;
  }
}

// The right singular vector of a's smallest singular value (a is used up)
CS_HD void tri_smallest_singular_vector(double (&a)[4][4], double* h4) {
  double v[4][4];
  CS_UNROLL
  for (int i = 0; i < 4; i++) {
    CS_UNROLL
    for (int j = 0; j < 4; j++) v[i][j] = (i == j) ? 1.0 : 0.0;
  }
  CS_NOUNROLL
  for (int sweep = 0; sweep < TRI_JACOBI_SWEEPS; sweep++) {
    tri_jacobi_rotate<0, 1>(a, v);
    tri_jacobi_rotate<0, 2>(a, v);
    tri_jacobi_rotate<0, 3>(a, v);
    tri_jacobi_rotate<1, 2>(a, v);
    tri_jacobi_rotate<1, 3>(a, v);
    tri_jacobi_rotate<2, 3>(a, v);
  }
  // the first of the columns with the smallest norm
  double best = a[0][0] * a[0][0] + a[1][0] * a[1][0] + a[2][0] * a[2][0] + a[3][0] * a[3][0];
  h4[0] = v[0][0]; h4[1] = v[1][0]; h4[2] = v[2][0]; h4[3] = v[3][0];
  CS_UNROLL
  for (int k = 1; k < 4; k++) {
    const double nk = a[0][k] * a[0][k] + a[1][k] * a[1][k] + a[2][k] * a[2][k] + a[3][k] * a[3][k];
    const bool down = nk < best;
    best = down ? nk : best;
    CS_UNROLL
    for (int i = 0; i < 4; i++) h4[i] = down ? v[i][k] : h4[i];
  }
}

// X = xyz / w.  false: W_ZERO (w == 0, or a coordinate that is not finite)
CS_HD bool triangulate_dehomogenize(const double* h4, double* X) {
  X[0] = h4[0] / h4[3]; X[1] = h4[1] / h4[3]; X[2] = h4[2] / h4[3];
  return h4[3] != 0.0 && tri_finite(X[0]) && tri_finite(X[1]) && tri_finite(X[2]);
}

// The linear triangulation of step 2.  false: W_ZERO
CS_HD bool triangulate_linear(const TriPair& P, const double* xn1, const double* xn2, double* X) {
  double a[4][4];
  CS_UNROLL
  for (int j = 0; j < 4; j++) {
    const double r10 = (j < 3) ? P.R1[j] : P.t1[0], r11 = (j < 3) ? P.R1[3 + j] : P.t1[1], r12 = (j < 3) ? P.R1[6 + j] : P.t1[2];
    const double r20 = (j < 3) ? P.R2[j] : P.t2[0], r21 = (j < 3) ? P.R2[3 + j] : P.t2[1], r22 = (j < 3) ? P.R2[6 + j] : P.t2[2];
    a[0][j] = xn1[0] * r12 - r10;
    a[1][j] = xn1[1] * r12 - r11;
    a[2][j] = xn2[0] * r22 - r20;
    a[3][j] = xn2[1] * r22 - r21;
  }
  double h4[4];
  tri_smallest_singular_vector(a, h4);
  return triangulate_dehomogenize(h4, X);
}

// KeyFrame::UnprojectStereo
CS_HD void triangulate_unproject(const double* R, const double* O, const double* cam, double u, double v, double d, double* X) {
  const double x[3] = {(u - cam[2]) * d / cam[0], (v - cam[3]) * d / cam[1], d};
  double w[3];
  tri_rotate_back(R, x, w);
  CS_UNROLL
  for (int i = 0; i < 3; i++) X[i] = w[i] + O[i];
}

// Step 4 for one side: pc = R X + t with pc[2] > 0, kp = u v ur ... sigma2 at [4].  true: rejected
CS_HD bool triangulate_reprojection_fails(const double* pc, const double* cam, const double* kp, bool stereo, const TriParams& prm) {
  const double u = cam[0] * pc[0] / pc[2] + cam[2];
  const double v = cam[1] * pc[1] / pc[2] + cam[3];
  const double ex = u - kp[0], ey = v - kp[1];
  const double exr = (u - cam[4] / pc[2]) - kp[2];
  const double e2 = ex * ex + ey * ey;
  const double e = stereo ? e2 + exr * exr : e2;
  const double th = (stereo ? prm.chi2_stereo : prm.chi2_mono) * kp[4];
  return !(e <= th);      // (a NaN is a rejection)
}

// Steps 5 and 6 at the point o.X: ZERO_DIST, SCALE, or OK with normal and distances filled in
CS_HD int triangulate_scale_stage(const TriPair& P, const TriParams& prm, double scale1, double scale2, TriMatchOut& o) {
  const double n1[3] = {o.X[0] - P.O1[0], o.X[1] - P.O1[1], o.X[2] - P.O1[2]};
  const double n2[3] = {o.X[0] - P.O2[0], o.X[1] - P.O2[1], o.X[2] - P.O2[2]};
  const double dist1 = sqrt(n1[0] * n1[0] + n1[1] * n1[1] + n1[2] * n1[2]);
  const double dist2 = sqrt(n2[0] * n2[0] + n2[1] * n2[1] + n2[2] * n2[2]);
  if (dist1 == 0.0 || dist2 == 0.0) return TRI_ZERO_DIST;
  const double ratioDist = dist2 / dist1;
  const double ratioOctave = scale1 / scale2;
  if (ratioDist * prm.ratio_factor < ratioOctave || ratioDist > ratioOctave * prm.ratio_factor) return TRI_SCALE;
  CS_UNROLL
  for (int i = 0; i < 3; i++) o.normal[i] = (n1[i] / dist1 + n2[i] / dist2) / 2.0;
  o.max_distance = dist1 * scale1;
  o.min_distance = o.max_distance / prm.scale_range;
  return TRI_OK;
}

// One match m (TRI_MATCH_DOUBLES) of the pair P
CS_HD void triangulate_match(const TriPair& P, const TriParams& prm, const double* m, TriMatchOut& o) {
  CS_UNROLL
  for (int i = 0; i < 3; i++) { o.X[i] = 0.0; o.normal[i] = 0.0; }
  o.min_distance = 0.0; o.max_distance = 0.0;
  o.cosRays = 0.0; o.cosS1 = 0.0; o.cosS2 = 0.0;
  o.route = TRI_ROUTE_NONE;
  o.status = TRI_PAIR_NOT_RUN;
  if (P.ran == 0.0) return;
  const double* k1 = m;
  const double* k2 = m + 6;
  // ---- 1 rays and parallax
  const double xn1[3] = {(k1[0] - P.cam1[2]) / P.cam1[0], (k1[1] - P.cam1[3]) / P.cam1[1], 1.0};
  const double xn2[3] = {(k2[0] - P.cam2[2]) / P.cam2[0], (k2[1] - P.cam2[3]) / P.cam2[1], 1.0};
  double ray1[3], ray2[3];
  tri_rotate_back(P.R1, xn1, ray1);
  tri_rotate_back(P.R2, xn2, ray2);
  const double dot = ray1[0] * ray2[0] + ray1[1] * ray2[1] + ray1[2] * ray2[2];
  const double len1 = sqrt(ray1[0] * ray1[0] + ray1[1] * ray1[1] + ray1[2] * ray1[2]);
  const double len2 = sqrt(ray2[0] * ray2[0] + ray2[1] * ray2[1] + ray2[2] * ray2[2]);
  const double cosRays = dot / (len1 * len2);
  const bool stereo1 = k1[2] >= 0.0, stereo2 = k2[2] >= 0.0;
  double cosS1 = cosRays + 1.0, cosS2 = cosRays + 1.0;
  if (stereo1) cosS1 = tri_cos_stereo(k1[3], P.cam1[5]);
  else if (stereo2) cosS2 = tri_cos_stereo(k2[3], P.cam2[5]);      // (else: ORB-SLAM2's own, see the statement)
  const double cosS = cosS2 < cosS1 ? cosS2 : cosS1;
  o.cosRays = cosRays; o.cosS1 = cosS1; o.cosS2 = cosS2;
  // ---- 2 route
  if (cosRays < cosS && cosRays > 0.0 && (stereo1 || stereo2 || cosRays < prm.max_cos_parallax)) {
    o.route = TRI_ROUTE_TRIANGULATED;
    double X[3];
    if (!triangulate_linear(P, xn1, xn2, X)) { o.status = TRI_W_ZERO; return; }
    o.X[0] = X[0]; o.X[1] = X[1]; o.X[2] = X[2];
  } else if (stereo1 && cosS1 < cosS2) {
    o.route = TRI_ROUTE_STEREO1;
    triangulate_unproject(P.R1, P.O1, P.cam1, k1[0], k1[1], k1[3], o.X);
  } else if (stereo2 && cosS2 < cosS1) {
    o.route = TRI_ROUTE_STEREO2;
    triangulate_unproject(P.R2, P.O2, P.cam2, k2[0], k2[1], k2[3], o.X);
  } else {
    o.status = TRI_LOW_PARALLAX;
    return;
  }
  // ---- 3 depths
  double pc1[3], pc2[3];
  tri_to_camera(P.R1, P.t1, o.X, pc1);
  tri_to_camera(P.R2, P.t2, o.X, pc2);
  if (!(pc1[2] > 0.0)) { o.status = TRI_DEPTH1; return; }
  if (!(pc2[2] > 0.0)) { o.status = TRI_DEPTH2; return; }
  // ---- 4 reprojection
  if (triangulate_reprojection_fails(pc1, P.cam1, k1, stereo1, prm)) { o.status = TRI_REPROJ1; return; }
  if (triangulate_reprojection_fails(pc2, P.cam2, k2, stereo2, prm)) { o.status = TRI_REPROJ2; return; }
  // ---- 5 scale consistency, 6 accepted
  o.status = triangulate_scale_stage(P, prm, k1[5], k2[5], o);
}

// A result as the 8 doubles a match hands out
CS_HD void triangulate_store(const TriMatchOut& o, double* out8) {
  CS_UNROLL
  for (int i = 0; i < 3; i++) { out8[i] = o.X[i]; out8[3 + i] = o.normal[i]; }
  out8[6] = o.min_distance;
  out8[7] = o.max_distance;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// One pair, match after match.  rec: the pair's n packed matches; out8: n x 8; cos3: n x 3 (cosRays cosS1 cosS2) or null.
// -> the number of accepted matches
static inline int triangulate_pair_serial(const TriPair& P, const TriParams& prm, const double* rec, int n, double* out8, unsigned char* status, unsigned char* route, double* cos3) {
  int n_accepted = 0;
  for (int i = 0; i < n; i++) {
    TriMatchOut o;
    triangulate_match(P, prm, rec + (size_t)i * TRI_MATCH_DOUBLES, o);
    triangulate_store(o, out8 + (size_t)i * TRI_OUT_DOUBLES);
    status[i] = (unsigned char)o.status;
    route[i] = (unsigned char)o.route;
    if (cos3) { cos3[3 * (size_t)i] = o.cosRays; cos3[3 * (size_t)i + 1] = o.cosS1; cos3[3 * (size_t)i + 2] = o.cosS2; }
    n_accepted += o.status == TRI_OK ? 1 : 0;
  }
  return n_accepted;
}
#endif

}  // namespace cs
