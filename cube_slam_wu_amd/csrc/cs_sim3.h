// cs_sim3.h -- Sim(3) algebra of the g2o pose-graph path, for host and device.
//
// A branch-for-branch restatement of g2o's Sim3 (object_slam/Thirdparty/g2o/g2o/types/sim3.h:41-285): quaternion r, translation t, scale s,
// NONE of them renormalised anywhere -- a product's quaternion is the plain Hamilton product, exp's quaternion is Eigen's
// matrix-to-quaternion of a matrix that is orthogonal only to first order in its small-angle branch, log's rotation matrix is the
// unit-quaternion formula applied to whatever the quaternion is.  A state is 8 doubles in Sim3::operator[] order (sim3.h:232-257):
// qx qy qz qw tx ty tz s.  FP64 throughout, -ffp-contract=off; libm resolves to glibc on the host and to ocml on gfx950.
//
// KEPT, NOT FIXED (sim3.h:116 in exp, :192 in log): with |sigma| >= eps and a small rotation the coefficient of Omega^2 is
//   B = ((0.5 sigma^2 - sigma + 1) s) / sigma^3
// which grows like 1 / sigma^3 where the series of the consistent branches tends to 1/6.  In log it makes W = A Omega + B Omega^2 + C I
// nearly rank one as soon as an error has |log s| >= 1e-5 and a rotation under ~4.5e-3 rad (d > 1 - 1e-5): a free-scale graph close to
// convergence goes through it, and so does this header.
#pragma once
#include "cs_se3.h"

namespace cs {

struct Sim3 {
  double qx, qy, qz, qw;
  double t[3];
  double s;
};

constexpr double SIM3_EPS = 0.00001;    // sim3.h:90, :158

CS_HD Sim3 sim3_load(const double* v) { Sim3 S; S.qx = v[0]; S.qy = v[1]; S.qz = v[2]; S.qw = v[3]; S.t[0] = v[4]; S.t[1] = v[5]; S.t[2] = v[6]; S.s = v[7]; return S; }
CS_HD void sim3_store(const Sim3& S, double* v) { v[0] = S.qx; v[1] = S.qy; v[2] = S.qz; v[3] = S.qw; v[4] = S.t[0]; v[5] = S.t[1]; v[6] = S.t[2]; v[7] = S.s; }
CS_HD Pose sim3_quat(const Sim3& S) { Pose p; p.t[0] = p.t[1] = p.t[2] = 0; p.qx = S.qx; p.qy = S.qy; p.qz = S.qz; p.qw = S.qw; return p; }

// sim3.h:140: s (r xyz) + t
CS_HD void sim3_map(const Sim3& S, const double* x, double* o) {
  double rx[3];
  pose_rotate(sim3_quat(S), x, rx);
  for (int i = 0; i < 3; i++) o[i] = S.s * rx[i] + S.t[i];
}
// sim3.h:259-265: r = r1 r2 (Eigen's quaternion product, not normalised), t = s1 (r1 t2) + t1, s = s1 s2
CS_HD Sim3 sim3_mul(const Sim3& a, const Sim3& b) {
  Sim3 r;
  r.qw = a.qw * b.qw - a.qx * b.qx - a.qy * b.qy - a.qz * b.qz;
  r.qx = a.qw * b.qx + a.qx * b.qw + a.qy * b.qz - a.qz * b.qy;
  r.qy = a.qw * b.qy + a.qy * b.qw + a.qz * b.qx - a.qx * b.qz;
  r.qz = a.qw * b.qz + a.qz * b.qw + a.qx * b.qy - a.qy * b.qx;
  double rt[3];
  pose_rotate(sim3_quat(a), b.t, rt);
  for (int i = 0; i < 3; i++) r.t[i] = a.s * rt[i] + a.t[i];
  r.s = a.s * b.s;
  return r;
}
// sim3.h:226-229: (r*, r* ((-1 / s) t), 1 / s)
CS_HD Sim3 sim3_inv(const Sim3& a) {
  Sim3 r;
  r.qx = -a.qx; r.qy = -a.qy; r.qz = -a.qz; r.qw = a.qw;
  const double f = -1. / a.s;
  const double nt[3] = {f * a.t[0], f * a.t[1], f * a.t[2]};
  pose_rotate(sim3_quat(r), nt, r.t);
  r.s = 1. / a.s;
  return r;
}

// Eigen's Quaterniond(Matrix3d) (quat_from_rotmat of cs_se3.h), its three largest-diagonal branches written out: no index is computed,
// so nothing lives in memory on the device
CS_HD void sim3_quat_from_rotmat(const double* R, Sim3& S) {
  double t = R[0] + R[4] + R[8];
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    S.qw = 0.5 * t;
    t = 0.5 / t;
    S.qx = (R[7] - R[5]) * t; S.qy = (R[2] - R[6]) * t; S.qz = (R[3] - R[1]) * t;
  } else if (!(R[4] > R[0]) && !(R[8] > R[0])) {        // i = 0
    t = sqrt(R[0] - R[4] - R[8] + 1.0);
    S.qx = 0.5 * t;
    t = 0.5 / t;
    S.qw = (R[7] - R[5]) * t; S.qy = (R[3] + R[1]) * t; S.qz = (R[6] + R[2]) * t;
  } else if (R[4] > R[0] && !(R[8] > R[4])) {           // i = 1
    t = sqrt(R[4] - R[8] - R[0] + 1.0);
    S.qy = 0.5 * t;
    t = 0.5 / t;
    S.qw = (R[2] - R[6]) * t; S.qz = (R[7] + R[5]) * t; S.qx = (R[1] + R[3]) * t;
  } else {                                              // i = 2
    t = sqrt(R[8] - R[0] - R[4] + 1.0);
    S.qz = 0.5 * t;
    t = 0.5 / t;
    S.qw = (R[3] - R[1]) * t; S.qx = (R[2] + R[6]) * t; S.qy = (R[5] + R[7]) * t;
  }
}

// the coefficients of W = A Omega + B Omega^2 + C I for |sigma| >= eps (sim3.h:111-131 and :184-204: the same expressions in exp and log)
CS_HD void sim3_abc_scaled(double sigma, double s, double theta, bool small_rot, double& A, double& B, double& C) {
  C = (s - 1) / sigma;
  if (small_rot) {
    const double sigma2 = sigma * sigma;
    A = ((sigma - 1) * s + 1) / sigma2;
    B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);      // the reference's expression (see the head of this file)
  } else {
    const double a = s * sin(theta), b = s * cos(theta);
    const double theta2 = theta * theta, sigma2 = sigma * sigma;
    const double c = theta2 + sigma2;
    A = (a * sigma + (1 - b) * theta) / (theta * c);
    B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
  }
}

// sim3.h:70-138: update = [omega, upsilon, sigma]
CS_HD Sim3 sim3_exp(const double* u) {
  const double sigma = u[6];
  const double theta = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  double Om[9], Om2[9], R[9];
  skew3(u, Om);
  mat3_mul(Om, Om, Om2);
  Sim3 S;
  S.s = exp(sigma);
  double A, B, C;
  const bool small_rot = theta < SIM3_EPS;
  if (fabs(sigma) < SIM3_EPS) {
    C = 1;
    if (small_rot) { A = 1. / 2.; B = 1. / 6.; }
    else {
      const double theta2 = theta * theta;
      A = (1 - cos(theta)) / (theta2);
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    sim3_abc_scaled(sigma, S.s, theta, small_rot, A, B, C);
  }
  if (small_rot) {
    for (int i = 0; i < 9; i++) R[i] = (((i % 4 == 0) ? 1.0 : 0.0) + Om[i]) + Om2[i];        // I + Omega + Omega^2 (not 1/2 Omega^2)
  } else {
    const double ra = sin(theta) / theta, rb = (1 - cos(theta)) / (theta * theta);
    for (int i = 0; i < 9; i++) R[i] = (((i % 4 == 0) ? 1.0 : 0.0) + ra * Om[i]) + rb * Om2[i];
  }
  sim3_quat_from_rotmat(R, S);            // Quaterniond(R): no normalisation
  double W[9];
  for (int i = 0; i < 9; i++) W[i] = (A * Om[i] + B * Om2[i]) + C * ((i % 4 == 0) ? 1.0 : 0.0);
  mat3_vec(W, u + 3, S.t);
  return S;
}

// W x = b by LU with partial pivoting (Eigen's PartialPivLU as Matrix3d::lu(): the first largest |entry| of the column at or below the
// diagonal is the pivot).  Rows are exchanged by value, so every index is a constant and nothing lives in memory on the device.
CS_HD void lu3_solve(const double* W, const double* b, double* x) {
  double r0[4] = {W[0], W[1], W[2], b[0]}, r1[4] = {W[3], W[4], W[5], b[1]}, r2[4] = {W[6], W[7], W[8], b[2]};
#define CS_SWAP_ROWS(ra, rb) for (int c_ = 0; c_ < 4; c_++) { const double t_ = ra[c_]; ra[c_] = rb[c_]; rb[c_] = t_; }
  {
    int p = 0; double best = fabs(r0[0]);
    if (fabs(r1[0]) > best) { best = fabs(r1[0]); p = 1; }
    if (fabs(r2[0]) > best) { p = 2; }
    if (p == 1) { CS_SWAP_ROWS(r0, r1) } else if (p == 2) { CS_SWAP_ROWS(r0, r2) }
  }
  const double l10 = r1[0] / r0[0], l20 = r2[0] / r0[0];
  for (int c = 1; c < 3; c++) { r1[c] -= l10 * r0[c]; r2[c] -= l20 * r0[c]; }
  if (fabs(r2[1]) > fabs(r1[1])) { CS_SWAP_ROWS(r1, r2) }
  // (the exchanged rows carry their multipliers with them: l10 / l20 are re-read from column 0)
  const double m1 = r1[0] / r0[0], m2 = r2[0] / r0[0];
  const double l21 = r2[1] / r1[1];
  r2[2] -= l21 * r1[2];
#undef CS_SWAP_ROWS
  // L y = P b
  const double y0 = r0[3];
  const double y1 = r1[3] - m1 * y0;
  const double y2 = (r2[3] - m2 * y0) - l21 * y1;
  // U x = y
  x[2] = y2 / r2[2];
  x[1] = (y1 - r1[2] * x[2]) / r1[1];
  x[0] = ((y0 - r0[1] * x[1]) - r0[2] * x[2]) / r0[0];
}

// sim3.h:144-223: res = [omega, upsilon, sigma]
CS_HD void sim3_log(const Sim3& S, double* res) {
  const double sigma = log(S.s);
  double R[9];
  pose_rotmat(sim3_quat(S), R);           // r.toRotationMatrix(): the unit-quaternion formula, whatever |r| is
  const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};     // deltaR (se3_ops.hpp:38-45)
  double omega[3], A, B, C;
  const bool small_rot = d > 1 - SIM3_EPS;
  double theta = 0;
  if (small_rot) {
    for (int i = 0; i < 3; i++) omega[i] = 0.5 * dR[i];
  } else {
    theta = acos(d);
    const double f = theta / (2 * sqrt(1 - d * d));
    for (int i = 0; i < 3; i++) omega[i] = f * dR[i];
  }
  if (fabs(sigma) < SIM3_EPS) {
    C = 1;
    if (small_rot) { A = 1. / 2.; B = 1. / 6.; }
    else {
      const double theta2 = theta * theta;
      A = (1 - cos(theta)) / (theta2);
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    sim3_abc_scaled(sigma, S.s, theta, small_rot, A, B, C);
  }
  double Om[9], Om2[9], W[9], ups[3];
  skew3(omega, Om);
  mat3_mul(Om, Om, Om2);
  for (int i = 0; i < 9; i++) W[i] = (A * Om[i] + B * Om2[i]) + C * ((i % 4 == 0) ? 1.0 : 0.0);
  lu3_solve(W, S.t, ups);
  for (int i = 0; i < 3; i++) { res[i] = omega[i]; res[i + 3] = ups[i]; }
  res[6] = sigma;
}

// VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69): update[6] = 0 under _fix_scale, then exp(update) * estimate
CS_HD Sim3 sim3_oplus(const Sim3& S, const double* u, bool fix_scale) {
  double v[7];
  for (int i = 0; i < 6; i++) v[i] = u[i];
  v[6] = fix_scale ? 0.0 : u[6];
  return sim3_mul(sim3_exp(v), S);
}
// EdgeSim3::computeError (types_seven_dof_expmap.h:106-114): log(C S_i S_j^-1)
CS_HD void sim3_edge_error(const Sim3& Cm, const Sim3& Si, const Sim3& Sj, double* e) {
  sim3_log(sim3_mul(sim3_mul(Cm, Si), sim3_inv(Sj)), e);
}

}  // namespace cs
