// ba_proj_edge_check.cpp -- the projection edge of the bundle adjustment (cube_slam_wu_amd/csrc/ba_proj_edge.h) on its own, without a GPU:
// a few thousand random edges -- points in front of, near and behind the camera; full 2 x 2 / 3 x 3 information; every robust kind, with the
// kind array and without it; widths including 0; the classes' kernels switched off; level-1 edges, some at depth exactly 0 -- against
//   (a) the 2-row linearisation and products as ba_kernels.hip spelled them INLINE before the header existed (in ba_lin_cam_kernel,
//       lin_pt_edge, ba_lin_schur_segment and backsub_lin_point: four copies of one text), restated HERE once: byte for byte;
//   (b) the 3-row linearisation (proj_linearize_any) and its products (lin3_cam_terms, lin3_point_terms, lin3_hpl) as they were: byte for byte;
//   (c) each other: a mono edge through the 3-row form gives the 2-row values (equal as doubles: only the sign of a zero may differ), and
//       every product of a level-1 edge is a zero;
// and the table view and proj_edge_chi against the expressions the three chi2 sites used.
// Built with -ffp-contract=off like the library.  tests/test_ba_proj_edge_cpu.py builds it with the host compiler and the sanitizers and runs it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../cube_slam_wu_amd/csrc/ba_proj_edge.h"

using namespace cs;

static long g_fail = 0;
static int g_edge = -1;
#define CHECK(cond) do { if (!(cond)) { if (g_fail++ < 20) std::printf("FAIL line %d, edge %d: %s\n", __LINE__, g_edge, #cond); } } while (0)
template <size_t N> static bool same_bytes(const double (&a)[N], const double (&b)[N]) { return std::memcmp(a, b, sizeof a) == 0; }
static bool same_bytes(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }
// equal as doubles (-0 == +0); two NaNs count as equal: a kernel kind at width 0 (Cauchy, pseudo-Huber, Tukey: 1 / delta^2) gives NaN weights in both forms
static bool same_value(double a, double b) { return a == b || (a != a && b != b); }
template <size_t N> static bool same_values(const double* a, const double (&b)[N]) { for (size_t i = 0; i < N; i++) if (!same_value(a[i], b[i])) return false; return true; }
template <size_t N> static bool all_zero(const double (&a)[N]) { for (size_t i = 0; i < N; i++) if (!(a[i] == 0.0)) return false; return true; }

// ---- the parent's words ----------------------------------------------------------------------------------------------------------------
static bool parent_edge_off(double width_record) { return std::signbit(width_record); }
static void parent_rho(const int* rk, int k, double delta, bool off, double e, double& rho0, double& rho1) {
  if (off) { rho0 = e; rho1 = 1.0; }
  else if (rk) robust_rho(rk[k], delta, e, rho0, rho1);
  else huber_rho(e, delta, rho0, rho1);
}
struct ProjLin { double e[2], Jp[6], Jc[12], Wm[4], r[2], chi; };
static void parent_linearize(const Pose& T, const double* R, const double* X, const double* uv, const double* info, const double* intr, double huber, const int* rk, int k, int rk_off, ProjLin& L) {
  double pc[3];
  pose_map(T, X, pc);
  const bool off = parent_edge_off(huber);
  if (off) { pc[0] = 0.0; pc[1] = 0.0; pc[2] = 1.0; }
  L.e[0] = uv[0] - (pc[0] / pc[2] * intr[0] + intr[2]);
  L.e[1] = uv[1] - (pc[1] / pc[2] * intr[1] + intr[3]);
  double x = pc[0], y = pc[1], z = pc[2], z_2 = z * z, fx = intr[0], fy = intr[1];
  double tmp[6] = {fx, 0, -x / z * fx, 0, fy, -y / z * fy};
  for (int i = 0; i < 2; i++)
    for (int j = 0; j < 3; j++) {
      double s = 0;
      for (int q = 0; q < 3; q++) s += (-1. / z * tmp[3 * i + q]) * R[3 * q + j];
      L.Jp[3 * i + j] = s;
    }
  L.Jc[0] = x * y / z_2 * fx; L.Jc[1] = -(1 + (x * x / z_2)) * fx; L.Jc[2] = y / z * fx; L.Jc[3] = -1. / z * fx; L.Jc[4] = 0; L.Jc[5] = x / z_2 * fx;
  L.Jc[6] = (1 + y * y / z_2) * fy; L.Jc[7] = -x * y / z_2 * fy; L.Jc[8] = -x / z * fy; L.Jc[9] = 0; L.Jc[10] = -1. / z * fy; L.Jc[11] = y / z_2 * fy;
  double c = L.e[0] * (info[0] * L.e[0] + info[1] * L.e[1]) + L.e[1] * (info[2] * L.e[0] + info[3] * L.e[1]);
  double rho1;
  parent_rho(rk, k, huber, (rk_off & RK_OFF_MONO) != 0, c, L.chi, rho1);
  if (off) { rho1 = 0.0; L.chi = 0.0; }
  for (int i = 0; i < 4; i++) L.Wm[i] = rho1 * info[i];
  L.r[0] = -(info[0] * L.e[0] + info[1] * L.e[1]) * rho1;
  L.r[1] = -(info[2] * L.e[0] + info[3] * L.e[1]) * rho1;
}
// the inline products of the four 2-row sites
static void parent_cam_terms(const ProjLin& L, double* A, double* b) {
  int q = 0;
  for (int i = 0; i < 6; i++) {
    double jw0 = L.Jc[i] * L.Wm[0] + L.Jc[6 + i] * L.Wm[2];
    double jw1 = L.Jc[i] * L.Wm[1] + L.Jc[6 + i] * L.Wm[3];
    for (int j = i; j < 6; j++) A[q++] += jw0 * L.Jc[j] + jw1 * L.Jc[6 + j];
    b[i] += L.Jc[i] * L.r[0] + L.Jc[6 + i] * L.r[1];
  }
}
static void parent_point_terms(const ProjLin& L, double* H6, double* b3) {
  double pw[6];
  for (int i = 0; i < 3; i++) {
    pw[2 * i] = L.Jp[i] * L.Wm[0] + L.Jp[3 + i] * L.Wm[2];
    pw[2 * i + 1] = L.Jp[i] * L.Wm[1] + L.Jp[3 + i] * L.Wm[3];
  }
  int q = 0;
  for (int i = 0; i < 3; i++) {
    for (int j = i; j < 3; j++) H6[q++] = pw[2 * i] * L.Jp[j] + pw[2 * i + 1] * L.Jp[3 + j];
    b3[i] = L.Jp[i] * L.r[0] + L.Jp[3 + i] * L.r[1];
  }
}
static void parent_hpl(const ProjLin& L, bool both, double* Wk) {
  for (int i = 0; i < 6; i++) {
    const double jw0 = L.Jc[i] * L.Wm[0] + L.Jc[6 + i] * L.Wm[2];
    const double jw1 = L.Jc[i] * L.Wm[1] + L.Jc[6 + i] * L.Wm[3];
    for (int j = 0; j < 3; j++) Wk[3 * i + j] = both ? (jw0 * L.Jp[j] + jw1 * L.Jp[3 + j]) : 0.0;
  }
}
struct ProjLin3 { double e[3], Jp[9], Jc[18], Wm[9], r[3], chi; };
static double parent_quad3(const double* e, const double* info) {
  return e[0] * ((info[0] * e[0] + info[1] * e[1]) + info[2] * e[2]) + e[1] * ((info[3] * e[0] + info[4] * e[1]) + info[5] * e[2]) + e[2] * ((info[6] * e[0] + info[7] * e[1]) + info[8] * e[2]);
}
static void parent_linearize_any(bool stereo, const Pose& T, const double* R, const double* X, const double* uv, const double* info, const double* intr, double huber, const int* rk, int k, int rk_off,
                                 double ur, const double* srec, ProjLin3& L) {
  double pc[3];
  pose_map(T, X, pc);
  const bool off = parent_edge_off(huber);
  if (off) { pc[0] = 0.0; pc[1] = 0.0; pc[2] = 1.0; }
  const double x = pc[0], y = pc[1], z = pc[2], z_2 = z * z, fx = intr[0], fy = intr[1];
  L.Jc[0] = x * y / z_2 * fx; L.Jc[1] = -(1 + (x * x / z_2)) * fx; L.Jc[2] = y / z * fx; L.Jc[3] = -1. / z * fx; L.Jc[4] = 0; L.Jc[5] = x / z_2 * fx;
  L.Jc[6] = (1 + y * y / z_2) * fy; L.Jc[7] = -x * y / z_2 * fy; L.Jc[8] = -x / z * fy; L.Jc[9] = 0; L.Jc[10] = -1. / z * fy; L.Jc[11] = y / z_2 * fy;
  double e0, e1, e2, c, W[9], jp[9], jc2[6];
  if (stereo) {
    const double bf = srec[9];
    double e[3];
    stereo_cam_project_error(pc, uv, ur, intr, bf, e);
    e0 = e[0]; e1 = e[1]; e2 = e[2];
    for (int j = 0; j < 3; j++) {
      jp[j] = -fx * R[j] / z + fx * x * R[6 + j] / z_2;
      jp[3 + j] = -fy * R[3 + j] / z + fy * y * R[6 + j] / z_2;
      jp[6 + j] = jp[j] - bf * R[6 + j] / z_2;
    }
    jc2[0] = L.Jc[0] - bf * y / z_2; jc2[1] = L.Jc[1] + bf * x / z_2; jc2[2] = L.Jc[2]; jc2[3] = L.Jc[3]; jc2[4] = 0; jc2[5] = L.Jc[5] - bf / z_2;
    for (int i = 0; i < 9; i++) W[i] = srec[i];
  } else {
    e0 = uv[0] - (x / z * fx + intr[2]);
    e1 = uv[1] - (y / z * fy + intr[3]);
    e2 = 0;
    const double tmp[6] = {fx, 0, -x / z * fx, 0, fy, -y / z * fy};
    for (int i = 0; i < 2; i++)
      for (int j = 0; j < 3; j++) {
        double s = 0;
        for (int q = 0; q < 3; q++) s += (-1. / z * tmp[3 * i + q]) * R[3 * q + j];
        jp[3 * i + j] = s;
      }
    jp[6] = 0; jp[7] = 0; jp[8] = 0;
    for (int i = 0; i < 6; i++) jc2[i] = 0;
    W[0] = info[0]; W[1] = info[1]; W[2] = 0; W[3] = info[2]; W[4] = info[3]; W[5] = 0; W[6] = 0; W[7] = 0; W[8] = 0;
  }
  L.e[0] = e0; L.e[1] = e1; L.e[2] = e2;
  for (int i = 0; i < 9; i++) L.Jp[i] = jp[i];
  for (int i = 0; i < 6; i++) L.Jc[12 + i] = jc2[i];
  c = parent_quad3(L.e, W);
  double rho1;
  parent_rho(rk, k, huber, (rk_off & (stereo ? RK_OFF_STEREO : RK_OFF_MONO)) != 0, c, L.chi, rho1);
  if (off) { rho1 = 0.0; L.chi = 0.0; }
  for (int i = 0; i < 9; i++) L.Wm[i] = rho1 * W[i];
  for (int i = 0; i < 3; i++) L.r[i] = -((W[3 * i] * L.e[0] + W[3 * i + 1] * L.e[1]) + W[3 * i + 2] * L.e[2]) * rho1;
}
static void parent_lin3_cam_terms(const ProjLin3& L, double* A21, double* b6) {
  int q = 0;
  for (int i = 0; i < 6; i++) {
    const double jw0 = (L.Jc[i] * L.Wm[0] + L.Jc[6 + i] * L.Wm[3]) + L.Jc[12 + i] * L.Wm[6];
    const double jw1 = (L.Jc[i] * L.Wm[1] + L.Jc[6 + i] * L.Wm[4]) + L.Jc[12 + i] * L.Wm[7];
    const double jw2 = (L.Jc[i] * L.Wm[2] + L.Jc[6 + i] * L.Wm[5]) + L.Jc[12 + i] * L.Wm[8];
    for (int j = i; j < 6; j++) A21[q++] += (jw0 * L.Jc[j] + jw1 * L.Jc[6 + j]) + jw2 * L.Jc[12 + j];
    b6[i] += (L.Jc[i] * L.r[0] + L.Jc[6 + i] * L.r[1]) + L.Jc[12 + i] * L.r[2];
  }
}
static void parent_lin3_point_terms(const ProjLin3& L, double* H6, double* b3) {
  double pw[9];
  for (int i = 0; i < 3; i++)
    for (int d = 0; d < 3; d++) pw[3 * i + d] = (L.Jp[i] * L.Wm[d] + L.Jp[3 + i] * L.Wm[3 + d]) + L.Jp[6 + i] * L.Wm[6 + d];
  int q = 0;
  for (int i = 0; i < 3; i++) {
    for (int j = i; j < 3; j++) H6[q++] = (pw[3 * i] * L.Jp[j] + pw[3 * i + 1] * L.Jp[3 + j]) + pw[3 * i + 2] * L.Jp[6 + j];
    b3[i] = (L.Jp[i] * L.r[0] + L.Jp[3 + i] * L.r[1]) + L.Jp[6 + i] * L.r[2];
  }
}
static double parent_lin3_hpl(const ProjLin3& L, int i, int j) {
  const double jw0 = (L.Jc[i] * L.Wm[0] + L.Jc[6 + i] * L.Wm[3]) + L.Jc[12 + i] * L.Wm[6];
  const double jw1 = (L.Jc[i] * L.Wm[1] + L.Jc[6 + i] * L.Wm[4]) + L.Jc[12 + i] * L.Wm[7];
  const double jw2 = (L.Jc[i] * L.Wm[2] + L.Jc[6 + i] * L.Wm[5]) + L.Jc[12 + i] * L.Wm[8];
  return (jw0 * L.Jp[j] + jw1 * L.Jp[3 + j]) + jw2 * L.Jp[6 + j];
}
// the plain chi2 as chi2_proj_block, ba_edge_chi_kernel and ba_classify_kernel each spelled it
static double parent_plain_chi(const BaView& v, int k, double* pc) {
  Pose T = pose_load(v.cams + 7 * v.pm_cam[k]);
  if (v.pm_kind && v.pm_kind[k]) {
    double e3[3];
    const double* srec = v.sinfo_u ? v.sinfo_u : v.pm_sinfo + 10 * (size_t)k;
    stereo_proj_error(T, v.points + 3 * v.pm_pt[k], v.pm_uv + 2 * k, v.pm_ur[k], v.intr_u ? v.intr_u : v.pm_intr + 4 * k, srec[9], e3, pc);
    return parent_quad3(e3, srec);
  }
  double e[2];
  proj_error(T, v.points + 3 * v.pm_pt[k], v.pm_uv + 2 * k, v.intr_u ? v.intr_u : v.pm_intr + 4 * k, e, pc);
  const double* info = v.info_u ? v.info_u : v.pm_info + 4 * k;
  return e[0] * (info[0] * e[0] + info[1] * e[1]) + e[1] * (info[2] * e[0] + info[3] * e[1]);
}

// ---- random edges ----------------------------------------------------------------------------------------------------------------------
struct Edges {
  int n = 0;
  std::vector<double> cams, points, uv, info, intr, width, ur, sinfo;
  std::vector<int> pt, cam, kind, rk;
};
static void spd(std::mt19937_64& g, int n, double scale, double* out) {   // a full symmetric positive definite n x n: B^T B + 0.1 I
  std::uniform_real_distribution<double> u(-1.0, 1.0);
  double B[9];
  for (int i = 0; i < n * n; i++) B[i] = u(g);
  for (int i = 0; i < n; i++)
    for (int j = 0; j <= i; j++) {
      double s = i == j ? 0.1 : 0.0;
      for (int q = 0; q < n; q++) s += B[n * q + i] * B[n * q + j];
      out[n * i + j] = out[n * j + i] = scale * s;
    }
}
static Edges make_edges(int n, unsigned seed) {
  std::mt19937_64 g(seed);
  std::uniform_real_distribution<double> u(-1.0, 1.0), u01(0.0, 1.0);
  Edges E;
  E.n = n;
  const double widths[6] = {0.0, 0.05, 1.0, std::sqrt(5.991), std::sqrt(7.815), 40.0};
  for (int k = 0; k < n; k++) {
    const bool level1 = k % 7 == 3, depth0 = level1 && k % 3 == 0;
    Pose T;
    if (depth0) { T.qx = T.qy = T.qz = 0; T.qw = 1; T.t[0] = T.t[1] = T.t[2] = 0; }   // (the camera frame is the world's: depth = X[2])
    else {
      T.qx = u(g); T.qy = u(g); T.qz = u(g); T.qw = u01(g) + 0.05;
      pose_normalize(T);
      for (int i = 0; i < 3; i++) T.t[i] = 3 * u(g);
    }
    // the point from where it is to land in the camera frame: in front (1 .. 20), near (1e-6 .. 1e-2 on either side), behind, or -- level 1 only -- depth 0
    const int where = k % 5;
    double pc[3] = {2 * u(g), 2 * u(g), 0.0};
    if (depth0) pc[2] = 0.0;
    else if (where < 2) pc[2] = 1.0 + 19.0 * u01(g);
    else if (where == 2) pc[2] = std::pow(10.0, -6.0 + 4.0 * u01(g));
    else if (where == 3) pc[2] = -std::pow(10.0, -6.0 + 4.0 * u01(g));
    else pc[2] = -(0.5 + 10.0 * u01(g));
    double d[3] = {pc[0] - T.t[0], pc[1] - T.t[1], pc[2] - T.t[2]}, X[3];
    Pose Ti = T; Ti.qx = -T.qx; Ti.qy = -T.qy; Ti.qz = -T.qz;
    pose_rotate(Ti, d, X);
    E.cams.insert(E.cams.end(), {T.t[0], T.t[1], T.t[2], T.qx, T.qy, T.qz, T.qw});
    E.points.insert(E.points.end(), X, X + 3);
    E.pt.push_back(k); E.cam.push_back(k);
    E.uv.push_back(320 + 300 * u(g)); E.uv.push_back(240 + 200 * u(g));
    double I2[4], I3[9];
    spd(g, 2, 1.0 + 4.0 * u01(g), I2);
    spd(g, 3, 1.0 + 4.0 * u01(g), I3);
    E.info.insert(E.info.end(), I2, I2 + 4);
    E.intr.insert(E.intr.end(), {500 + 50 * u(g), 510 + 50 * u(g), 320 + 5 * u(g), 240 + 5 * u(g)});
    E.sinfo.insert(E.sinfo.end(), I3, I3 + 9);
    E.sinfo.push_back(35.0 + 10 * u01(g));                  // bf
    E.ur.push_back(300 + 300 * u(g));
    const double w = widths[(k / 7) % 6];
    E.width.push_back(level1 ? -w : w);                     // (level 1 at width 0: the record is -0.0)
    E.kind.push_back((k / 2) % 3 == 0 ? 1 : 0);
    E.rk.push_back((k / 3) % RK_KINDS);
  }
  return E;
}

template <bool STEREO>
static void check_view(const BaView& v, const Edges& E) {
  const ProjTable<STEREO> tab(v, PointMajor{});
  for (int k = 0; k < E.n; k++) {
    g_edge = k;
    double pc_a[3], pc_b[3];
    const double a = proj_edge_chi(tab, (size_t)k, pc_a), b = parent_plain_chi(v, k, pc_b);
    CHECK(same_bytes(a, b) && same_bytes(pc_a, pc_b));
    CHECK(tab.stereo(k) == (STEREO && E.kind[k] != 0));
    // the table's linearisation is the raw one on the records the accessors pick
    const Pose T = pose_load(v.cams + 7 * k);
    double R[9];
    pose_rotmat(T, R);
    ProjLinT<STEREO ? 3 : 2> La, Lb;
    std::memset(&La, 0, sizeof La); std::memset(&Lb, 0, sizeof Lb);
    proj_linearize(tab, (size_t)k, T, R, tab.point_of(k), La);
    proj_linearize(T, R, v.points + 3 * k, v.pm_uv + 2 * k, v.info_u ? v.info_u : v.pm_info + 4 * k, v.intr_u ? v.intr_u : v.pm_intr + 4 * k, v.pm_huber[k], v.pm_rk, k, v.rk_off,
                   STEREO && E.kind[k] != 0, STEREO ? E.ur[k] : 0.0, STEREO ? (v.sinfo_u ? v.sinfo_u : v.pm_sinfo + 10 * k) : nullptr, Lb);
    CHECK(std::memcmp(&La, &Lb, sizeof La) == 0);
    for (int q = 0; q < 4; q++) CHECK(tab.info_at(k, q) == tab.info_of(k)[q] && tab.intr_at(k, q) == tab.intr_of(k)[q]);
  }
}

int main() {
  // the level's bit, read on the host as on the device
  CHECK(!edge_off(0.0) && edge_off(-0.0) && !edge_off(2.5) && edge_off(-2.5) && !edge_off(INFINITY) && edge_off(-INFINITY));

  const int N = 4200;
  const Edges E = make_edges(N, 20240611u);
  long n_level1 = 0, n_depth0 = 0, n_behind = 0, n_stereo = 0;
  for (int pass = 0; pass < 4; pass++) {
    // pass 0: Huber-or-none from the width alone; 1: every kind through the kind array; 2, 3: the same with the classes' kernels switched off in turn
    const int* rk = (pass & 1) ? E.rk.data() : nullptr;
    const int rk_off = pass == 2 ? RK_OFF_MONO : (pass == 3 ? RK_OFF_STEREO | RK_OFF_CUB3 : 0);
    for (int k = 0; k < N; k++) {
      g_edge = k;
      const Pose T = pose_load(E.cams.data() + 7 * k);
      double R[9];
      pose_rotmat(T, R);
      const double *X = E.points.data() + 3 * k, *uv = E.uv.data() + 2 * k, *info = E.info.data() + 4 * k, *intr = E.intr.data() + 4 * k, *srec = E.sinfo.data() + 10 * k;
      const double width = E.width[k], ur = E.ur[k];
      const bool stereo = E.kind[k] != 0, level1 = edge_off(width);
      double pc[3];
      pose_map(T, X, pc);
      if (pass == 0) { n_level1 += level1; n_depth0 += level1 && pc[2] == 0.0; n_behind += pc[2] < 0; n_stereo += stereo; }
      // accumulators that are not zero: the camera terms ADD
      double A0[21], b0[6];
      for (int i = 0; i < 21; i++) A0[i] = 0.25 * i - 2.0;
      for (int i = 0; i < 6; i++) b0[i] = 1.5 - i;

      // (a) the 2-row form
      ProjLin P2; ProjLinT<2> L2;
      std::memset(&P2, 0, sizeof P2); std::memset(&L2, 0, sizeof L2);
      parent_linearize(T, R, X, uv, info, intr, width, rk, k, rk_off, P2);
      proj_linearize(T, R, X, uv, info, intr, width, rk, (size_t)k, rk_off, false, 0.0, nullptr, L2);
      CHECK(same_bytes(P2.e, L2.e) && same_bytes(P2.Jp, L2.Jp) && same_bytes(P2.Jc, L2.Jc) && same_bytes(P2.Wm, L2.Wm) && same_bytes(P2.r, L2.r) && same_bytes(P2.chi, L2.chi));
      double pA[21], pb[6], lA[21], lb[6], pH[6], pb3[3], lH[6], lb3[3], pW[18], lW[18], zA[21] = {0}, zb[6] = {0};
      std::memcpy(pA, A0, sizeof pA); std::memcpy(lA, A0, sizeof lA); std::memcpy(pb, b0, sizeof pb); std::memcpy(lb, b0, sizeof lb);
      parent_cam_terms(P2, pA, pb); lin_cam_terms(L2, lA, lb);
      CHECK(same_bytes(pA, lA) && same_bytes(pb, lb));
      parent_point_terms(P2, pH, pb3); lin_point_terms(L2, lH, lb3);
      CHECK(same_bytes(pH, lH) && same_bytes(pb3, lb3));
      for (int both = 0; both < 2; both++) {
        parent_hpl(P2, both != 0, pW);
        lin_hpl(L2, both != 0, [&](int i, int j) -> double& { return lW[3 * i + j]; });
        CHECK(same_bytes(pW, lW));
      }
      for (int i = 0; i < 6; i++) { double h3[3]; lin_hpl_row(L2, i, h3); CHECK(std::memcmp(h3, pW + 3 * i, sizeof h3) == 0); }
      lin_cam_terms(L2, zA, zb);
      if (level1) CHECK(all_zero(zA) && all_zero(zb) && all_zero(lH) && all_zero(lb3) && all_zero(lW) && L2.chi == 0.0);

      // (b) the 3-row form, the edge as the kind it has
      ProjLin3 P3; ProjLinT<3> L3;
      std::memset(&P3, 0, sizeof P3); std::memset(&L3, 0, sizeof L3);
      parent_linearize_any(stereo, T, R, X, uv, info, intr, width, rk, k, rk_off, ur, srec, P3);
      proj_linearize(T, R, X, uv, info, intr, width, rk, (size_t)k, rk_off, stereo, ur, srec, L3);
      CHECK(same_bytes(P3.e, L3.e) && same_bytes(P3.Jp, L3.Jp) && same_bytes(P3.Jc, L3.Jc) && same_bytes(P3.Wm, L3.Wm) && same_bytes(P3.r, L3.r) && same_bytes(P3.chi, L3.chi));
      double qA[21], qb[6], mA[21], mb[6], qH[6], qb3[3], mH[6], mb3[3], qW[18], mW[18], yA[21] = {0}, yb[6] = {0};
      std::memcpy(qA, A0, sizeof qA); std::memcpy(mA, A0, sizeof mA); std::memcpy(qb, b0, sizeof qb); std::memcpy(mb, b0, sizeof mb);
      parent_lin3_cam_terms(P3, qA, qb); lin_cam_terms(L3, mA, mb);
      CHECK(same_bytes(qA, mA) && same_bytes(qb, mb));
      parent_lin3_point_terms(P3, qH, qb3); lin_point_terms(L3, mH, mb3);
      CHECK(same_bytes(qH, mH) && same_bytes(qb3, mb3));
      for (int both = 0; both < 2; both++) {
        for (int i = 0; i < 6; i++) for (int j = 0; j < 3; j++) qW[3 * i + j] = both ? parent_lin3_hpl(P3, i, j) : 0.0;
        lin_hpl(L3, both != 0, [&](int i, int j) -> double& { return mW[3 * i + j]; });
        CHECK(same_bytes(qW, mW));
      }
      lin_cam_terms(L3, yA, yb);
      if (level1) CHECK(all_zero(yA) && all_zero(yb) && all_zero(mH) && all_zero(mb3) && all_zero(mW) && L3.chi == 0.0);

      // (c) the edge as a MONO edge through the 3-row form: the 2-row values
      ProjLinT<3> M3;
      std::memset(&M3, 0, sizeof M3);
      proj_linearize(T, R, X, uv, info, intr, width, rk, (size_t)k, rk_off, false, ur, srec, M3);
      CHECK(same_values(M3.e, L2.e) && M3.e[2] == 0.0 && same_values(M3.Jp, L2.Jp) && same_values(M3.Jc, L2.Jc) && same_values(M3.r, L2.r) && same_value(M3.r[2], 0.0 * L2.r[0]) && same_value(M3.chi, L2.chi));
      for (int i = 0; i < 3; i++) CHECK(M3.Jp[6 + i] == 0.0);
      for (int i = 0; i < 6; i++) CHECK(M3.Jc[12 + i] == 0.0);
      for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) CHECK(same_value(M3.Wm[3 * i + j], (i < 2 && j < 2) ? L2.Wm[2 * i + j] : 0.0 * L2.Wm[0]));      // (0 * rho': a zero, or NaN with rho')
      double cA[21], cb[6], cH[6], cb3[3], cW[18];
      std::memcpy(cA, A0, sizeof cA); std::memcpy(cb, b0, sizeof cb);
      lin_cam_terms(M3, cA, cb); lin_point_terms(M3, cH, cb3);
      lin_hpl(M3, true, [&](int i, int j) -> double& { return cW[3 * i + j]; });
      CHECK(same_values(cA, lA) && same_values(cb, lb) && same_values(cH, lH) && same_values(cb3, lb3) && same_values(cW, lW));
      double wA[21] = {0}, wb[6] = {0};
      lin_cam_terms(M3, wA, wb);
      CHECK(same_values(wA, zA) && same_values(wb, zb));
    }
  }
  // what the generator promises
  g_edge = -1;
  CHECK(n_level1 > 500 && n_depth0 > 100 && n_behind > 1000 && n_stereo > 1000 && n_stereo < N - 1000);

  // the table view and the plain chi2: per-edge records, then the graph's one record of each kind; mono graph and stereo graph
  for (int uniform = 0; uniform < 2; uniform++) {
    BaView v;
    std::memset(&v, 0, sizeof v);
    std::vector<double> cams = E.cams, points = E.points;
    v.cams = cams.data(); v.points = points.data(); v.n_proj = N;
    v.pm_pt = E.pt.data(); v.pm_cam = E.cam.data(); v.pm_uv = E.uv.data(); v.pm_huber = E.width.data(); v.pm_rk = E.rk.data();
    if (uniform) { v.info_u = E.info.data() + 4 * 11; v.intr_u = E.intr.data() + 4 * 11; v.sinfo_u = E.sinfo.data() + 10 * 11; }
    else { v.pm_info = E.info.data(); v.pm_intr = E.intr.data(); v.pm_sinfo = E.sinfo.data(); }
    check_view<false>(v, E);
    v.pm_kind = E.kind.data(); v.pm_ur = E.ur.data();
    check_view<true>(v, E);
    // the camera-major table: the cm_* arrays, the same uniform records, no camera index
    v.cm_pt = E.pt.data() + 1; v.cm_uv = E.uv.data() + 2; v.cm_info = E.info.data() + 4; v.cm_intr = E.intr.data() + 4; v.cm_huber = E.width.data() + 1;
    v.cm_kind = E.kind.data() + 1; v.cm_ur = E.ur.data() + 1; v.cm_sinfo = E.sinfo.data() + 10; v.cm_rk = E.rk.data() + 1;
    const ProjTable<true> cm(v, CameraMajor{});
    CHECK(cm.pt == v.cm_pt && cm.cam == nullptr && cm.uv == v.cm_uv && cm.info == v.cm_info && cm.intr == v.cm_intr && cm.width == v.cm_huber && cm.kind == v.cm_kind && cm.ur_ == v.cm_ur &&
          cm.sinfo == v.cm_sinfo && cm.rk == v.cm_rk && cm.info_u == v.info_u && cm.intr_u == v.intr_u && cm.sinfo_u == v.sinfo_u && cm.rk_off == v.rk_off);
  }
  if (g_fail) { std::printf("ba_proj_edge_check: %ld FAILED\n", g_fail); return 1; }
  std::printf("%d edges x 4 passes: %ld at level 1 (%ld at depth 0), %ld behind the camera, %ld stereo\n", N, n_level1, n_depth0, n_behind, n_stereo);
  std::printf("ba_proj_edge_check: ok\n");
  return 0;
}
