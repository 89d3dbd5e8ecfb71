// cs_sim3_ransac.h -- RANSAC over 3-point Horn alignments of one keyframe pair's matches, for host and device
// (include/cubeslam_hip.h: cs_sim3_ransac_*).
//
// What an ORB-SLAM2-derived loop closer runs per loop candidate in front of Optimizer::OptimizeSim3: Sim3Solver (its constructor,
// SetRansacParameters, iterate called until it succeeds or says bNoMore, ComputeSim3, CheckInliers), NOT IN THE REFERENCE.  The statement:
//
//   image points   p1 = proj1(P1), p2 = proj2(P2): the projections of the stored points themselves, not the keypoints;
//                  proj(P) = (fx P.x (1 / P.z) + cx, fy P.y (1 / P.z) + cy); no depth test.
//   budget         N matches.  N < max(3, min_inliers): the pair is not run.  Otherwise eps = min_inliers / N, its = 1 if eps >= 1, else
//                  ceil(log(1 - probability) / log(1 - eps^3)) (every hypothesis when log(1 - eps^3) is 0: eps^3 below the rounding of 1),
//                  max_its = max(1, min(its, max_iterations)); in double on the host (sim3_ransac_budget).
//   draws          hypothesis h takes three distinct matches as Sim3Solver does: from the list 0 .. N-1 pick position r among the remaining
//                  entries, take it, overwrite it with the last entry, shrink.  r = splitmix64(seed + (3 h + k) * 0x9E3779B97F4A7C15)
//                  modulo the remaining count, k = 0, 1, 2: counter-based, so a lane computes its own triple, and without the list
//                  (sim3_ransac_triple: three picks with swap-with-last are a few compares).
//   hypothesis     Horn 1987 as Sim3Solver::ComputeSim3: centroids O1, O2, centred triples Pr1, Pr2, M = Pr2 Pr1^T, the symmetric 4 x 4
//                    N11 = M00+M11+M22  N12 = M12-M21  N13 = M20-M02  N14 = M01-M10   N22 = M00-M11-M22  N23 = M01+M10  N24 = M20+M02
//                    N33 = -M00+M11-M22  N34 = M12+M21   N44 = -M00-M11+M22
//                  whose eigenvector of the largest eigenvalue is the quaternion (w, x, y, z): cyclic Jacobi rotations, a fixed number of
//                  sweeps, a rotation whose off-diagonal entry is zero skipped by selects (no lane diverges); normalised, and its sign
//                  flipped so that w >= 0 (w == 0: the first non-zero of x, y, z positive).  R12 is built from the unit quaternion
//                  DIRECTLY.  ORB-SLAM2 goes through atan2 and cv::Rodrigues to the same rotation; going direct needs no libm and has no
//                  0 / 0 at the identity.  s = 1 under fix_scale, else sum(Pr1 . (R Pr2)) / sum((R Pr2)^2); t12 = O1 - s R O2; the
//                  inverse map is R^T / s, -R^T t / s.  A hypothesis whose s is not finite and positive counts 0 inliers and is never stored.
//   inliers        |p1 - proj1(s R P2 + t)|^2 < max_err1 AND |p2 - proj2(R^T (P1 - t) / s)|^2 < max_err2; a NaN or inf error is no inlier.
//   selection      h = 0 .. max_its - 1 in order; count >= best is stored (>=: the LAST of equals); the first count > min_inliers
//                  (strict) ends the search: found.  Nothing found: the stored best is handed out with found = 0 (ORB-SLAM2 returns an
//                  empty matrix there).  Nothing stored: hyp = -1, the identity, no inlier.
//
// sim3_ransac_pair_serial is the selection as stated, one hypothesis after the other (tools/hostonly/sim3_ransac_host_check.cpp);
// sim3_ransac_kernels.hip evaluates 64 hypotheses at a time, one per lane, from the same routines.  FP64, -ffp-contract=off.
#pragma once
#include <float.h>
#include <stdint.h>

#include "cs_dense_lm.h"      // CS_HD, CS_UNROLL, CS_NOUNROLL
#include "cs_se3.h"           // quat_rotmat

namespace cs {

// A match as the host packs it: 8 doubles = 64 bytes   [0..2] P1   [3..5] P2   [6] max_err1   [7] max_err2
// and as it is staged (the projections done once):     [0..2] P1   [3..5] P2   [6..7] p1   [8..9] p2   [10] max_err1   [11] max_err2
enum { SIM3_RANSAC_MATCH_DOUBLES = 8, SIM3_RANSAC_STAGED_DOUBLES = 12, SIM3_RANSAC_MAX_ITERATIONS = 1024, SIM3_RANSAC_JACOBI_SWEEPS = 12 };

CS_HD uint64_t sim3_ransac_splitmix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// The three matches of hypothesis h among n >= 3.  After pick r0 the list is the identity but for entry r0, which holds n-1; after pick r1
// entry r1 holds what entry n-2 held; the third pick reads one entry of that.
CS_HD void sim3_ransac_triple(uint64_t seed, int h, int n, int* idx) {
  const uint64_t c = 3ull * (uint64_t)h;
  const int r0 = (int)(sim3_ransac_splitmix64(seed + (c + 0) * 0x9E3779B97F4A7C15ull) % (uint64_t)n);
  const int r1 = (int)(sim3_ransac_splitmix64(seed + (c + 1) * 0x9E3779B97F4A7C15ull) % (uint64_t)(n - 1));
  const int r2 = (int)(sim3_ransac_splitmix64(seed + (c + 2) * 0x9E3779B97F4A7C15ull) % (uint64_t)(n - 2));
  const int last1 = (r0 == n - 2) ? n - 1 : n - 2;      // entry n-2 after the first pick
  idx[0] = r0;
  idx[1] = (r1 == r0) ? n - 1 : r1;
  idx[2] = (r2 == r1) ? last1 : (r2 == r0) ? n - 1 : r2;
}

// max_its of a pair, 0 = not run.  Host only in spirit (log is libm's); the kernel is handed the result.
CS_HD int sim3_ransac_budget(int n, double probability, int min_inliers, int max_iterations) {
  if (n < 3 || n < min_inliers) return 0;
  const double eps = (double)min_inliers / (double)n;
  double its = 1.0;
  if (!(eps >= 1.0)) {
    const double den = log(1.0 - eps * eps * eps);
    its = (den == 0.0) ? (double)max_iterations : ceil(log(1.0 - probability) / den);
  }
  if (!(its < (double)max_iterations)) its = (double)max_iterations;
  return its < 1.0 ? 1 : (int)its;
}

// One Jacobi rotation of the symmetric 4 x 4 a (both triangles kept) in the plane (P, Q), accumulated into v (columns = eigenvectors).
// P and Q are template arguments: every index is a constant, nothing is addressed, and a lane whose entry is already zero rotates by
// the identity (c = 1, s = 0) instead of branching.
template <int P, int Q>
CS_HD void sim3_ransac_jacobi_rotate(double (&a)[4][4], double (&v)[4][4]) {
  const double apq = a[P][Q];
  const bool skip = (apq == 0.0);
  const double theta = (a[Q][Q] - a[P][P]) / (skip ? 1.0 : 2.0 * apq);
  const double r = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));      // (theta^2 = inf: r = 0)
  const double t = skip ? 0.0 : (theta < 0.0 ? -r : r);
  const double c = 1.0 / sqrt(t * t + 1.0);
  const double s = t * c;
  const double tau = s / (1.0 + c);
  a[P][P] = a[P][P] - t * apq;
  a[Q][Q] = a[Q][Q] + t * apq;
  a[P][Q] = 0.0; a[Q][P] = 0.0;
  CS_UNROLL
  for (int k = 0; k < 4; k++) {
    if (k != P && k != Q) {
      const double g = a[k][P], hq = a[k][Q];
      const double np = g - s * (hq + g * tau), nq = hq + s * (g - hq * tau);
      a[k][P] = np; a[P][k] = np;
      a[k][Q] = nq; a[Q][k] = nq;
    }
  }
  CS_UNROLL
  for (int k = 0; k < 4; k++) {
    const double g = v[k][P], hq = v[k][Q];
    v[k][P] = g - s * (hq + g * tau);
    v[k][Q] = hq + s * (g - hq * tau);
  }
}

// The unit eigenvector (w, x, y, z) of the largest eigenvalue of the symmetric 4 x 4 whose upper triangle is n10 (row by row), sign fixed.
CS_HD void sim3_ransac_top_eigenvector(const double* n10, double* q) {
  double a[4][4], v[4][4];
  a[0][0] = n10[0]; a[0][1] = n10[1]; a[0][2] = n10[2]; a[0][3] = n10[3];
  a[1][1] = n10[4]; a[1][2] = n10[5]; a[1][3] = n10[6];
  a[2][2] = n10[7]; a[2][3] = n10[8];
  a[3][3] = n10[9];
  a[1][0] = a[0][1]; a[2][0] = a[0][2]; a[3][0] = a[0][3]; a[2][1] = a[1][2]; a[3][1] = a[1][3]; a[3][2] = a[2][3];
  CS_UNROLL
  for (int i = 0; i < 4; i++) {
    CS_UNROLL
    for (int j = 0; j < 4; j++) v[i][j] = (i == j) ? 1.0 : 0.0;
  }
  CS_NOUNROLL
  for (int sweep = 0; sweep < SIM3_RANSAC_JACOBI_SWEEPS; sweep++) {
    sim3_ransac_jacobi_rotate<0, 1>(a, v);
    sim3_ransac_jacobi_rotate<0, 2>(a, v);
    sim3_ransac_jacobi_rotate<0, 3>(a, v);
    sim3_ransac_jacobi_rotate<1, 2>(a, v);
    sim3_ransac_jacobi_rotate<1, 3>(a, v);
    sim3_ransac_jacobi_rotate<2, 3>(a, v);
  }
  // the first of equal largest diagonal entries
  double best = a[0][0];
  q[0] = v[0][0]; q[1] = v[1][0]; q[2] = v[2][0]; q[3] = v[3][0];
  CS_UNROLL
  for (int k = 1; k < 4; k++) {
    const bool up = a[k][k] > best;
    best = up ? a[k][k] : best;
    CS_UNROLL
    for (int i = 0; i < 4; i++) q[i] = up ? v[i][k] : q[i];
  }
  const double inv = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  CS_UNROLL
  for (int i = 0; i < 4; i++) q[i] = q[i] * inv;
  // w >= 0; w == 0: the first non-zero of x, y, z positive
  const double lead = (q[0] != 0.0) ? q[0] : (q[1] != 0.0) ? q[1] : (q[2] != 0.0) ? q[2] : q[3];
  const bool flip = lead < 0.0;
  CS_UNROLL
  for (int i = 0; i < 4; i++) q[i] = flip ? -q[i] : q[i];
}

// The rotation matrix (row-major) of the unit quaternion (w, x, y, z)
CS_HD void sim3_ransac_rotation(const double* q, double* R) {
  quat_rotmat(q[0], q[1], q[2], q[3], R);
}

// A hypothesis as it is kept and handed out: the unit quaternion (w, x, y, z), t12 and s.
struct Sim3RansacHyp {
  double q[4], t[3], s;
};

// Horn's alignment of three matches.  X1 / X2: the three points in camera 1 / camera 2, point k at [3 k ..].  false: refused.
CS_HD bool sim3_ransac_hypothesis(const double* X1, const double* X2, bool fix_scale, Sim3RansacHyp& H) {
  double O1[3], O2[3], Pr1[9], Pr2[9];
  CS_UNROLL
  for (int i = 0; i < 3; i++) {
    O1[i] = (X1[i] + X1[3 + i] + X1[6 + i]) / 3.0;
    O2[i] = (X2[i] + X2[3 + i] + X2[6 + i]) / 3.0;
    CS_UNROLL
    for (int k = 0; k < 3; k++) { Pr1[3 * k + i] = X1[3 * k + i] - O1[i]; Pr2[3 * k + i] = X2[3 * k + i] - O2[i]; }
  }
  double M[9];      // M = Pr2 Pr1^T: M[i][j] = sum over the points of Pr2_i Pr1_j
  CS_UNROLL
  for (int i = 0; i < 3; i++) {
    CS_UNROLL
    for (int j = 0; j < 3; j++) M[3 * i + j] = Pr2[i] * Pr1[j] + Pr2[3 + i] * Pr1[3 + j] + Pr2[6 + i] * Pr1[6 + j];
  }
  double n10[10];
  n10[0] = M[0] + M[4] + M[8]; n10[1] = M[5] - M[7]; n10[2] = M[6] - M[2]; n10[3] = M[1] - M[3];
  n10[4] = M[0] - M[4] - M[8]; n10[5] = M[1] + M[3]; n10[6] = M[6] + M[2];
  n10[7] = -M[0] + M[4] - M[8]; n10[8] = M[5] + M[7];
  n10[9] = -M[0] - M[4] + M[8];
  sim3_ransac_top_eigenvector(n10, H.q);
  double R[9];
  sim3_ransac_rotation(H.q, R);
  double s = 1.0;
  if (!fix_scale) {
    double nom = 0.0, den = 0.0;
    CS_UNROLL
    for (int k = 0; k < 3; k++) {
      CS_UNROLL
      for (int i = 0; i < 3; i++) {
        const double p3 = R[3 * i] * Pr2[3 * k] + R[3 * i + 1] * Pr2[3 * k + 1] + R[3 * i + 2] * Pr2[3 * k + 2];
        nom = nom + Pr1[3 * k + i] * p3;
        den = den + p3 * p3;
      }
    }
    s = nom / den;
  }
  H.s = s;
  CS_UNROLL
  for (int i = 0; i < 3; i++) H.t[i] = O1[i] - s * (R[3 * i] * O2[0] + R[3 * i + 1] * O2[1] + R[3 * i + 2] * O2[2]);
  return s > 0.0 && s <= DBL_MAX;      // finite and positive (a NaN compares false)
}

// The two maps of a hypothesis: x1 = A12 x2 + b12 (A12 = s R) and x2 = A21 x1 + b21 (A21 = R^T / s, b21 = -A21 t).
struct Sim3RansacMaps {
  double A12[9], b12[3], A21[9], b21[3];
};

CS_HD Sim3RansacMaps sim3_ransac_maps(const Sim3RansacHyp& H) {
  Sim3RansacMaps T;
  double R[9];
  sim3_ransac_rotation(H.q, R);
  const double inv_s = 1.0 / H.s;
  CS_UNROLL
  for (int i = 0; i < 3; i++) {
    CS_UNROLL
    for (int j = 0; j < 3; j++) { T.A12[3 * i + j] = H.s * R[3 * i + j]; T.A21[3 * i + j] = R[3 * j + i] * inv_s; }
    T.b12[i] = H.t[i];
  }
  CS_UNROLL
  for (int i = 0; i < 3; i++) T.b21[i] = -(T.A21[3 * i] * H.t[0] + T.A21[3 * i + 1] * H.t[1] + T.A21[3 * i + 2] * H.t[2]);
  return T;
}

// proj(P) with intr4 = fx fy cx cy
CS_HD void sim3_ransac_project(const double* P, const double* intr4, double* p) {
  const double iz = 1.0 / P[2];
  p[0] = intr4[0] * P[0] * iz + intr4[2];
  p[1] = intr4[1] * P[1] * iz + intr4[3];
}

// A packed match (8 doubles) as a staged one (12 doubles)
CS_HD void sim3_ransac_stage(const double* in8, const double* intr8, double* out12) {
  CS_UNROLL
  for (int k = 0; k < 6; k++) out12[k] = in8[k];
  sim3_ransac_project(in8, intr8, out12 + 6);
  sim3_ransac_project(in8 + 3, intr8 + 4, out12 + 8);
  out12[10] = in8[6];
  out12[11] = in8[7];
}

// |p - proj(A x + b)|^2
CS_HD double sim3_ransac_error(const double* A, const double* b, const double* x, const double* intr4, const double* p) {
  double y[3], u[2];
  CS_UNROLL
  for (int i = 0; i < 3; i++) y[i] = A[3 * i] * x[0] + A[3 * i + 1] * x[1] + A[3 * i + 2] * x[2] + b[i];
  sim3_ransac_project(y, intr4, u);
  const double d0 = p[0] - u[0], d1 = p[1] - u[1];
  return d0 * d0 + d1 * d1;
}

// A staged match against a hypothesis' maps (a NaN compares false)
CS_HD bool sim3_ransac_inlier(const Sim3RansacMaps& T, const double* m12, const double* intr8) {
  const double e1 = sim3_ransac_error(T.A12, T.b12, m12 + 3, intr8, m12 + 6);
  const double e2 = sim3_ransac_error(T.A21, T.b21, m12, intr8 + 4, m12 + 8);
  return (e1 < m12[10]) & (e2 < m12[11]);
}

// What a pair hands out.  S12 in Sim3::operator[] order: qx qy qz qw tx ty tz s.
struct Sim3RansacResult {
  int found, hyp, iterations, n_inliers;
  double S12[8];
};

CS_HD void sim3_ransac_result_init(Sim3RansacResult& r, int iterations) {
  r.found = 0; r.hyp = -1; r.iterations = iterations; r.n_inliers = 0;
  CS_UNROLL
  for (int k = 0; k < 8; k++) r.S12[k] = (k == 3 || k == 7) ? 1.0 : 0.0;
}

CS_HD void sim3_ransac_store(const Sim3RansacHyp& H, double* S12) {
  S12[0] = H.q[1]; S12[1] = H.q[2]; S12[2] = H.q[3]; S12[3] = H.q[0];
  S12[4] = H.t[0]; S12[5] = H.t[1]; S12[6] = H.t[2]; S12[7] = H.s;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// Hypothesis h of a pair and its count.  rec: the pair's n packed matches.  false: refused (count 0).
static inline bool sim3_ransac_evaluate(const double* rec, int n, const double* intr8, bool fix_scale, uint64_t seed, int h, Sim3RansacHyp& H, int& count) {
  int idx[3];
  sim3_ransac_triple(seed, h, n, idx);
  double X1[9], X2[9];
  for (int k = 0; k < 3; k++)
    for (int i = 0; i < 3; i++) { X1[3 * k + i] = rec[(size_t)idx[k] * SIM3_RANSAC_MATCH_DOUBLES + i]; X2[3 * k + i] = rec[(size_t)idx[k] * SIM3_RANSAC_MATCH_DOUBLES + 3 + i]; }
  count = 0;
  if (!sim3_ransac_hypothesis(X1, X2, fix_scale, H)) return false;
  const Sim3RansacMaps T = sim3_ransac_maps(H);
  for (int i = 0; i < n; i++) {
    double m[SIM3_RANSAC_STAGED_DOUBLES];
    sim3_ransac_stage(rec + (size_t)i * SIM3_RANSAC_MATCH_DOUBLES, intr8, m);
    count += sim3_ransac_inlier(T, m, intr8) ? 1 : 0;
  }
  return true;
}

// The selection as stated, one hypothesis after the other.  max_its from sim3_ransac_budget; flags: n bytes.
static inline Sim3RansacResult sim3_ransac_pair_serial(const double* rec, int n, const double* intr8, bool fix_scale, uint64_t seed, int min_inliers, int max_its,
                                                       unsigned char* flags) {
  Sim3RansacResult r;
  sim3_ransac_result_init(r, max_its);
  for (int i = 0; i < n; i++) flags[i] = 0;
  Sim3RansacHyp best;
  int best_count = 0;
  for (int h = 0; h < max_its; h++) {
    Sim3RansacHyp H;
    int count;
    if (!sim3_ransac_evaluate(rec, n, intr8, fix_scale, seed, h, H, count)) continue;
    if (count >= best_count) { best = H; best_count = count; r.hyp = h; }
    if (count > min_inliers) { r.found = 1; r.iterations = h + 1; break; }
  }
  if (r.hyp < 0) return r;
  r.n_inliers = best_count;
  sim3_ransac_store(best, r.S12);
  const Sim3RansacMaps T = sim3_ransac_maps(best);
  for (int i = 0; i < n; i++) {
    double m[SIM3_RANSAC_STAGED_DOUBLES];
    sim3_ransac_stage(rec + (size_t)i * SIM3_RANSAC_MATCH_DOUBLES, intr8, m);
    flags[i] = sim3_ransac_inlier(T, m, intr8) ? 1 : 0;
  }
  return r;
}
#endif

}  // namespace cs
