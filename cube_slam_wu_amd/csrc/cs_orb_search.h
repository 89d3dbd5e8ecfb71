// cs_orb_search.h -- guided ORB matching by projection: for each projected map point the nearest 256-bit descriptor among the keypoints of
// a keyframe inside a window around the projection, for host and device (include/cubeslam_hip.h: cs_orb_search_*).
//
// What an ORB-SLAM2-derived back end runs between its geometric steps: ORBmatcher::Fuse(pKF, vpMapPoints, th) in
// LocalMapping::SearchInNeighbors, ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint) in LoopClosing::SearchAndFuse and
// ORBmatcher::SearchBySim3 in LoopClosing::ComputeSim3, with KeyFrame::GetFeaturesInArea and MapPoint::PredictScale, NOT IN THE
// REFERENCE.  In these routines a query's result depends on that query alone.  ORBmatcher::SearchByProjection (tracking) and
// SearchForTriangulation assign keypoints while they loop -- a later point sees what an earlier one took -- and are NOT what this states.
// ORB-SLAM2 computes in float32; this statement is FP64.
//
//   frame          n keypoints (u, v, ur), ur < 0: no right-image coordinate; an octave and 32 descriptor bytes per keypoint;
//                  cam = fx fy cx cy bf; bounds = min_x max_x min_y max_y; scale_factor > 1; n_levels in 1 .. 16.
//                  scale[0] = 1, scale[l] = scale[l-1] scale_factor, inv_sigma2[l] = 1 / (scale[l] scale[l])      (orb_frame_record)
//   grid           cols x rows cells, inv_w = cols / (max_x - min_x), inv_h = rows / (max_y - min_y).  A keypoint's cell is
//                  (floor((u - min_x) inv_w + 0.5), floor((v - min_y) inv_h + 0.5)); a keypoint whose cell is outside the grid is in NO cell
//                  and is never a candidate -- ORB-SLAM2's own behaviour at the right and bottom border (Frame::PosInGrid rounds to
//                  nearest and refuses cell == cols), kept.  The keypoints are laid out sorted by cell = cx rows + cy, stable in their
//                  index (orb_pack_frame); start[cell] .. start[cell + 1] - 1 are the cell's.
//   job            a frame; Xc = s (R X) + t, R the rotation matrix of q / |q| of the pose x y z qx qy qz qw, t = x y z; th; max_hamming;
//                  flags CHECK_VIEW, CHECK_REPROJ.                                                               (orb_job_record)
//   query          X, normal, min_distance, max_distance, 32 descriptor bytes, a skip byte.  The first step that fails gives the status:
//   1              skip: SKIPPED
//   2              Xc[2] <= 0: BEHIND      (ORB-SLAM2 tests < 0; a point of depth zero has no projection: a stated deviation)
//   3              u = fx Xc0 / Xc2 + cx, v = fy Xc1 / Xc2 + cy; not (min_x <= u < max_x and min_y <= v < max_y): OUT_OF_IMAGE;
//                  ur = u - bf / Xc2
//   4              dist = |Xc|; dist < min_dist_factor min_distance or dist > max_dist_factor max_distance: OUT_OF_RANGE
//   5              CHECK_VIEW: Xc . (R normal) < view_cos dist: VIEW_ANGLE
//   6              ratio = max_distance / dist; level = the smallest l >= 0 with scale[l] >= ratio, at most n_levels - 1
//                  (MapPoint::PredictScale's ceil(log ratio / log scale_factor) without libm: the two differ only where ratio equals a
//                  table entry: a stated deviation); radius = th scale[level]
//   7              the cell window of KeyFrame::GetFeaturesInArea: c0 = max(0, floor(((u - min_x) - radius) inv_w)),
//                  c1 = min(cols - 1, ceil(((u - min_x) + radius) inv_w)), none if c0 >= cols or c1 < 0; rows likewise.  Cell columns
//                  outermost, cell rows inside, the keypoints of a cell in ascending index.  A keypoint is IN THE WINDOW if
//                  |kp.u - u| < radius and |kp.v - v| < radius, and a CANDIDATE if also level - 1 <= octave <= level and, with
//                  CHECK_REPROJ, e2 inv_sigma2[octave] <= chi2: kp.ur < 0: e2 = du^2 + dv^2, chi2 = chi2_mono; otherwise
//                  e2 = du^2 + dv^2 + (ur - kp.ur)^2, chi2 = chi2_stereo.  The best candidate has the smallest Hamming distance; AMONG
//                  EQUAL DISTANCES THE FIRST IN WALK ORDER WINS (the strict < of ORB-SLAM2's loop).  None: NO_CANDIDATE.
//   8              best_dist > max_hamming: TOO_FAR (best_idx and best_dist are still handed out); otherwise OK
//   outputs        status, best_idx (the keypoint's index in its frame, -1: none), best_dist (-1: none), level (255 before step 6); for
//                  inspection u v ur dist radius (zeros before they are computed), n_window, n_candidates.
//
// Every sum is taken left to right as written below.  orb_search_query runs one query; orb_search_job_serial runs a job query after query
// (tools/hostonly/orb_search_host_check.cpp); orb_search_kernels.hip runs one query per lane from the same routines.  FP64, no libm
// except sqrt (floor and ceil are exact), -ffp-contract=off.
#pragma once
#include <float.h>
#include <math.h>

#include "cs_dense_lm.h"      // CS_HD, CS_UNROLL, CS_NOUNROLL
#include "cs_se3.h"           // quat_rotmat

namespace cs {

enum { ORB_MAX_LEVELS = 16, ORB_MAX_GRID = 128, ORB_DESC_WORDS = 8, ORB_KP_DOUBLES = 4, ORB_QUERY_DOUBLES = 8, ORB_INSPECT_DOUBLES = 5, ORB_LEVEL_NONE = 255 };

// (the values of cs_orb_search_status / cs_orb_search_flags of include/cubeslam_hip.h; orb_search_host.cpp asserts that they agree)
enum { ORB_OK = 0, ORB_SKIPPED = 1, ORB_BEHIND = 2, ORB_OUT_OF_IMAGE = 3, ORB_OUT_OF_RANGE = 4, ORB_VIEW_ANGLE = 5, ORB_NO_CANDIDATE = 6, ORB_TOO_FAR = 7 };
enum { ORB_CHECK_VIEW = 1, ORB_CHECK_REPROJ = 2 };

struct OrbParams {
  double min_dist_factor, max_dist_factor, view_cos, chi2_mono, chi2_stereo;
  int grid_cols, grid_rows;
};

// What is the same for every query into a frame, made once per frame by orb_frame_record.  kp_first: the frame's first SORTED keypoint
// in the set's arrays; cell_first: its first entry in the set's start table (cols rows + 1 entries, relative to kp_first).
struct OrbFrame {
  double cam[5], inv_w;                       // fx fy cx cy bf
  double bounds[4], inv_h, pad0;              // min_x max_x min_y max_y
  double scale[ORB_MAX_LEVELS], inv_sigma2[ORB_MAX_LEVELS];
  int n_levels, cols, rows, kp_first, cell_first, n_sorted, pad1, pad2;
};

// What is the same for every query of a job, made once per job by orb_job_record.  R row-major.
struct OrbJob {
  double R[9], t[3], s, th;
  int frame, max_hamming, flags, pad;
};

struct OrbQueryOut {
  double u, v, ur, dist, radius;             // the inspection form's
  int status, best_idx, best_dist, level, n_window, n_candidates;
};

CS_HD void orb_frame_record(const double* cam5, const double* bounds4, double scale_factor, int n_levels, int cols, int rows, int kp_first, int cell_first, OrbFrame& F) {
  CS_UNROLL
  for (int k = 0; k < 5; k++) F.cam[k] = cam5[k];
  CS_UNROLL
  for (int k = 0; k < 4; k++) F.bounds[k] = bounds4[k];
  F.inv_w = (double)cols / (bounds4[1] - bounds4[0]);
  F.inv_h = (double)rows / (bounds4[3] - bounds4[2]);
  F.pad0 = 0.0;
  double sc = 1.0;
  for (int l = 0; l < ORB_MAX_LEVELS; l++) {
    if (l > 0 && l < n_levels) sc = sc * scale_factor;
    F.scale[l] = sc;
    F.inv_sigma2[l] = 1.0 / (sc * sc);
  }
  F.n_levels = n_levels; F.cols = cols; F.rows = rows; F.kp_first = kp_first; F.cell_first = cell_first; F.n_sorted = 0; F.pad1 = 0; F.pad2 = 0;
}

// pose8: x y z qx qy qz qw s
CS_HD void orb_job_record(const double* pose8, double th, int frame, int max_hamming, int flags, OrbJob& J) {
  const double n = sqrt(pose8[3] * pose8[3] + pose8[4] * pose8[4] + pose8[5] * pose8[5] + pose8[6] * pose8[6]);
  quat_rotmat(pose8[6] / n, pose8[3] / n, pose8[4] / n, pose8[5] / n, J.R);
  CS_UNROLL
  for (int i = 0; i < 3; i++) J.t[i] = pose8[i];
  J.s = pose8[7]; J.th = th;
  J.frame = frame; J.max_hamming = max_hamming; J.flags = flags; J.pad = 0;
}

// The cell coordinate of a keypoint along one axis: floor((x - lo) inv + 0.5); -1 when it is outside 0 .. n - 1 (or not a number)
CS_HD int orb_keypoint_cell(double x, double lo, double inv, int n) {
  const double c = floor((x - lo) * inv + 0.5);
  return (c >= 0.0 && c <= (double)(n - 1)) ? (int)c : -1;
}

// The cells lo .. hi of GetFeaturesInArea along one axis (x = u - min_x or v - min_y); false: none
CS_HD bool orb_cell_range(double x, double radius, double inv, int n, int& lo, int& hi) {
  const double a = floor((x - radius) * inv), b = ceil((x + radius) * inv);
  const double top = (double)(n - 1);
  const double c0 = a > 0.0 ? a : 0.0;            // (a NaN: 0)
  const double c1 = b < top ? b : top;            // (a NaN: n - 1)
  lo = c0 <= top ? (int)c0 : n;
  hi = c1 >= 0.0 ? (int)c1 : -1;
  return lo < n && hi >= 0;
}

CS_HD int orb_hamming(const unsigned* a, const unsigned* b) {
  int d = 0;
  CS_UNROLL
  for (int k = 0; k < ORB_DESC_WORDS; k++) d += __builtin_popcount(a[k] ^ b[k]);
  return d;
}

// Steps 2 to 6 of the query q = X[3] normal[3] min_distance max_distance.  -> ORB_OK when the walk of step 7 is to follow
CS_HD int orb_query_project(const OrbFrame& F, const OrbJob& J, const OrbParams& prm, const double* q, OrbQueryOut& o) {
  double Xc[3];
  CS_UNROLL
  for (int i = 0; i < 3; i++) Xc[i] = J.s * (J.R[3 * i] * q[0] + J.R[3 * i + 1] * q[1] + J.R[3 * i + 2] * q[2]) + J.t[i];
  if (!(Xc[2] > 0.0)) return ORB_BEHIND;
  o.u = F.cam[0] * Xc[0] / Xc[2] + F.cam[2];
  o.v = F.cam[1] * Xc[1] / Xc[2] + F.cam[3];
  if (!(o.u >= F.bounds[0] && o.u < F.bounds[1] && o.v >= F.bounds[2] && o.v < F.bounds[3])) return ORB_OUT_OF_IMAGE;
  o.ur = o.u - F.cam[4] / Xc[2];
  o.dist = sqrt(Xc[0] * Xc[0] + Xc[1] * Xc[1] + Xc[2] * Xc[2]);
  if (o.dist < prm.min_dist_factor * q[6] || o.dist > prm.max_dist_factor * q[7]) return ORB_OUT_OF_RANGE;
  if (J.flags & ORB_CHECK_VIEW) {
    double Rn[3];
    CS_UNROLL
    for (int i = 0; i < 3; i++) Rn[i] = J.R[3 * i] * q[3] + J.R[3 * i + 1] * q[4] + J.R[3 * i + 2] * q[5];
    const double dot = Xc[0] * Rn[0] + Xc[1] * Rn[1] + Xc[2] * Rn[2];
    if (dot < prm.view_cos * o.dist) return ORB_VIEW_ANGLE;
  }
  const double ratio = q[7] / o.dist;
  int level = 0;
  CS_NOUNROLL
  for (int l = 0; l + 1 < F.n_levels; l++) level += F.scale[l] < ratio ? 1 : 0;      // (the table increases: the count IS the smallest l)
  o.level = level;
  o.radius = J.th * F.scale[level];
  return ORB_OK;
}

// Step 7 and 8.  start: the frame's cols rows + 1 entries; kp4 / orig / desc: the frame's sorted keypoints (u v ur octave; the index in
// the frame; ORB_DESC_WORDS words), all three from the frame's first sorted keypoint on.
CS_HD void orb_query_walk(const OrbFrame& F, const OrbJob& J, const OrbParams& prm, const int* start, const double* kp4, const int* orig, const unsigned* desc,
                          const unsigned* qd, OrbQueryOut& o) {
  int cx0, cx1, cy0, cy1;
  const bool any_x = orb_cell_range(o.u - F.bounds[0], o.radius, F.inv_w, F.cols, cx0, cx1);
  const bool any_y = orb_cell_range(o.v - F.bounds[2], o.radius, F.inv_h, F.rows, cy0, cy1);
  const double lvl = (double)o.level;
  const double is2_hi = F.inv_sigma2[o.level], is2_lo = F.inv_sigma2[o.level > 0 ? o.level - 1 : 0];
  const bool reproj = (J.flags & ORB_CHECK_REPROJ) != 0;
  int best = -1, best_dist = 257;
  if (any_x && any_y) {
    CS_NOUNROLL
    for (int cx = cx0; cx <= cx1; cx++) {
      const int a = start[cx * F.rows + cy0], b = start[cx * F.rows + cy1 + 1];      // one cell column of the window is one run
      CS_NOUNROLL
      for (int k = a; k < b; k++) {
        const double* kp = kp4 + (size_t)k * ORB_KP_DOUBLES;
        const double ku = kp[0], kv = kp[1], kur = kp[2], oct = kp[3];
        const double du = ku - o.u, dv = kv - o.v;
        if (!(fabs(du) < o.radius && fabs(dv) < o.radius)) continue;
        o.n_window++;
        if (!(oct >= lvl - 1.0 && oct <= lvl)) continue;
        if (reproj) {
          const bool stereo = kur >= 0.0;
          const double dr = o.ur - kur;
          const double e2m = du * du + dv * dv;
          const double e2 = stereo ? e2m + dr * dr : e2m;
          const double is2 = oct == lvl ? is2_hi : is2_lo;
          if (!(e2 * is2 <= (stereo ? prm.chi2_stereo : prm.chi2_mono))) continue;
        }
        o.n_candidates++;
        const int d = orb_hamming(qd, desc + (size_t)k * ORB_DESC_WORDS);
        if (d < best_dist) { best_dist = d; best = k; }      // (strict: of equals the first in walk order stays)
      }
    }
  }
  if (best < 0) { o.status = ORB_NO_CANDIDATE; return; }
  o.best_idx = orig[best];
  o.best_dist = best_dist;
  o.status = best_dist > J.max_hamming ? ORB_TOO_FAR : ORB_OK;
}

// One query: q (ORB_QUERY_DOUBLES), qd (ORB_DESC_WORDS), skip
CS_HD void orb_search_query(const OrbFrame& F, const OrbJob& J, const OrbParams& prm, const int* start, const double* kp4, const int* orig, const unsigned* desc,
                            const double* q, const unsigned* qd, bool skip, OrbQueryOut& o) {
  o.u = 0.0; o.v = 0.0; o.ur = 0.0; o.dist = 0.0; o.radius = 0.0;
  o.best_idx = -1; o.best_dist = -1; o.level = ORB_LEVEL_NONE; o.n_window = 0; o.n_candidates = 0;
  o.status = ORB_SKIPPED;
  if (skip) return;
  o.status = orb_query_project(F, J, prm, q, o);
  if (o.status != ORB_OK) return;
  orb_query_walk(F, J, prm, start, kp4, orig, desc, qd, o);
}

// Host code from here on.
// A frame's grid: the stable counting sort of its n keypoints (kp3: u v ur; octave; desc32: 32 bytes each) by cell = cx rows + cy.
// start: cols rows + 1 entries; kp4, orig, desc: room for n sorted keypoints.  -> how many are in a cell (the others are dropped)
static inline int orb_pack_frame(const OrbFrame& F, int n, const double* kp3, const int* octave, const unsigned char* desc32, int* start, double* kp4, int* orig, unsigned* desc) {
  const int cells = F.cols * F.rows;
  for (int c = 0; c <= cells; c++) start[c] = 0;
  auto cell_of = [&](int i) {
    const int cx = orb_keypoint_cell(kp3[3 * (size_t)i], F.bounds[0], F.inv_w, F.cols), cy = orb_keypoint_cell(kp3[3 * (size_t)i + 1], F.bounds[2], F.inv_h, F.rows);
    return (cx < 0 || cy < 0) ? -1 : cx * F.rows + cy;
  };
  for (int i = 0; i < n; i++) { const int c = cell_of(i); if (c >= 0) start[c + 1]++; }
  for (int c = 0; c < cells; c++) start[c + 1] += start[c];
  const int n_sorted = start[cells];
  for (int i = 0; i < n; i++) {                                  // start[c] is the cell's cursor in this pass
    const int c = cell_of(i);
    if (c < 0) continue;
    const int at = start[c]++;
    kp4[4 * (size_t)at] = kp3[3 * (size_t)i]; kp4[4 * (size_t)at + 1] = kp3[3 * (size_t)i + 1]; kp4[4 * (size_t)at + 2] = kp3[3 * (size_t)i + 2];
    kp4[4 * (size_t)at + 3] = (double)octave[i];
    orig[at] = i;
    for (int w = 0; w < ORB_DESC_WORDS; w++) {
      const unsigned char* b = desc32 + 32 * (size_t)i + 4 * w;
      desc[ORB_DESC_WORDS * (size_t)at + w] = (unsigned)b[0] | ((unsigned)b[1] << 8) | ((unsigned)b[2] << 16) | ((unsigned)b[3] << 24);
    }
  }
  for (int c = cells; c > 0; c--) start[c] = start[c - 1];      // every start moved to its cell's end: shift them back
  start[0] = 0;
  return n_sorted;
}

static inline void orb_pack_descriptor(const unsigned char* desc32, unsigned* words) {
  for (int w = 0; w < ORB_DESC_WORDS; w++)
    words[w] = (unsigned)desc32[4 * w] | ((unsigned)desc32[4 * w + 1] << 8) | ((unsigned)desc32[4 * w + 2] << 16) | ((unsigned)desc32[4 * w + 3] << 24);
}

// One job, query after query.  q8: n x ORB_QUERY_DOUBLES; qdesc: n x ORB_DESC_WORDS; the outputs n each (insp5: n x 5 or null).
// -> the number of OK queries
static inline int orb_search_job_serial(const OrbFrame& F, const OrbJob& J, const OrbParams& prm, const int* start, const double* kp4, const int* orig, const unsigned* desc, int n,
                                        const double* q8, const unsigned* qdesc, const unsigned char* skip, unsigned char* status, int* best_idx, int* best_dist,
                                        unsigned char* level, double* insp5, int* n_window, int* n_candidates) {
  int n_ok = 0;
  for (int i = 0; i < n; i++) {
    OrbQueryOut o;
    orb_search_query(F, J, prm, start, kp4, orig, desc, q8 + (size_t)i * ORB_QUERY_DOUBLES, qdesc + (size_t)i * ORB_DESC_WORDS, skip[i] != 0, o);
    status[i] = (unsigned char)o.status; best_idx[i] = o.best_idx; best_dist[i] = o.best_dist; level[i] = (unsigned char)o.level;
    if (insp5) { double* p = insp5 + 5 * (size_t)i; p[0] = o.u; p[1] = o.v; p[2] = o.ur; p[3] = o.dist; p[4] = o.radius; }
    if (n_window) n_window[i] = o.n_window;
    if (n_candidates) n_candidates[i] = o.n_candidates;
    n_ok += o.status == ORB_OK ? 1 : 0;
  }
  return n_ok;
}

}  // namespace cs
