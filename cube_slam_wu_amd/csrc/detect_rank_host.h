// detect_rank_host.h -- the rules every sweep path of detect_host.cpp shares, once each: the slot numbering's inverse, the 9-value
// candidate row, fuse_normalize_scores_v2 and the exact final ranking of a box (tie order is part of the contract: the output is
// byte-identical to the reference), the geometry of a job descriptor, the cs_cuboid record of a winner, the host's rebuild of a winner's
// corners, and the writers of a box's records and count into the caller's output (OutView).
// Plain C++: nothing here launches a kernel or calls a HIP function (tests/test_detect_rank_host_cpu.py builds it with the host compiler).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>
#include <vector>

#include "../../include/cubeslam_hip.h"
#include "detect_types.h"

namespace cs_dh {

// sin and cos stay two libm calls (the reference's default Debug build makes two calls; glibc's fused
// sincos() rounds differently in ~1.4e-3 of arguments).  The volatile copy keeps compilers from merging.
inline double h_sin(double x) { volatile double v = x; return std::sin(v); }
inline double h_cos(double x) { volatile double v = x; return std::cos(v); }

struct FrameIn {
  double K[9], invK[9], R[9], t[3];
  int img_w, img_h, n_boxes, n_lines;
  std::vector<double> boxes;     // n x 5
  std::vector<double> lines;     // M x 4, left-to-right aligned (object_3d_util.cpp:246-258)
  std::vector<long long> map_offs;  // per (box, k): float offset into the device map pool (-1 = absent)
  std::vector<cs_roi> rois;      // n x 3
  std::vector<int> n_heights;    // n
};

// ---- slot numbering: slot = slot_off + ((rp*Y + yaw)*T + top)*2 + (config-1)  (detect_types.h) ----------------------------------
struct SlotRef { int cfg, t, rp, y; };   // config (1 / 2), top-edge sample, roll/pitch sample, yaw sample
inline SlotRef decode_slot(const cs::JobDesc& jd, long long slot) {
  const long long local = slot - jd.slot_off, rest = local >> 1;
  const int t = (int)(rest % jd.T), ry = (int)(rest / jd.T), rp = ry / jd.Y;
  return SlotRef{(int)(local & 1) + 1, t, rp, ry - rp * jd.Y};
}

// one row of the reference's candidate table (box_proposal_detail.cpp:677-693)
inline void candidate_row9(const SlotRef& s, int flag, double dist_err, double angle_err, double yaw, int down_expand, double roll, double pitch, double r9[9]) {
  r9[0] = s.cfg; r9[1] = flag & cs::CAND_VP_MASK; r9[2] = yaw; r9[3] = s.t; r9[4] = dist_err; r9[5] = angle_err; r9[6] = down_expand;
  r9[7] = roll; r9[8] = pitch;
}

// fuse_normalize_scores_v2 (object_3d_util.cpp:726-837)
inline void fuse_scores(const double* dist, const double* angle, int n, double w_angle, std::vector<int>& keep, std::vector<double>& score) {
  keep.clear();
  if (n > 4) {
    int bn = (int)std::round(float(n) / 3.0 * 2.0);
    // std::partial_sort of the ids by value (sort_indexes, matrix_utils.cpp:327-335).  The keys travel with the ids: the
    // algorithm makes the same comparisons and moves as on a bare id array (so ties resolve identically), without the
    // indirect loads
    struct KI { double key; int id; };
    std::vector<KI> ds(n), as(n);
    for (int i = 0; i < n; i++) { ds[i] = KI{dist[i], i}; as[i] = KI{angle[i], i}; }
    auto by_key = [](const KI& a, const KI& b) { return a.key < b.key; };
    std::partial_sort(ds.begin(), ds.begin() + bn, ds.end(), by_key);
    std::partial_sort(as.begin(), as.begin() + bn, as.end(), by_key);
    std::vector<int> di(bn), ai(bn);
    for (int i = 0; i < bn; i++) { di[i] = ds[i].id; ai[i] = as[i].id; }
    std::vector<int> dk(di.begin(), di.begin() + bn - 1);
    if (angle[ai[bn - 1]] > angle[ai[bn - 2]]) {
      // sort both id lists + set_intersection (:771-776) = the ids present in both, ascending: one pass over a marker array
      std::vector<unsigned char> in(n, 0);
      for (int i = 0; i < bn - 1; i++) { in[di[i]] |= 1; in[ai[i]] |= 2; }
      for (int id = 0; id < n; id++) if (in[id] == 3) keep.push_back(id);
    } else {
      keep = dk;
    }
  } else {
    keep.resize(n);
    std::iota(keep.begin(), keep.end(), 0);
  }
  int k = (int)keep.size();
  double dmin = 1e6, dmax = -1, amin = 1e6, amax = -1;
  for (int i = 0; i < k; i++) {
    double d = dist[keep[i]], a = angle[keep[i]];
    dmin = std::min(dmin, d); dmax = std::max(dmax, d);
    amin = std::min(amin, a); amax = std::max(amax, a);
  }
  score.resize(k);
  if (k > 1) {
    bool na = (amax - amin) > 0;
    for (int i = 0; i < k; i++) {
      double d = (dist[keep[i]] - dmin) / (dmax - dmin);
      double a = angle[keep[i]];
      if (na) a = (a - amin) / (amax - amin);
      score[i] = (d + w_angle * a) / (1 + w_angle);
    }
  } else {
    for (int i = 0; i < k; i++) score[i] = (dist[keep[i]] + w_angle * angle[keep[i]]) / (1 + w_angle);
  }
}

// ---- the exact final ranking of one box (box_proposal_detail.cpp:766-838) --------------------------------------------------------
// The compacted columns of one height sample of the box, wherever the caller keeps them.  keep / score: fuse_scores' products when the
// caller has them already (the round path's host ranking retains them for the debug getters), else null and computed here.
struct HeightCols {
  const double *dist, *angle, *skew;
  const int* flag;
  const long long* slot;
  int V;
  const std::vector<int>* keep = nullptr;
  const std::vector<double>* score = nullptr;
};
struct RankWeights { double w_angle, w_skew, nominal_skew, max_cut_skew; };   // weight_vp_angle, weight_skew_error, nominal_skew_ratio, max_cut_skew
// the ranking's parameters out of the detector's: the host's and the kernels' form
inline RankWeights rank_weights(const cs_detect_params& P) { return RankWeights{P.weight_vp_angle, P.weight_skew_error, P.nominal_skew_ratio, P.max_cut_skew}; }
inline cs::RankParams rank_params(const cs_detect_params& P, const cs::SweepParams& sp) {
  return cs::RankParams{P.weight_vp_angle, P.weight_skew_error, P.nominal_skew_ratio, P.max_cut_skew, P.max_cuboid_num, sp.short_sq_bound};
}
struct ExactWinner {
  long long slot;
  int h, cand;             // height sample, candidate index inside it
  double score, dist, angle;
  int flag;                // masked: vp_1_position
};
// Winners in order (at most kmax); returns the last kept slot of the last height sample, -1 when it kept nothing (what the reference's
// last set_cam_pose() of the box follows, :727-737).  Proposals are gathered height-major in `keep` order and ranked by std::partial_sort over an
// index array on comb[a] < comb[c]: the comparison sequence decides ties, so these container shapes stay.
inline long long exact_rank_box(const HeightCols* cols, int nh, const RankWeights& W, int kmax, std::vector<ExactWinner>& winners) {
  struct HP { int h, cand; double score, skew; };
  std::vector<HP> props;
  std::vector<int> keep_own;
  std::vector<double> score_own;
  long long last_slot = -1;
  for (int h = 0; h < nh; h++) {
    const HeightCols& c = cols[h];
    if (!c.keep) fuse_scores(c.dist, c.angle, c.V, W.w_angle, keep_own, score_own);
    const std::vector<int>& keep = c.keep ? *c.keep : keep_own;
    const std::vector<double>& score = c.keep ? *c.score : score_own;
    if (h == nh - 1) last_slot = keep.empty() ? -1 : c.slot[keep.back()];
    for (size_t z = 0; z < keep.size(); z++) {
      if (c.flag[keep[z]] & cs::CAND_NEG_SCALE) continue;  // :766
      props.push_back(HP{h, keep[z], score[z], c.skew[keep[z]]});
    }
  }
  const int n = (int)props.size(), kk = std::min(kmax, n);
  std::vector<double> comb(n);
  for (int i = 0; i < n; i++) {
    double skew_error = W.w_skew * std::max(props[i].skew - W.nominal_skew, 0.0);
    if (props[i].skew > W.max_cut_skew) skew_error = 100;
    comb[i] = props[i].score + W.w_skew * skew_error;  // weight applied twice (:813,:820)
  }
  std::vector<int> idx(n);
  std::iota(idx.begin(), idx.end(), 0);
  std::partial_sort(idx.begin(), idx.begin() + kk, idx.end(), [&comb](int a, int c) { return comb[a] < comb[c]; });
  winners.clear();
  for (int r = 0; r < kk; r++) {
    const HP& hp = props[idx[r]];
    const HeightCols& c = cols[hp.h];
    winners.push_back(ExactWinner{c.slot[hp.cand], hp.h, hp.cand, hp.score, c.dist[hp.cand], c.angle[hp.cand], c.flag[hp.cand] & cs::CAND_VP_MASK});
  }
  return last_slot;
}

// ---- job descriptors: what every job builder sets identically for (box, height sample k) of a frame.  Y, T, RP, the offsets and
// `frame` stay with each path. -----------------------------------------------------------------------------------------------------
inline void fill_job_geometry(cs::JobDesc& jd, const FrameIn& F, int box, int k, int rp_off) {
  std::memset(&jd, 0, sizeof(jd));
  const double* bb = &F.boxes[5 * box];
  const cs_roi& roi = F.rois[3 * box + k];
  int left = bb[0], top = bb[1], w = bb[2], h = bb[3];
  int right = left + bb[2];
  int he = h + roi.down_expand;
  jd.g.left = left; jd.g.top = top; jd.g.right = right; jd.g.down = top + he;
  jd.g.el = roi.left; jd.g.et = roi.top; jd.g.er = roi.left + roi.width; jd.g.eb = roi.top + roi.height;
  jd.map_w = roi.width; jd.down_expand = roi.down_expand;
  jd.box = box; jd.hid = k; jd.map_off = F.map_offs[3 * box + k]; jd.rp_off = rp_off;
  jd.diag = std::sqrt(double(w * w + he * he));
}

// ---- records ---------------------------------------------------------------------------------------------------------------------
// Build one cs_cuboid from the winner's corners (box_proposal_detail.cpp:740-798, object_3d_util.cpp:941-1011).
inline void finish_cuboid(const FrameIn& F, const cs::RpPose& pose, const double* rows9, const double* corners16, const double raw_euler[3],
                          bool sample_rp, double normalized_error, cs_cuboid& o) {
  std::memset(&o, 0, sizeof(o));
  cs::V2 c[8];
  for (int i = 0; i < 8; i++) c[i] = cs::v2(corners16[i], corners16[8 + i]);
  cs::lift_to_3d(c, pose.R, pose.t, F.invK, pose.plane, o.pos, o.scale);
  o.rotY = rows9[2];
  o.box_config_type[0] = rows9[0]; o.box_config_type[1] = rows9[1];
  static const int left_ids[8] = {6, 5, 8, 7, 2, 3, 4, 1}, right_ids[8] = {5, 6, 7, 8, 3, 2, 1, 4};
  const int* ids = (rows9[1] == 1) ? left_ids : right_ids;
  for (int i = 0; i < 8; i++) {
    o.box_corners_2d[i] = (int)corners16[ids[i] - 1];
    o.box_corners_2d[8 + i] = (int)corners16[8 + ids[i] - 1];
  }
  // compute3D_BoxCorner (object_3d_util.cpp:59-73) with similarityTransformation (:15-44)
  static const double body[3][8] = {{1, 1, -1, -1, 1, 1, -1, -1}, {1, -1, -1, 1, 1, -1, -1, 1}, {-1, -1, -1, -1, 1, 1, 1, 1}};
  double cr = h_cos(o.rotY), sr = h_sin(o.rotY);
  double rot[3][3] = {{cr, -sr, 0}, {sr, cr, 0}, {0, 0, 1}};
  double S[4][4] = {{0}};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) S[i][j] = rot[i][j] * o.scale[j];
    S[i][3] = o.pos[i];
  }
  S[3][3] = 1;
  for (int k = 0; k < 8; k++) {
    double p[4] = {body[0][k], body[1][k], body[2][k], 1.0}, w[4];
    for (int i = 0; i < 4; i++) w[i] = ((S[i][0] * p[0] + S[i][1] * p[1]) + S[i][2] * p[2]) + S[i][3] * p[3];
    for (int i = 0; i < 3; i++) o.box_corners_3d_world[8 * i + k] = w[i] / w[3];
  }
  o.edge_distance_error = rows9[4];
  o.edge_angle_error = rows9[5];
  o.normalized_error = normalized_error;
  o.skew_ratio = std::max(o.scale[0], o.scale[1]) / std::min(o.scale[0], o.scale[1]);
  o.down_expand_height = rows9[6];
  if (sample_rp) {
    o.camera_roll_delta = rows9[7] - raw_euler[0];
    o.camera_pitch_delta = rows9[8] - raw_euler[1];
  }
}

// The corners of proposal s of job jd, rebuilt on the host (the lean roll/pitch path's tie winners): the vanishing points of pose matrix
// A = KinvR and the yaw sample's (cos, sin) -- vp_points_kernel's arithmetic, operation for operation -- then build_corners at top-edge sample top_x.
inline void host_corners16(const double* A, double cy, double sy, const cs::JobDesc& jd, const SlotRef& s, double top_x, double short_sq_bound, double c16[16]) {
  const double dd[3][3] = {{cy, sy, 0.0}, {-sy, cy, 0.0}, {0.0, 0.0, 1.0}};
  cs::V2 vp[3], c8[8];
  for (int k = 0; k < 3; k++) {
    double h[3];
    for (int i = 0; i < 3; i++) h[i] = (A[3 * i] * dd[k][0] + A[3 * i + 1] * dd[k][1]) + A[3 * i + 2] * dd[k][2];
    vp[k] = cs::v2(h[0] / h[2], h[1] / h[2]);
  }
  for (auto& c : c8) c = cs::v2(0.0, 0.0);
  (void)cs::build_corners(jd.g, vp[0], vp[1], vp[2], top_x, s.cfg, short_sq_bound, c8);
  for (int k = 0; k < 8; k++) { c16[k] = c8[k].x; c16[8 + k] = c8[k].y; }
}

inline void set_caller_rect(const FrameIn& F, int box, cs_cuboid& o) {
  const double* bb = &F.boxes[5 * box];
  o.rect_detect_2d[0] = (int)bb[0]; o.rect_detect_2d[1] = (int)bb[1]; o.rect_detect_2d[2] = (int)bb[2]; o.rect_detect_2d[3] = (int)bb[3];
}

// a winner the host knows by slot: candidate row -> finish_cuboid -> the caller's rectangle.  `pose` is the roll/pitch sample s.rp of the
// frame, `yaw` the value of yaw sample s.y of the job
inline void write_winner_record(const FrameIn& F, const cs::JobDesc& jd, const SlotRef& s, int flag, double dist_err, double angle_err, double yaw,
                                const cs::RpPose& pose, const double* corners16, const double raw_euler[3], bool sample_rp, double normalized_error, cs_cuboid& o) {
  double r9[9];
  candidate_row9(s, flag, dist_err, angle_err, yaw, jd.down_expand, pose.roll, pose.pitch, r9);
  finish_cuboid(F, pose, r9, corners16, raw_euler, sample_rp, normalized_error, o);
  set_caller_rect(F, jd.box, o);
}

// a record record_kernel wrote: complete but for the caller's rectangle
inline void copy_device_record(const FrameIn& F, int box, const cs_cuboid& rec, cs_cuboid& o) {
  o = rec;
  set_caller_rect(F, box, o);
}

// ---- the caller's output: KMAX records and one count per (frame, box of max_boxes) ---------------------------------------------------
struct OutView {
  cs_cuboid* out = nullptr; int* out_counts = nullptr; int max_boxes = 0, kmax = 0;
  cs_cuboid& rec(int f, int box, int r) const { return out[((size_t)f * max_boxes + box) * kmax + r]; }
  int& count(int f, int box) const { return out_counts[(size_t)f * max_boxes + box]; }
};

// The exact winners `wl` of a box into its records and count.  jobs: the box's jobs (one per height sample); yaw: the path's yaw table
// (jd.yaw_off indexes it); cams[rp].pose: the frame's roll/pitch sample poses; corners_of(r, jd, s): the 16 corner doubles of winner r.
template <class Cams, class CornersOf>
inline void write_exact_winners(const OutView& O, const FrameIn& F, const cs::JobDesc* jobs, const std::vector<ExactWinner>& wl, const double* yaw, const Cams& cams,
                                const double raw_euler[3], bool sample_rp, CornersOf corners_of) {
  const int f = jobs[0].frame, box = jobs[0].box;
  for (size_t r = 0; r < wl.size(); r++) {
    const ExactWinner& w = wl[r];
    const cs::JobDesc& jd = jobs[w.h];
    const SlotRef s = decode_slot(jd, w.slot);
    write_winner_record(F, jd, s, w.flag, w.dist, w.angle, yaw[jd.yaw_off + s.y], cams[s.rp].pose, corners_of(r, jd, s), raw_euler, sample_rp, w.score, O.rec(f, box, (int)r));
  }
  O.count(f, box) = (int)wl.size();
}
// the corner source of winners whose corners lie one after the other from corners16
inline auto corners_at(const double* corners16) { return [corners16](size_t r, const cs::JobDesc&, const SlotRef&) { return corners16 + 16 * r; }; }

// The nw records record_kernel wrote for box `box` of frame f, and the count
inline void write_device_records(const OutView& O, const FrameIn& F, int f, int box, const cs_cuboid* recs, int nw) {
  for (int r = 0; r < nw; r++) copy_device_record(F, box, recs[r], O.rec(f, box, r));
  O.count(f, box) = nw;
}

}  // namespace cs_dh
