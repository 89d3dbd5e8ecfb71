// detect_rank_host_check.cpp -- the detector host's shared rules (cube_slam_wu_amd/csrc/detect_rank_host.h) on their own, without a GPU:
// decode_slot against the slot numbering, and the properties of exact_rank_box on the shapes where a ranking goes wrong (no candidates,
// no cut, a cut through equal keys, a height sample that is all flagged, fewer proposals than winners asked for, three height samples).
// Then the camera cache (detect_cam_host.h: Euler round trip over every branch of the quaternion step, make_cam against K R^-1 in long double, the
// 25 roll/pitch sample poses), host_corners16 against the vanishing-point formula restated here, and the two record writers against the output
// layout (records and counts at rec(f, box, r) / count(f, box), nothing beside them written).
// tests/test_detect_rank_host_cpu.py builds it with the host compiler and the sanitizers and runs it.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../cube_slam_wu_amd/csrc/detect_cam_host.h"
#include "../../cube_slam_wu_amd/csrc/detect_rank_host.h"

using namespace cs_dh;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static unsigned long long g_seed = 12345;
static double rnd() { g_seed = g_seed * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(g_seed >> 11) / 9007199254740992.0; }

static void check_decode() {
  cs::JobDesc jd{};
  jd.RP = 3; jd.Y = 5; jd.T = 4; jd.slot_off = 98304 + 26;
  int n = 0;
  for (int rp = 0; rp < jd.RP; rp++)
    for (int y = 0; y < jd.Y; y++)
      for (int t = 0; t < jd.T; t++)
        for (int cfg = 1; cfg <= 2; cfg++, n++) {
          const long long slot = jd.slot_off + (((long long)rp * jd.Y + y) * jd.T + t) * 2 + (cfg - 1);
          const SlotRef s = decode_slot(jd, slot);
          CHECK(s.cfg == cfg && s.t == t && s.rp == rp && s.y == y, "slot %lld -> cfg %d t %d rp %d y %d", slot, s.cfg, s.t, s.rp, s.y);
        }
  CHECK(n == 3 * 5 * 4 * 2, "%d slots", n);
}

struct Height {
  std::vector<double> dist, angle, skew;
  std::vector<int> flag;
  std::vector<long long> slot;
};
static Height make_height(int V, long long slot0, bool equal_dist, bool all_flagged) {
  Height H;
  for (int i = 0; i < V; i++) {
    H.dist.push_back(equal_dist ? 2.5 : 10.0 * rnd());
    H.angle.push_back(rnd());
    H.skew.push_back(0.5 + 4.0 * rnd());                                   // some beyond max_cut_skew = 3
    H.flag.push_back((1 + i % 2) | (all_flagged || i % 7 == 3 ? cs::CAND_NEG_SCALE : 0));
    H.slot.push_back(slot0 + 3 * i);
  }
  return H;
}

static void check_rank(const char* name, const std::vector<Height>& hs, int kmax) {
  const RankWeights W{0.8, 1.5, 1.0, 3.0};
  const int nh = (int)hs.size();
  std::vector<HeightCols> cols(nh), cols_pre(nh);
  std::vector<std::vector<int>> keep(nh);
  std::vector<std::vector<double>> score(nh);
  int proposals = 0;
  for (int h = 0; h < nh; h++) {
    const Height& H = hs[h];
    const int V = (int)H.dist.size();
    cols[h] = HeightCols{H.dist.data(), H.angle.data(), H.skew.data(), H.flag.data(), H.slot.data(), V};
    fuse_scores(H.dist.data(), H.angle.data(), V, W.w_angle, keep[h], score[h]);
    cols_pre[h] = cols[h]; cols_pre[h].keep = &keep[h]; cols_pre[h].score = &score[h];
    for (int id : keep[h]) proposals += (H.flag[id] & cs::CAND_NEG_SCALE) ? 0 : 1;
  }
  std::vector<ExactWinner> win, win_pre;
  const long long last = exact_rank_box(cols.data(), nh, W, kmax, win);
  const long long last_pre = exact_rank_box(cols_pre.data(), nh, W, kmax, win_pre);
  CHECK((int)win.size() == std::min(kmax, proposals), "%s: %d winners, %d proposals, kmax %d", name, (int)win.size(), proposals, kmax);
  const long long want_last = (nh == 0 || keep[nh - 1].empty()) ? -1 : hs[nh - 1].slot[keep[nh - 1].back()];
  CHECK(last == want_last && last_pre == want_last, "%s: last slot %lld / %lld, want %lld", name, last, last_pre, want_last);
  CHECK(win.size() == win_pre.size(), "%s: precomputed keep gives %d winners", name, (int)win_pre.size());
  double prev = 0;
  for (size_t r = 0; r < win.size(); r++) {
    const ExactWinner& w = win[r];
    CHECK(w.h >= 0 && w.h < nh, "%s: winner %d height %d", name, (int)r, w.h);
    const Height& H = hs[w.h];
    bool kept = false;
    double sc = 0;
    for (size_t z = 0; z < keep[w.h].size(); z++) if (keep[w.h][z] == w.cand) { kept = true; sc = score[w.h][z]; }
    CHECK(kept, "%s: winner %d (height %d, candidate %d) is not in keep", name, (int)r, w.h, w.cand);
    CHECK(!(H.flag[w.cand] & cs::CAND_NEG_SCALE), "%s: winner %d is a flagged candidate", name, (int)r);
    CHECK(w.slot == H.slot[w.cand] && w.dist == H.dist[w.cand] && w.angle == H.angle[w.cand] && w.flag == (H.flag[w.cand] & cs::CAND_VP_MASK), "%s: winner %d columns", name, (int)r);
    CHECK(w.score == sc || (w.score != w.score && sc != sc), "%s: winner %d score", name, (int)r);
    double skew_error = W.w_skew * std::max(H.skew[w.cand] - W.nominal_skew, 0.0);
    if (H.skew[w.cand] > W.max_cut_skew) skew_error = 100;
    const double comb = w.score + W.w_skew * skew_error;
    if (r > 0) CHECK(!(comb < prev), "%s: comb decreases at winner %d (%g after %g)", name, (int)r, comb, prev);
    prev = comb;
    if (r < win_pre.size()) CHECK(win_pre[r].slot == w.slot && win_pre[r].h == w.h && win_pre[r].cand == w.cand, "%s: precomputed keep, winner %d differs", name, (int)r);
  }
}


// ---- camera cache ----------------------------------------------------------------------------------------------------------------
static const double K_CAM[9] = {718.856, 0.0, 607.19, 0.0, 718.856, 185.22, 0.0, 0.0, 1.0};
// a camera looking along the world's y axis, heading a, tilted down by t (columns: right, down, forward)
static void look_rotation(double a, double t, double R[9]) {
  const double f[3] = {std::sin(a) * std::cos(t), std::cos(a) * std::cos(t), -std::sin(t)}, r[3] = {std::cos(a), -std::sin(a), 0.0};
  const double d[3] = {f[1] * r[2] - f[2] * r[1], f[2] * r[0] - f[0] * r[2], f[0] * r[1] - f[1] * r[0]};
  for (int i = 0; i < 3; i++) { R[3 * i] = r[i]; R[3 * i + 1] = d[i]; R[3 * i + 2] = f[i]; }
}

static void check_euler_round_trip() {
  // roll, yaw in (-pi, pi), pitch in (-pi/2, pi/2): the ZYX angles of a rotation are unique there.  1e-12: a dozen roundings on values of
  // size one, away from the gimbal lock (|pitch| <= 1.2)
  const double rolls[] = {-3.0, -1.5, -0.4, 0.0, 0.3, 1.2, 3.0}, pitches[] = {-1.2, -0.5, 0.0, 0.4, 1.2}, yaws[] = {-3.0, -2.0, -0.7, 0.0, 1.0, 2.5, 3.1};
  int branch[4] = {0, 0, 0, 0};      // positive trace; largest diagonal entry 0, 1, 2
  for (double r : rolls)
    for (double p : pitches)
      for (double y : yaws) {
        double R[9], e[3];
        euler_to_rot(r, p, y, R);
        if (R[0] + R[4] + R[8] > 0.0) branch[0]++;
        else { int i = 0; if (R[4] > R[0]) i = 1; if (R[8] > R[4 * i]) i = 2; branch[1 + i]++; }
        rot_to_euler(R, e);
        CHECK(std::abs(e[0] - r) < 1e-12 && std::abs(e[1] - p) < 1e-12 && std::abs(e[2] - y) < 1e-12, "euler (%g %g %g) -> (%.17g %.17g %.17g)", r, p, y, e[0], e[1], e[2]);
      }
  CHECK(branch[0] > 0 && branch[1] > 0 && branch[2] > 0 && branch[3] > 0, "quaternion branches taken: %d %d %d %d", branch[0], branch[1], branch[2], branch[3]);
}

static void check_make_cam(CamCache& raw) {
  double R[9];
  look_rotation(0.1, 3.0 / 180.0 * CS_PI, R);
  const double t[3] = {0.3, -0.6, 1.65};
  make_cam(K_CAM, R, t, raw);
  // K R^-1 in long double (cofactor inverse)
  long double Rl[9], inv[9];
  for (int i = 0; i < 9; i++) Rl[i] = R[i];
  auto cof = [&](int i, int j) { int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3; return Rl[3 * i1 + j1] * Rl[3 * i2 + j2] - Rl[3 * i1 + j2] * Rl[3 * i2 + j1]; };
  const long double det = Rl[0] * cof(0, 0) + Rl[1] * cof(0, 1) + Rl[2] * cof(0, 2);
  for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) inv[3 * i + j] = cof(j, i) / det;
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      long double want = 0;
      for (int k = 0; k < 3; k++) want += (long double)K_CAM[3 * i + k] * inv[3 * k + j];
      // 1e-12 of K's largest entry: some ten roundings of the double path on terms no larger than it, with room
      CHECK(std::abs((double)(want - raw.pose.KinvR[3 * i + j])) < 1e-12 * 718.856, "KinvR[%d][%d] = %.17g, want %.17Lg", i, j, raw.pose.KinvR[3 * i + j], want);
    }
  CHECK(raw.pose.plane[0] == R[6] && raw.pose.plane[1] == R[7] && raw.pose.plane[2] == R[8] && raw.pose.plane[3] == t[2], "ground plane row %g %g %g %g", raw.pose.plane[0], raw.pose.plane[1], raw.pose.plane[2], raw.pose.plane[3]);
  CHECK(raw.pose.roll == raw.euler[0] && raw.pose.pitch == raw.euler[1] && raw.cam_yaw == raw.euler[2], "raw pose angles");
  CHECK(std::memcmp(raw.pose.R, R, sizeof(R)) == 0 && std::memcmp(raw.pose.t, t, sizeof(t)) == 0, "R, t copied");
}

// The sample lists are linespace's: from raw - 6 degrees in steps of 3 while <= raw + 6 degrees, so five entries where the fourth addition does
// not round past the end and four where it does (counted here by the same loop).  want: the number of poses this camera is known to give.
static void check_sample_poses(const CamCache& raw, std::vector<CamCache>& rp, int want) {
  const double t[3] = {raw.pose.t[0], raw.pose.t[1], raw.pose.t[2]}, six = 6.0 / 180.0 * CS_PI, step = 3.0 / 180.0 * CS_PI;
  rp.clear();
  sample_rp_poses(K_CAM, t, raw, rp);
  int nr = 0, np = 0;
  for (double a = raw.euler[0] - six; a <= raw.euler[0] + six; a += step) nr++;
  for (double a = raw.euler[1] - six; a <= raw.euler[1] + six; a += step) np++;
  CHECK((int)rp.size() == nr * np && (int)rp.size() == want && nr >= 4 && np >= 4, "%d sample poses, lists of %d and %d, want %d", (int)rp.size(), nr, np, want);
  if ((int)rp.size() != nr * np) return;
  CHECK(rp[0].pose.roll == raw.euler[0] - six && rp[0].pose.pitch == raw.euler[1] - six, "first sample is raw - 6 degrees");
  for (int i = 0; i < nr; i++)
    for (int j = 0; j < np; j++) {
      const CamCache& c = rp[np * i + j];
      CHECK(c.pose.roll == rp[np * i].pose.roll && c.pose.pitch == rp[j].pose.pitch, "sample %d %d: roll-major grid", i, j);
      CHECK(std::abs(c.pose.roll - (rp[0].pose.roll + i * step)) < 1e-14 && std::abs(c.pose.pitch - (rp[0].pose.pitch + j * step)) < 1e-14, "sample %d %d: steps of 3 degrees", i, j);
      // the pose is that of the sample angles at the raw yaw (the stored roll / pitch are the sample angles themselves, not the recovered ones)
      CHECK(std::abs(c.euler[0] - c.pose.roll) < 1e-12 && std::abs(c.euler[1] - c.pose.pitch) < 1e-12 && std::abs(c.euler[2] - raw.euler[2]) < 1e-12, "sample %d %d: rotation of its angles", i, j);
      CHECK(c.pose.plane[3] == t[2], "sample %d %d: camera height", i, j);
    }
}

// ---- host_corners16 against the vanishing points restated: vp_k = dehomogenised KinvR * column k of Rz(yaw) ------------------------
static int check_host_corners(const CamCache& cam, const cs::JobDesc& jd, double c16_out[16], SlotRef& s_out, double& yaw_out) {
  int accepted = 0;
  const double* A = cam.pose.KinvR;
  for (int yi = 0; yi < 96; yi++) {
    const double yaw = -CS_PI + yi * (2 * CS_PI / 96), cy = h_cos(yaw), sy = h_sin(yaw);
    const double col[3][3] = {{cy, sy, 0.0}, {-sy, cy, 0.0}, {0.0, 0.0, 1.0}};
    cs::V2 vp[3];
    for (int k = 0; k < 3; k++) {
      double h[3];
      for (int i = 0; i < 3; i++) h[i] = (A[3 * i] * col[k][0] + A[3 * i + 1] * col[k][1]) + A[3 * i + 2] * col[k][2];
      vp[k] = cs::v2(h[0] / h[2], h[1] / h[2]);
    }
    for (int t = 0; t < jd.T; t++)
      for (int cfg = 1; cfg <= 2; cfg++) {
        const double top_x = jd.g.left + 5 + 19 * t;
        cs::V2 c8[8];
        for (auto& c : c8) c = cs::v2(0.0, 0.0);
        const int ok = cs::build_corners(jd.g, vp[0], vp[1], vp[2], top_x, cfg, 400.0, c8);
        const SlotRef s{cfg, t, 0, yi % jd.Y};
        double c16[16];
        host_corners16(A, cy, sy, jd, s, top_x, 400.0, c16);
        bool same = true;
        for (int k = 0; k < 8; k++) same = same && c16[k] == c8[k].x && c16[8 + k] == c8[k].y;
        CHECK(same, "host_corners16 differs at yaw %d top %d config %d", yi, t, cfg);
        if (ok > 0 && !accepted++) { std::memcpy(c16_out, c16, sizeof(c16)); s_out = s; yaw_out = yaw; }
      }
  }
  return accepted;
}

// ---- the record writers against the output layout: 2 frames, 3 boxes, KMAX = 2 -------------------------------------------------------
static void check_writers(const std::vector<CamCache>& cams, const CamCache& raw, cs::JobDesc jd, const double* c16, const SlotRef& s_ok) {
  enum { NF = 2, MB = 3, KMAX = 2 };
  std::vector<cs_cuboid> out(NF * MB * KMAX + 2);      // (one spare record at either end)
  std::vector<int> counts(NF * MB + 2, -7);
  std::memset(out.data(), 0xAB, sizeof(cs_cuboid) * out.size());
  const OutView O{out.data() + 1, counts.data() + 1, MB, KMAX};
  CHECK(&O.rec(1, 2, 1) == out.data() + 1 + (1 * MB + 2) * KMAX + 1 && &O.count(1, 2) == counts.data() + 1 + 1 * MB + 2, "OutView addresses");
  FrameIn F{};
  std::memcpy(F.K, K_CAM, sizeof(F.K)); inv3(F.K, F.invK);
  F.n_boxes = MB;
  for (int q = 0; q < MB; q++) { const double bx[5] = {100.0 + 150 * q, 150, 200, 120, 0.9}; F.boxes.insert(F.boxes.end(), bx, bx + 5); }
  // exact winners of box 2 of frame 1: the accepted proposal twice (two yaw samples), corners through both forms of the writer
  jd.frame = 1; jd.box = 2; jd.slot_off = 64; jd.yaw_off = 3;
  const double yaw[8] = {0, 0, 0, 0.25, 0.5, 0.75, 1.0, 1.25};
  auto slot_of = [&](int y) { return jd.slot_off + (((long long)s_ok.rp * jd.Y + y) * jd.T + s_ok.t) * 2 + (s_ok.cfg - 1); };
  const std::vector<ExactWinner> wl = {ExactWinner{slot_of(1), 0, 11, 0.125, 2.5, 0.0625, 1}, ExactWinner{slot_of(4), 0, 12, 0.375, 3.5, 0.1875, 2}};
  double two[32];
  std::memcpy(two, c16, 16 * sizeof(double)); std::memcpy(two + 16, c16, 16 * sizeof(double));
  for (int form = 0; form < 2; form++) {
    int calls = 0;
    if (form == 0) write_exact_winners(O, F, &jd, wl, yaw, cams, raw.euler, true, corners_at(two));
    else write_exact_winners(O, F, &jd, wl, yaw, cams, raw.euler, true, [&](size_t r, const cs::JobDesc& j, const SlotRef& s) {
      calls++;
      CHECK(&j == &jd && s.cfg == s_ok.cfg && s.t == s_ok.t && s.rp == s_ok.rp && s.y == (r == 0 ? 1 : 4), "corner source called with winner %d's job and slot", (int)r);
      return (const double*)(two + 16 * r);
    });
    CHECK(form == 0 || calls == 2, "corner source called %d times", calls);
    CHECK(O.count(1, 2) == 2, "exact winners: count %d", O.count(1, 2));
    for (int r = 0; r < 2; r++) {
      const cs_cuboid& o = O.rec(1, 2, r);
      CHECK(o.rotY == yaw[3 + (r == 0 ? 1 : 4)] && o.edge_distance_error == wl[r].dist && o.edge_angle_error == wl[r].angle && o.normalized_error == wl[r].score, "exact winner %d: values", r);
      CHECK(o.box_config_type[0] == s_ok.cfg && o.box_config_type[1] == wl[r].flag && o.rect_detect_2d[0] == 400 && o.rect_detect_2d[2] == 200, "exact winner %d: config and rectangle", r);
      CHECK(o.camera_roll_delta == cams[s_ok.rp].pose.roll - raw.euler[0] && o.camera_pitch_delta == cams[s_ok.rp].pose.pitch - raw.euler[1], "exact winner %d: roll/pitch delta", r);
    }
    O.count(1, 2) = -7;
    std::memset(&O.rec(1, 2, 0), 0xAB, 2 * sizeof(cs_cuboid));
  }
  write_exact_winners(O, F, &jd, wl, yaw, cams, raw.euler, true, corners_at(two));
  // device records of box 1 of frame 0: one of two
  cs_cuboid dev[2];
  std::memset(dev, 0, sizeof(dev));
  dev[0].rotY = 0.5; dev[0].normalized_error = 0.25; dev[1].rotY = 9.0;
  write_device_records(O, F, 0, 1, dev, 1);
  CHECK(O.count(0, 1) == 1 && O.rec(0, 1, 0).rotY == 0.5 && O.rec(0, 1, 0).normalized_error == 0.25 && O.rec(0, 1, 0).rect_detect_2d[0] == 250 && O.rec(0, 1, 0).rect_detect_2d[3] == 120, "device record");
  // nothing else written
  for (int q = -1; q <= NF * MB; q++) {
    const bool mine = q == 0 * MB + 1 || q == 1 * MB + 2;
    CHECK(mine || counts[1 + q] == -7, "count %d written", q);
  }
  for (int z = -1; z <= NF * MB * KMAX; z++) {
    const bool mine = z == (0 * MB + 1) * KMAX || z == (1 * MB + 2) * KMAX || z == (1 * MB + 2) * KMAX + 1;
    bool untouched = true;
    const unsigned char* p = reinterpret_cast<const unsigned char*>(out.data() + 1 + z);
    for (size_t k = 0; k < sizeof(cs_cuboid); k++) untouched = untouched && p[k] == 0xAB;
    CHECK(mine || untouched, "record %d written", z);
  }
  const cs_detect_params P = [] { cs_detect_params p{}; p.weight_vp_angle = 0.8; p.weight_skew_error = 1.5; p.nominal_skew_ratio = 1; p.max_cut_skew = 3; p.max_cuboid_num = 2; return p; }();
  cs::SweepParams sp{};
  sp.short_sq_bound = 400.0;
  const RankWeights W = rank_weights(P);
  const cs::RankParams RP = rank_params(P, sp);
  CHECK(W.w_angle == 0.8 && W.w_skew == 1.5 && W.nominal_skew == 1 && W.max_cut_skew == 3, "rank_weights");
  CHECK(RP.w_angle == 0.8 && RP.w_skew == 1.5 && RP.nominal_skew == 1 && RP.max_cut_skew == 3 && RP.kmax == 2 && RP.short_sq_bound == 400.0, "rank_params");
}

static void check_camera_corners_writers() {
  check_euler_round_trip();
  CamCache raw;
  check_make_cam(raw);
  std::vector<CamCache> rp;
  check_sample_poses(raw, rp, 20);      // (a forward-looking camera: its roll list, around -1.62, rounds past +6 degrees)
  CamCache tilted;
  double Rt[9];
  euler_to_rot(0.2, 0.125, -0.1, Rt);
  make_cam(K_CAM, Rt, raw.pose.t, tilted);
  check_sample_poses(tilted, rp, 25);   // both lists close at +6 degrees: the full 5 x 5 grid
  if (rp.size() != 25) return;
  cs::JobDesc jd{};
  jd.g.left = 400; jd.g.top = 150; jd.g.right = 600; jd.g.down = 270; jd.g.el = 380; jd.g.et = 130; jd.g.er = 620; jd.g.eb = 290;
  jd.RP = 25; jd.Y = 5; jd.T = 10;
  double c16[16] = {0};
  SlotRef s_ok{1, 0, 0, 0};
  double yaw_ok = 0;
  const int accepted = check_host_corners(raw, jd, c16, s_ok, yaw_ok);
  CHECK(accepted > 0, "no accepted proposal: the corner check compared zeros only");
  if (!accepted) return;
  for (int k : {0, 12, 24}) { double c[16]; SlotRef s{1, 0, 0, 0}; double y = 0; check_host_corners(rp[k], jd, c, s, y); }
  s_ok.rp = 24;
  check_writers(rp, raw, jd, c16, s_ok);
}

int main() {
  check_decode();
  check_camera_corners_writers();
  check_rank("V=0", {make_height(0, 100, false, false)}, 2);
  check_rank("V=3 (no cut)", {make_height(3, 100, false, false)}, 2);
  check_rank("V=4 (no cut)", {make_height(4, 100, false, false)}, 8);
  check_rank("V=30, equal distance keys", {make_height(30, 100, true, false)}, 3);
  check_rank("a flagged height alone", {make_height(12, 100, false, true)}, 2);
  check_rank("a flagged height between two others", {make_height(9, 0, false, false), make_height(12, 1000, false, true), make_height(7, 2000, false, false)}, 4);
  check_rank("a flagged last height", {make_height(9, 0, false, false), make_height(6, 1000, false, true)}, 1);
  check_rank("kmax > proposals", {make_height(5, 100, false, false)}, 8);
  check_rank("three heights", {make_height(40, 0, false, false), make_height(0, 5000, false, false), make_height(33, 9000, true, false)}, 5);
  check_rank("three heights, top 1", {make_height(17, 0, false, false), make_height(23, 5000, false, false), make_height(5, 9000, false, false)}, 1);
  if (g_fail) { std::printf("detect_rank_host_check: %d failure(s)\n", g_fail); return 1; }
  std::printf("detect_rank_host_check: ok\n");
  return 0;
}
