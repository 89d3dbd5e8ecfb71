// detect_rank_host_check.cpp -- the detector host's shared rules (cube_slam_wu_amd/csrc/detect_rank_host.h) on their own, without a GPU:
// decode_slot against the slot numbering, and the properties of exact_rank_box on the shapes where a ranking goes wrong (no candidates,
// no cut, a cut through equal keys, a height sample that is all flagged, fewer proposals than winners asked for, three height samples).
// tests/test_detect_rank_host_cpu.py builds it with the host compiler and the sanitizers and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

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

int main() {
  check_decode();
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
