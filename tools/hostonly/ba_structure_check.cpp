// ba_structure_check.cpp -- the passes of the bundle adjustment's structure phase (cube_slam_wu_amd/csrc/ba_structure.h) on their own, without a
// GPU and without the library: every table is held to a brute-force definition written here (stable sorts and linear scans over the edges), on
// graphs of a few cameras generated from a fixed seed, with 1, 3 and 8 threads.  tests/test_ba_structure_cpu.py builds it with the host
// compiler and the sanitizers and runs it.
#include <algorithm>
#include <cstdio>
#include <map>
#include <set>
#include <tuple>
#include <vector>

#include "../../cube_slam_wu_amd/csrc/ba_structure.h"

using namespace cs;
typedef std::vector<int> VI;

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static unsigned long long g_seed = 20240607;
static int rnd(int n) { g_seed = g_seed * 6364136223846793005ULL + 1442695040888963407ULL; return (int)((g_seed >> 33) % (unsigned long long)n); }
static const int THREADS[3] = {1, 3, 8};

struct Graph {
  int nc = 0, no = 0, np = 0;
  VI cam_fixed, cub_fixed, pt_fixed, e_pt, e_cam, ce_cam, ce_cub, oe_i, oe_j, ext_e4;
  Vertices V() const { return Vertices{nc, no, np, cam_fixed.data(), cub_fixed.data(), pt_fixed.data()}; }
  PoseEdgeEnds P() const { return PoseEdgeEnds{(int)ce_cam.size(), ce_cam.data(), ce_cub.data(), (int)oe_i.size(), oe_i.data(), oe_j.data(), (int)ext_e4.size() / 4, ext_e4.data()}; }
};
// 9 cameras (two fixed), 60 landmarks seen by 0-6 cameras (landmarks 20-39 repeat the sets of 0-19 and 40-49 those of 0-9: camera sets with two
// and three landmarks; landmark 7 has no edge, every eleventh is fixed), edges in a shuffled order, 3 cuboids (one fixed), 8 odometry edges, camera 2 with two edges to cuboid 0
static Graph base_graph() {
  Graph g;
  g.nc = 9; g.no = 3; g.np = 60;
  g.cam_fixed.assign(9, 0); g.cam_fixed[0] = g.cam_fixed[4] = 1;
  g.cub_fixed.assign(3, 0); g.cub_fixed[1] = 1;
  g.pt_fixed.assign(60, 0);
  std::vector<std::set<int>> sets(60);
  for (int p = 0; p < 60; p++) {
    g.pt_fixed[p] = p % 11 == 3;
    if (p == 7) continue;
    if (p >= 20 && p < 50) { sets[p] = sets[p % 20]; continue; }
    const int k = rnd(7);
    while ((int)sets[p].size() < k) sets[p].insert(rnd(9));
  }
  std::vector<std::pair<int, int>> e;
  for (int p = 0; p < 60; p++) for (int c : sets[p]) e.push_back({p, c});
  for (size_t i = e.size(); i > 1; i--) std::swap(e[i - 1], e[rnd((int)i)]);
  for (auto& x : e) { g.e_pt.push_back(x.first); g.e_cam.push_back(x.second); }
  const int ce[][2] = {{2, 0}, {3, 0}, {2, 0}, {5, 0}, {0, 0}, {1, 1}, {2, 1}, {6, 2}, {7, 2}, {4, 2}, {8, 2}, {1, 0}};
  for (auto& x : ce) { g.ce_cam.push_back(x[0]); g.ce_cub.push_back(x[1]); }
  for (int i = 0; i < 8; i++) { g.oe_i.push_back(i); g.oe_j.push_back(i + 1); }
  return g;
}
// a chain: camera i sees landmarks shared with camera i + 1 only
static Graph chain_graph(int nc) {
  Graph g;
  g.nc = nc; g.np = 2 * (nc - 1);
  g.cam_fixed.assign(nc, 0); g.pt_fixed.assign(g.np, 0);
  for (int p = 0; p < g.np; p++) { g.e_pt.push_back(p); g.e_cam.push_back(p / 2 + 1); g.e_pt.push_back(p); g.e_cam.push_back(p / 2); }
  return g;
}

struct Lists { CameraLists L; VI cams, edges; };
static void make_lists(const Graph& g, int np, int n_proj, const PrevLists* prev, int nt, Lists& out) {
  out.cams.assign(std::max(1, n_proj), -7); out.edges.assign(std::max(1, n_proj), -7);
  out.L.cams_of = out.cams.data(); out.L.edge_of = out.edges.data();
  landmark_camera_lists(np, n_proj, g.e_pt.data(), g.e_cam.data(), prev, nt, out.L);
}
static bool same_lists(const Lists& a, const Lists& b) { return a.L.cam_cnt == b.L.cam_cnt && a.cams == b.cams && a.edges == b.edges; }

// ---- camera lists = the edges in a stable sort by (landmark, camera)
static void check_camera_lists(const Graph& g, const char* what) {
  const int n = (int)g.e_pt.size();
  VI idx(n);
  for (int k = 0; k < n; k++) idx[k] = k;
  std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return std::make_pair(g.e_pt[x], g.e_cam[x]) < std::make_pair(g.e_pt[y], g.e_cam[y]); });
  for (int nt : THREADS) {
    Lists A;
    make_lists(g, g.np, n, nullptr, nt, A);
    CHECK((int)A.L.cam_cnt.size() == g.np + 1 && A.L.cam_cnt[0] == 0 && A.L.cam_cnt[g.np] == n, "%s nt %d", what, nt);
    for (int p = 0; p < g.np; p++) CHECK(A.L.count(p) == (int)std::count(g.e_pt.begin(), g.e_pt.end(), p), "%s nt %d landmark %d", what, nt, p);
    for (int k = 0; k < n; k++) CHECK(A.edges[k] == idx[k] && A.cams[k] == g.e_cam[idx[k]], "%s nt %d entry %d", what, nt, k);
  }
}
// the grown path: a prefix of the edges on the first np0 landmarks, then the rest appended -- edges of new landmarks, and held-back edges of
// old ones, some with a camera that sorts before the landmark's existing ones
static void check_grown_lists(const Graph& base) {
  const int np0 = 50;
  Graph g = base;
  VI first_cam(g.np, 1 << 30);
  for (size_t k = 0; k < g.e_pt.size(); k++) first_cam[g.e_pt[k]] = std::min(first_cam[g.e_pt[k]], g.e_cam[k]);
  std::vector<std::pair<int, int>> head, tail;
  int early = 0;
  for (size_t k = 0; k < base.e_pt.size(); k++) {
    const int p = base.e_pt[k], c = base.e_cam[k];
    const bool lowest_of_several = p < np0 && c == first_cam[p] && std::count(base.e_pt.begin(), base.e_pt.end(), p) > 1;
    const bool held = p >= np0 || rnd(8) == 0 || (lowest_of_several && p % 4 == 1);      // (every fourth old landmark's lowest camera arrives late)
    if (held && lowest_of_several) early++;
    (held ? tail : head).push_back({p, c});
  }
  CHECK(early > 0, "no appended edge sorts before its landmark's existing ones");
  g.e_pt.clear(); g.e_cam.clear();
  for (auto& x : head) { g.e_pt.push_back(x.first); g.e_cam.push_back(x.second); }
  for (auto& x : tail) { g.e_pt.push_back(x.first); g.e_cam.push_back(x.second); }
  const int E0 = (int)head.size(), n = (int)g.e_pt.size();
  Lists old, at_once;
  make_lists(g, np0, E0, nullptr, 1, old);
  make_lists(g, g.np, n, nullptr, 1, at_once);
  const PrevLists prev{E0, &old.L.cam_cnt, old.cams.data(), old.edges.data()};
  for (int nt : THREADS) {
    Lists grown;
    make_lists(g, g.np, n, &prev, nt, grown);
    CHECK(same_lists(grown, at_once), "grown lists, nt %d", nt);
  }
  check_camera_lists(g, "grown graph at once");
}

static VI cams_of(const Lists& A, int p) { return VI(A.L.begin(p), A.L.end(p)); }

// ---- camera-set groups = the free landmarks with an edge in a stable sort by (number of cameras, camera list)
static CameraSets check_groups(const Graph& g, const Lists& A) {
  VI seen;
  CHECK(check_lists_collect_seen(A.L, g.np, g.pt_fixed.data(), seen), "duplicate reported on the base graph");
  VI want;
  for (int p = 0; p < g.np; p++) if (!g.pt_fixed[p] && A.L.count(p) > 0) want.push_back(p);
  CHECK(seen == want, "seen landmarks");
  CHECK(std::find(want.begin(), want.end(), 7) == want.end(), "the landmark without an edge is grouped");
  std::stable_sort(want.begin(), want.end(), [&](int x, int y) { const VI a = cams_of(A, x), b = cams_of(A, y); return a.size() != b.size() ? a.size() < b.size() : a < b; });
  VI runs;
  for (size_t i = 0; i < want.size(); i++) if (i == 0 || cams_of(A, want[i]) != cams_of(A, want[i - 1])) runs.push_back((int)i);
  runs.push_back((int)want.size());
  CHECK(runs.size() < want.size(), "no two landmarks share a camera set");
  CameraSets S1;
  for (int nt : THREADS) {
    const CameraSets S = group_by_camera_set(A.L, seen, nt);
    CHECK(S.gorder == want && S.run_first == runs, "camera sets, nt %d", nt);
    if (nt == 1) S1 = S;
  }
  // a repeated (landmark, camera) pair is reported
  Graph d = g;
  d.e_pt.push_back(g.e_pt[5]); d.e_cam.push_back(g.e_cam[5]);
  for (int nt : THREADS) { Lists D; make_lists(d, d.np, (int)d.e_pt.size(), nullptr, nt, D); VI s; CHECK(!check_lists_collect_seen(D.L, d.np, d.pt_fixed.data(), s), "duplicate not reported, nt %d", nt); }
  check_camera_lists(d, "with a repeated pair");          // (equal cameras stay in the caller's order: the sort is stable)
  return S1;
}
// 2 100 distinct camera sets over 12 cameras (landmark p: the cameras of the bits of p + 1): the per-thread table (1 024 slots) and the merged one
// (4 096) both grow
static void check_many_sets() {
  Graph g;
  g.nc = 12; g.np = 2100;
  g.cam_fixed.assign(g.nc, 0); g.pt_fixed.assign(g.np, 0);
  for (int p = g.np - 1; p >= 0; p--) for (int c = 0; c < g.nc; c++) if (((p + 1) >> c) & 1) { g.e_pt.push_back(p); g.e_cam.push_back(c); }
  Lists A;
  make_lists(g, g.np, (int)g.e_pt.size(), nullptr, 3, A);
  VI seen;
  CHECK(check_lists_collect_seen(A.L, g.np, g.pt_fixed.data(), seen) && (int)seen.size() == g.np, "many sets: seen");
  VI want(seen);
  std::stable_sort(want.begin(), want.end(), [&](int x, int y) { return A.L.count(x) != A.L.count(y) ? A.L.count(x) < A.L.count(y) : std::lexicographical_compare(A.L.begin(x), A.L.end(x), A.L.begin(y), A.L.end(y)); });
  for (int nt : THREADS) {
    const CameraSets S = group_by_camera_set(A.L, seen, nt);
    CHECK(S.gorder == want && (int)S.runs() == g.np, "many sets, nt %d: %d runs", nt, (int)S.runs());
    for (size_t r = 0; r < S.run_first.size(); r++) CHECK(S.run_first[r] == (int)r, "many sets, nt %d: run %d", nt, (int)r);
  }
}

// ---- orderings
static bool same_ordering(const Ordering& a, const Ordering& b) { return a.cam_col == b.cam_col && a.cub_col == b.cub_col && a.n_red == b.n_red && a.bw == b.bw && a.adj == b.adj && a.free_ids == b.free_ids; }
static Ordering check_ordering(const Graph& g, const Lists& A, const CameraSets& S, const std::vector<VI>& cub_cams, bool elim, const char* what) {
  PoseGraph G; G.V = g.V(); G.L = &A.L; G.S = &S; G.P = g.P(); G.cub_cams = &cub_cams;
  const Ordering O = rcm_ordering(G, elim);
  G.bits_max = 0;
  CHECK(same_ordering(O, rcm_ordering(G, elim)), "%s: adjacency as bits and as lists differ", what);
  // the columns: a packing of exactly the free vertices, 6 per camera and 9 per cuboid; with elim the cuboids' follow n_red
  std::vector<std::pair<int, int>> blk, tail;
  for (int c = 0; c < g.nc; c++) { CHECK((O.cam_col[c] < 0) == (g.cam_fixed[c] != 0), "%s camera %d", what, c); if (O.cam_col[c] >= 0) blk.push_back({O.cam_col[c], 6}); }
  for (int o = 0; o < g.no; o++) { CHECK((O.cub_col[o] < 0) == (g.cub_fixed[o] != 0), "%s cuboid %d", what, o); if (O.cub_col[o] >= 0) (elim ? tail : blk).push_back({O.cub_col[o], 9}); }
  std::sort(blk.begin(), blk.end());
  int col = 0;
  for (auto& b : blk) { CHECK(b.first == col, "%s: column %d, expected %d", what, b.first, col); col += b.second; }
  CHECK(col == O.n_red, "%s n_red %d", what, O.n_red);
  for (auto& b : tail) { CHECK(b.first == col, "%s: eliminated cuboid at %d, expected %d", what, b.first, col); col += b.second; }   // (by id)
  CHECK(O.free_ids.size() == blk.size(), "%s free_ids", what);
  // bw from adj
  auto vcol = [&](int v) { return v < g.nc ? O.cam_col[v] : O.cub_col[v - g.nc]; };
  auto vdim = [&](int v) { return v < g.nc ? 6 : 9; };
  int bw = 0;
  for (int v : O.free_ids) {
    bw = std::max(bw, vdim(v) - 1);
    for (int w : O.adj[v]) { CHECK(std::count(O.free_ids.begin(), O.free_ids.end(), w) == 1, "%s: neighbour %d not free", what, w); bw = std::max(bw, std::max(vcol(v) + vdim(v), vcol(w) + vdim(w)) - 1 - std::min(vcol(v), vcol(w))); }
  }
  CHECK(bw == O.bw, "%s bw %d, from adj %d", what, O.bw, bw);
  return O;
}

// ---- edge orders
struct Orders { EdgeOrders O; VI pm_pt, pm_cam, src, cm_pm, cm_pt; };
static void make_orders(const Graph& g, const Lists& A, const VI& owner, int rank, const VI& cam_col, int nt, Orders& R) {
  landmark_slot_ranges(A.L, g.np, owner, rank, R.O);
  const int E = R.O.E;
  for (VI* v : {&R.pm_pt, &R.pm_cam, &R.src, &R.cm_pm, &R.cm_pt}) v->assign(std::max(1, E), -7);
  R.O.pm_pt = R.pm_pt.data(); R.O.pm_cam = R.pm_cam.data(); R.O.src_of_slot = R.src.data(); R.O.cm_pm = R.cm_pm.data(); R.O.cm_pt = R.cm_pt.data();
  point_major_order(A.L, g.np, owner, rank, cam_col, nt, R.O);
  camera_major_order(g.nc, nt, R.O);
}
static void check_orders(const Graph& g, const Lists& A, const VI& owner, int rank, const VI& cam_col, Orders& R1) {
  for (int nt : THREADS) {
    Orders R;
    make_orders(g, A, owner, rank, cam_col, nt, R);
    const int E = R.O.E;
    int at = 0;
    for (int p = 0; p < g.np; p++) {
      CHECK(R.O.pt_ptr[p] == at, "pt_ptr[%d]", p);
      if (owner[p] != rank) continue;        // a rank holds only its own landmarks' edges
      std::vector<std::tuple<int, int, int>> want;      // (column, camera, caller edge): fixed cameras (column -1) first
      for (size_t k = 0; k < g.e_pt.size(); k++) if (g.e_pt[k] == p) want.push_back(std::make_tuple(cam_col[g.e_cam[k]], g.e_cam[k], (int)k));
      std::sort(want.begin(), want.end());
      for (auto& w : want) { CHECK(R.pm_pt[at] == p && R.pm_cam[at] == std::get<1>(w) && R.src[at] == std::get<2>(w), "rank %d nt %d landmark %d slot %d", rank, nt, p, at); at++; }
    }
    CHECK(at == E && R.O.pt_ptr[g.np] == E, "rank %d: %d slots, E %d", rank, at, E);
    VI idx(E);
    for (int s = 0; s < E; s++) idx[s] = s;
    std::stable_sort(idx.begin(), idx.end(), [&](int x, int y) { return R.pm_cam[x] < R.pm_cam[y]; });
    for (int q = 0; q < E; q++) CHECK(R.cm_pm[q] == idx[q] && R.cm_pt[q] == R.pm_pt[idx[q]], "rank %d nt %d camera-major %d", rank, nt, q);
    for (int c = 0; c <= g.nc; c++) { int m = 0; for (int s = 0; s < E; s++) m += R.pm_cam[s] < c; CHECK(R.O.cam_ptr[c] == m, "cam_ptr[%d]", c); }
    if (nt == 1) { R1 = R; R1.O.pm_pt = R1.pm_pt.data(); R1.O.pm_cam = R1.pm_cam.data(); R1.O.src_of_slot = R1.src.data(); R1.O.cm_pm = R1.cm_pm.data(); R1.O.cm_pt = R1.cm_pt.data(); }
  }
}

// ---- fused schedule
static bool same_schedule(const FusedSchedule& a, const FusedSchedule& b) {
  return a.run_lm == b.run_lm && a.seg_ptr == b.seg_ptr && a.seg_k == b.seg_k && a.seg_tile == b.seg_tile && a.seg_slot == b.seg_slot && a.run_e0 == b.run_e0 && a.seg_cam == b.seg_cam &&
         a.gp_ptr == b.gp_ptr && a.gp_i1 == b.gp_i1 && a.gp_i2 == b.gp_i2 && a.gtile == b.gtile && a.gcam_ptr == b.gcam_ptr && a.gslot == b.gslot && a.cubS_ptr == b.cubS_ptr &&
         a.cubS_cam == b.cubS_cam && a.ce_slot == b.ce_slot && a.cub_tile == b.cub_tile && a.cub_coef == b.cub_coef && a.slotE_ptr == b.slotE_ptr && a.slotE_idx == b.slotE_idx &&
         a.n_seg == b.n_seg && a.n_gpairs == b.n_gpairs && a.n_tiles == b.n_tiles && a.n_slots == b.n_slots && std::equal(a.seg_class, a.seg_class + 5, b.seg_class);
}
static void check_fused(const Graph& g, const Lists& A, const CameraSets& S, const std::vector<VI>& cub_cams, const Ordering& Ord, bool elim, const VI& owner, int rank) {
  const VI& col = Ord.cam_col;
  Orders R;
  make_orders(g, A, owner, rank, col, 1, R);
  SchurInput in;
  in.V = g.V(); in.L = &A.L; in.S = &S; in.owner = &owner; in.rank = rank; in.cam_col = &col; in.pt_ptr = &R.O.pt_ptr; in.n_pose = Ord.n_red + (elim ? 9 * 2 : 0);
  in.elim = elim; in.cub_cams = &cub_cams; in.P = g.P(); in.seg_lm = 2; in.fused_kmax = 4;       // (two landmarks per segment: a camera set with three gives a full segment and a rest)
  const FusedSchedule F = schur_schedule_fused(in, 1);
  for (int nt : THREADS) CHECK(same_schedule(F, schur_schedule_fused(in, nt)), "fused schedule, elim %d rank %d, nt %d", (int)elim, rank, nt);
  auto by_col = [&](VI c) { std::sort(c.begin(), c.end(), [&](int x, int y) { return std::make_pair(col[x], x) < std::make_pair(col[y], y); }); return c; };
  // every owned landmark in exactly one segment, which has its camera set
  const int n_seg = (int)F.seg_k.size();
  CHECK(F.n_seg == n_seg && (int)F.seg_ptr.size() == n_seg + 1 && F.seg_ptr[0] == 0 && F.seg_ptr[n_seg] == (int)F.run_lm.size(), "segment table sizes");
  VI want_lm;
  for (int p : S.gorder) if (owner[p] == rank) want_lm.push_back(p);
  VI got(F.run_lm); std::sort(got.begin(), got.end()); std::sort(want_lm.begin(), want_lm.end());
  CHECK(got == want_lm, "owned landmarks and run_lm differ");
  int tiles = 0, slots = 0, cam_at = 0;
  std::vector<std::tuple<int, int, int>> tri;          // (column a, column b, id) in creation order
  std::vector<VI> cam_slots(g.nc);
  for (int s = 0; s < n_seg; s++) {
    const int k = F.seg_k[s], m = F.seg_ptr[s + 1] - F.seg_ptr[s];
    CHECK(m >= 1 && m <= in.seg_lm, "segment %d holds %d landmarks", s, m);
    CHECK(s == 0 || F.seg_k[s - 1] <= k, "segment %d: k decreases", s);
    CHECK(F.seg_tile[s] == tiles && F.seg_slot[s] == slots, "segment %d offsets", s);
    const VI sc(F.seg_cam.begin() + cam_at, F.seg_cam.begin() + cam_at + k);
    for (int i = F.seg_ptr[s]; i < F.seg_ptr[s + 1]; i++) {
      const int p = F.run_lm[i];
      CHECK(by_col(cams_of(A, p)) == sc, "segment %d landmark %d: camera set", s, p);
      CHECK(F.run_e0[i] == R.O.pt_ptr[p], "run_e0 of landmark %d", p);
    }
    for (int a = 0; a < k; a++) {
      if (col[sc[a]] < 0) continue;
      cam_slots[sc[a]].push_back(slots + a);
      int id = tiles;
      for (int a2 = 0; a2 < a; a2++) id += k - a2;         // rows before a in the upper triangle
      for (int b = a; b < k; b++) tri.push_back(std::make_tuple(col[sc[a]], col[sc[b]], id + (b - a)));
    }
    tiles += k * (k + 1) / 2; slots += k; cam_at += k;
  }
  CHECK(cam_at == (int)F.seg_cam.size(), "seg_cam size");
  for (int q = 0; q < 5; q++) { const int lim[5] = {2, 5, 7, 10, in.fused_kmax}; int c = 0; for (int s = 0; s < n_seg; s++) if (F.seg_k[s] <= lim[q]) c = s + 1; CHECK(F.seg_class[q] == c, "seg_class[%d]", q); }
  // eliminated cuboids: slots = the observing free cameras by column
  CHECK((int)F.cubS_ptr.size() == g.no + 1, "cubS_ptr size");
  std::vector<VI> slot_edges;
  if (elim) {
    int q = 0;
    for (int o = 0; o < g.no; o++) {
      CHECK(F.cubS_ptr[o] == q, "cubS_ptr[%d]", o);
      if (g.cub_fixed[o]) continue;
      const VI sc = by_col(cub_cams[o]);
      const int k = (int)sc.size();
      CHECK(F.cub_tile[o] == tiles && F.cub_coef[o] == slots, "cuboid %d offsets", o);
      for (int a = 0; a < k; a++) {
        CHECK(F.cubS_cam[q + a] == sc[a], "cuboid %d slot %d", o, a);
        cam_slots[sc[a]].push_back(slots + a);
        int id = tiles;
        for (int a2 = 0; a2 < a; a2++) id += k - a2;
        for (int b = a; b < k; b++) tri.push_back(std::make_tuple(col[sc[a]], col[sc[b]], id + (b - a)));
      }
      tiles += k * (k + 1) / 2; slots += k; q += k;
    }
    CHECK(F.cubS_ptr[g.no] == q, "cubS_ptr end");
    slot_edges.resize(q);
    for (size_t k = 0; k < g.ce_cam.size(); k++) {
      const int o = g.ce_cub[k], c = g.ce_cam[k];
      int want = -1;
      if (!g.cub_fixed[o] && !g.cam_fixed[c]) for (int s = F.cubS_ptr[o]; s < F.cubS_ptr[o + 1]; s++) if (F.cubS_cam[s] == c) want = s;
      CHECK(F.ce_slot[k] == want, "ce_slot[%d] = %d, expected %d", (int)k, F.ce_slot[k], want);
      if (want >= 0) slot_edges[want].push_back((int)k);
    }
    bool two = false;
    for (size_t s = 0; s < slot_edges.size(); s++) {
      two = two || slot_edges[s].size() > 1;
      CHECK(VI(F.slotE_idx.begin() + F.slotE_ptr[s], F.slotE_idx.begin() + F.slotE_ptr[s + 1]) == slot_edges[s], "edges of slot %d", (int)s);
    }
    CHECK(two, "no slot with two edges");
  } else {
    CHECK(F.cubS_ptr == VI(g.no + 1, 0) && F.ce_slot == VI(g.ce_cam.size(), -1), "cuboid tables without elimination");
  }
  CHECK(F.n_tiles == tiles && F.n_slots == slots, "n_tiles %d (%d), n_slots %d (%d)", F.n_tiles, tiles, F.n_slots, slots);
  // destination lists = the stable sort of the triples by their two columns
  std::stable_sort(tri.begin(), tri.end(), [](const std::tuple<int, int, int>& x, const std::tuple<int, int, int>& y) { return std::make_pair(std::get<0>(x), std::get<1>(x)) < std::make_pair(std::get<0>(y), std::get<1>(y)); });
  CHECK(F.gtile.size() == tri.size(), "gtile size");
  VI gp_ptr, gp_i1, gp_i2;
  for (size_t i = 0; i < tri.size(); i++) {
    if (i == 0 || std::get<0>(tri[i]) != std::get<0>(tri[i - 1]) || std::get<1>(tri[i]) != std::get<1>(tri[i - 1])) { gp_ptr.push_back((int)i); gp_i1.push_back(std::get<0>(tri[i])); gp_i2.push_back(std::get<1>(tri[i])); }
    if (i < F.gtile.size()) CHECK(F.gtile[i] == std::get<2>(tri[i]), "gtile[%d]", (int)i);
  }
  gp_ptr.push_back((int)tri.size());
  CHECK(F.gp_ptr == gp_ptr && F.gp_i1 == gp_i1 && F.gp_i2 == gp_i2 && F.n_gpairs == (int)gp_i1.size(), "destination pairs");
  VI gcam_ptr(1, 0), gslot;
  for (int c = 0; c < g.nc; c++) { gslot.insert(gslot.end(), cam_slots[c].begin(), cam_slots[c].end()); gcam_ptr.push_back((int)gslot.size()); }
  CHECK(F.gcam_ptr == gcam_ptr && F.gslot == gslot, "per-camera slot lists");
}

// ---- pair-major = the stable sort by (column a, column b) of all (a <= b) slot pairs of free landmarks with free cameras
static void check_pairs(const Graph& g, const Orders& R, const VI& cam_col, int n_pose) {
  VI pt_free(g.np);
  for (int p = 0; p < g.np; p++) pt_free[p] = !g.pt_fixed[p];
  const PairSchedule Q = schur_pairs(g.np, pt_free, R.O, cam_col, n_pose);
  std::vector<std::tuple<int, int, int, int>> ent;
  for (int a = 0; a < R.O.E; a++) for (int b = a; b < R.O.E; b++)
    if (R.pm_pt[a] == R.pm_pt[b] && pt_free[R.pm_pt[a]] && cam_col[R.pm_cam[a]] >= 0 && cam_col[R.pm_cam[b]] >= 0) ent.push_back(std::make_tuple(cam_col[R.pm_cam[a]], cam_col[R.pm_cam[b]], a, b));
  std::stable_sort(ent.begin(), ent.end(), [](const std::tuple<int, int, int, int>& x, const std::tuple<int, int, int, int>& y) { return std::make_pair(std::get<0>(x), std::get<1>(x)) < std::make_pair(std::get<0>(y), std::get<1>(y)); });
  VI pp, i1, i2, ea, eb;
  for (size_t i = 0; i < ent.size(); i++) {
    if (i == 0 || std::get<0>(ent[i]) != std::get<0>(ent[i - 1]) || std::get<1>(ent[i]) != std::get<1>(ent[i - 1])) { pp.push_back((int)i); i1.push_back(std::get<0>(ent[i])); i2.push_back(std::get<1>(ent[i])); }
    ea.push_back(std::get<2>(ent[i])); eb.push_back(std::get<3>(ent[i]));
  }
  pp.push_back((int)ent.size());
  CHECK(!ent.empty() && Q.pair_ptr == pp && Q.pair_i1 == i1 && Q.pair_i2 == i2 && Q.ent_a == ea && Q.ent_b == eb && Q.n_pairs == (int)i1.size(), "pair-major schedule (%d entries)", (int)ent.size());
}

// ---- owners: the rank found by a linear scan over the cut
static int scan_rank(const VI& cut, int lo) { if (lo == 1 << 30) return 0; int r = 0; for (size_t q = 1; q + 1 < cut.size(); q++) if (lo >= cut[q]) r = (int)q; return r; }
static void check_owners(const Graph& g, const Lists& A, const std::vector<VI>& cub_cams, const Ordering& O, bool elim, const VI& cut) {
  const int R = (int)cut.size() - 1;
  auto lowest = [&](std::initializer_list<int> cols) { int lo = 1 << 30; for (int c : cols) if (c >= 0) lo = std::min(lo, c); return lo; };
  const VI lm = landmark_owners_by_column(A.L, g.np, O.cam_col, cut);
  std::set<int> ranks;
  for (int p = 0; p < g.np; p++) {
    int lo = 1 << 30;
    for (size_t k = 0; k < g.e_pt.size(); k++) if (g.e_pt[k] == p) lo = std::min(lo, lowest({O.cam_col[g.e_cam[k]]}));
    CHECK(lm[p] == scan_rank(cut, lo), "owner of landmark %d", p);
    ranks.insert(lm[p]);
  }
  CHECK((int)ranks.size() == R, "the landmarks reach %d of %d ranks", (int)ranks.size(), R);
  for (int rank = 0; rank < R; rank++) {
    const Sharding sh{rank, R, &cut};
    const PoseEdgeOwners W = pose_edge_owners(g.V(), g.P(), cub_cams, O.cam_col, O.cub_col, O.n_red, elim, sh);
    for (int o = 0; o < g.no; o++) { int lo = 1 << 30; for (int c : cub_cams[o]) lo = std::min(lo, O.cam_col[c]); CHECK(W.cub_owner[o] == scan_rank(cut, lo), "owner of cuboid %d", o); }
    for (size_t k = 0; k < g.ce_cam.size(); k++) {
      const int o = g.ce_cub[k];
      const int own = elim && !g.cub_fixed[o] ? W.cub_owner[o] : scan_rank(cut, lowest({O.cam_col[g.ce_cam[k]], O.cub_col[o] < O.n_red ? O.cub_col[o] : -1}));
      CHECK(W.ca[k] == (own == rank), "cuboid edge %d on rank %d", (int)k, rank);
    }
    for (size_t k = 0; k < g.oe_i.size(); k++) CHECK(W.oa[k] == (scan_rank(cut, lowest({O.cam_col[g.oe_i[k]], O.cam_col[g.oe_j[k]]})) == rank), "odometry edge %d on rank %d", (int)k, rank);
  }
  // without a cut: by camera subsequence
  const VI none;
  for (int rank = 0; rank < 2; rank++) {
    const Sharding sh{rank, 2, &none};
    const PoseEdgeOwners W = pose_edge_owners(g.V(), g.P(), cub_cams, O.cam_col, O.cub_col, O.n_red, elim, sh);
    for (size_t k = 0; k < g.ce_cam.size(); k++) {
      int first = 1 << 30;
      for (size_t q = 0; q < g.ce_cam.size(); q++) if (g.ce_cub[q] == g.ce_cub[k]) first = std::min(first, g.ce_cam[q]);
      CHECK(W.ca[k] == (cam_rank(elim ? first : g.ce_cam[k], g.nc, 2) == rank), "cuboid edge %d on rank %d (no cut)", (int)k, rank);
    }
    for (size_t k = 0; k < g.oe_i.size(); k++) CHECK(W.oa[k] == (cam_rank(g.oe_j[k], g.nc, 2) == rank), "odometry edge %d on rank %d (no cut)", (int)k, rank);
  }
}

// ---- separator cut on a 60-camera chain
static void check_separator_cut() {
  const Graph g = chain_graph(60);
  Lists A;
  make_lists(g, g.np, (int)g.e_pt.size(), nullptr, 3, A);
  VI seen;
  check_lists_collect_seen(A.L, g.np, g.pt_fixed.data(), seen);
  const CameraSets S = group_by_camera_set(A.L, seen, 3);
  const std::vector<VI> cub_cams;
  const Ordering O = check_ordering(g, A, S, cub_cams, false, "chain");
  CHECK(O.n_red == 360 && O.bw == 11, "chain of 60 cameras: n_red %d, bandwidth %d", O.n_red, O.bw);
  // REVERSE Cuthill-McKee: the first minimum-degree vertex is camera 0, the two sweeps go to camera 59 and back, the breadth-first order from
  // camera 0 is 0, 1, ..., 59, and reversed it gives camera 0 the last block
  for (int c = 0; c < 60; c++) CHECK(O.cam_col[c] == 6 * (59 - c), "chain: camera %d at column %d", c, O.cam_col[c]);
  int found = 0;
  for (int R = 2; R <= 3; R++) {
    VI cut, sepw;
    const int band_ld = O.bw + 1;
    if (!separator_cut(O.cam_col, O.cub_col, O.n_red, band_ld, R, cut, sepw)) continue;
    found++;
    CHECK((int)cut.size() == R + 1 && (int)sepw.size() == R && cut[0] == 0 && cut[R] == O.n_red && sepw[0] == 0, "cut shape, R %d", R);
    for (int r = 0; r < R; r++) {
      const int ni = cut[r + 1] - cut[r] - sepw[r];
      CHECK(ni >= 129 && ni > band_ld, "R %d rank %d: interior of %d columns", R, r, ni);
      if (r > 0) CHECK(sepw[r] >= O.bw && cut[r] % 6 == 0 && sepw[r] % 6 == 0, "R %d separator %d: %d columns at %d", R, r, sepw[r], cut[r]);
    }
  }
  CHECK(found >= 1, "no cut on the chain for R = 2");
}

int main() {
  const Graph g = base_graph();
  check_camera_lists(g, "base");
  check_grown_lists(g);
  { Graph s = g; s.np = 5; s.e_pt.clear(); s.e_cam.clear(); for (int k = 0; k < 9; k++) { s.e_pt.push_back((k * 3) % 5 == 1 ? 4 : (k * 3) % 5); s.e_cam.push_back(8 - k); } s.pt_fixed.assign(5, 0); check_camera_lists(s, "5 landmarks in 8 ranges"); }
  Lists A;
  make_lists(g, g.np, (int)g.e_pt.size(), nullptr, 1, A);
  const CameraSets S = check_groups(g, A);
  check_many_sets();
  const std::vector<VI> cub_cams = cuboid_camera_lists(g.V(), g.P());
  CHECK(cub_cams[0] == (VI{1, 2, 3, 5}) && cub_cams[1].empty() && cub_cams[2] == (VI{6, 7, 8}), "cuboid camera lists");
  const Ordering keep = check_ordering(g, A, S, cub_cams, false, "base"), elim = check_ordering(g, A, S, cub_cams, true, "base, cuboids eliminated");
  { Graph x = g; x.ext_e4 = {0, 1, 1, 2, 2, 5, 0, -1, 0, 3, 0, 8}; PoseGraph G; G.V = x.V(); G.L = &A.L; G.S = &S; G.P = x.P(); G.cub_cams = &cub_cams; const Ordering O = rcm_ordering(G, false);
    CHECK(std::count(O.adj[1].begin(), O.adj[1].end(), g.nc + 2) == 1 && std::count(O.adj[3].begin(), O.adj[3].end(), 8) == 1, "external binary edges in the pose graph"); }
  // edge orders, one rank and two
  const VI all0(g.np, 0);
  VI half(g.np);
  for (int p = 0; p < g.np; p++) half[p] = p % 2;
  Orders R0, Rh;
  check_orders(g, A, all0, 0, keep.cam_col, R0);
  for (int rank = 0; rank < 2; rank++) check_orders(g, A, half, rank, elim.cam_col, Rh);
  // schedules
  check_fused(g, A, S, cub_cams, keep, false, all0, 0);
  check_fused(g, A, S, cub_cams, elim, true, all0, 0);
  for (int rank = 0; rank < 2; rank++) check_fused(g, A, S, cub_cams, elim, true, half, rank);
  check_pairs(g, R0, keep.cam_col, keep.n_red);
  { const FusedSchedule F(g.no); const PairSchedule Q;
    CHECK(F.run_lm == VI{0} && F.seg_ptr == VI{0} && F.gslot == VI{0} && F.ce_slot == VI{0} && F.slotE_idx == VI{0} && F.cubS_ptr == VI(g.no + 1, 0) && F.n_seg == 0 && Q.pair_ptr == VI{0} && Q.ent_b == VI{0} && Q.n_pairs == 0, "placeholders"); }
  // owners and the cut
  check_owners(g, A, cub_cams, keep, false, VI{0, 18, 36, keep.n_red});
  check_owners(g, A, cub_cams, elim, true, VI{0, 24, elim.n_red});
  check_separator_cut();
  // a vertex's edges, and a per-edge attribute in both orders
  { const VertexEdges C = vertex_edge_csr(g.nc, g.ce_cam.data(), (int)g.ce_cam.size());
    for (int v = 0; v < g.nc; v++) { VI want; for (size_t k = 0; k < g.ce_cam.size(); k++) if (g.ce_cam[k] == v) want.push_back((int)k); CHECK(VI(C.idx.begin() + C.ptr[v], C.idx.begin() + C.ptr[v + 1]) == want, "edges of camera %d", v); }
    VI pk, ck;
    proj_kind_tables(R0.O, [](int src) { return src % 5; }, pk, ck);
    for (int s = 0; s < R0.O.E; s++) CHECK(pk[s] == R0.src[s] % 5 && ck[s] == R0.src[R0.cm_pm[s]] % 5, "kinds of slot %d", s);
    EdgeOrders none; proj_kind_tables(none, [](int) { return 1; }, pk, ck); CHECK(pk == VI{0} && ck == VI{0}, "kind tables without edges"); }
  if (g_fail) { std::printf("ba_structure_check: %d FAILED\n", g_fail); return 1; }
  std::printf("ba_structure_check: ok\n");
  return 0;
}
