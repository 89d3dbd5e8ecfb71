// ba_structure.h -- the bundle adjustment's structure phase as named host passes (BlockSolver::buildStructure, block_solver.hpp:142-295, plus
// what this project adds to it: camera sets, the solver ordering, sharding, the Schur schedules).  Plain C++17, no HIP: every pass is integer
// work on host arrays with const inputs and a result of vectors, so each table is stated once and can be held to its definition on its own
// (tools/hostonly/ba_structure_check.cpp, under the sanitizers).  ba_host.cpp's finalize_structure calls the passes in order, decides the
// thread counts (the thresholds stay there) and owns everything that touches the device.  Where the phase reuses host scratch across calls
// (the camera lists, the edge orders) a pass writes into storage the caller hands it.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

namespace cs {

// Host scratch of the structure phase: UNINITIALISED storage (std::vector<int>(n) zero-fills on the constructing thread, which takes the
// page faults of a fresh multi-megabyte array one by one; the worker threads that fill these arrays then fault their own ranges side by side)
template <class T>
struct UBuf {
  std::unique_ptr<T[]> p;
  size_t n = 0, cap = 0;
  UBuf() {}
  explicit UBuf(size_t m) : p(new T[std::max<size_t>(1, m)]), n(m), cap(std::max<size_t>(1, m)) {}
  // a buffer kept on the handle between structure phases: the same (already faulted-in) memory again, grown with head room -- a fresh
  // 400 KB array is ~100 page faults, 0.1-0.2 ms on the thread that fills it; contents are NOT kept when it grows
  void ensure(size_t m) { if (m > cap || !p) { cap = m + m / 4 + 1024; p.reset(new T[cap]); } n = m; }
  T& operator[](size_t i) { return p[i]; }
  const T& operator[](size_t i) const { return p[i]; }
  T* begin() { return p.get(); }
  const T* begin() const { return p.get(); }
  T* data() { return p.get(); }
  const T* data() const { return p.get(); }
  size_t size() const { return n; }
};

// The structure phase's threaded loops (seven or eight short bursts of <= 8 items): a process-wide set of seven parked threads instead of
// 8 x std::thread per burst (20-30 us each to create and join: over a millisecond of the phase at a million edges).  One user at a time;
// a second handle building its structure at the same moment (the sharded tests' rank threads) falls back to plain threads.
class StructPool {
 public:
  static StructPool& get() { static StructPool p; return p; }
  bool try_run(int n, const std::function<void(int)>& fn) {
    std::unique_lock<std::mutex> use(use_, std::try_to_lock);
    if (!use.owns_lock()) return false;
    if (th_.empty()) for (int i = 0; i < 7; i++) th_.emplace_back([this] { loop(); });
    fn_ = &fn; n_ = n; next_.store(0); pending_.store((int)th_.size());
    gen_.fetch_add(1);                                   // (publishes fn_ / n_ / next_ / pending_ to the workers)
    if (sleepers_.load() > 0) { std::lock_guard<std::mutex> lk(m_); cv_.notify_all(); }
    work();
    // every worker acknowledges the burst (fn must outlive their last look at it): the hot ones within a microsecond, a parked one after its wake-up
    for (int spins = 0; pending_.load(std::memory_order_acquire) != 0; spins++) { if (spins < 2000) cpu_relax(); else std::this_thread::yield(); }
    fn_ = nullptr;
    return true;
  }
  ~StructPool() {
    stop_.store(true); gen_.fetch_add(1);
    { std::lock_guard<std::mutex> lk(m_); cv_.notify_all(); }
    for (auto& t : th_) t.join();
  }
 private:
  static void cpu_relax() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#else
    std::this_thread::yield();
#endif
  }
  void work() { for (;;) { const int i = next_.fetch_add(1); if (i >= n_) break; (*fn_)(i); } }
  // A worker can stay hot for SPIN_US after a burst (CS_BA_POOL_SPIN_US; the structure phase is seven or eight bursts inside 1-2 ms, and
  // waking a parked thread is 20-40 us of the calling thread's wait each time) before it parks on the condition variable.  Default 0: on the
  // measurement boxes (a 16-CPU cgroup quota) seven spinning threads bought nothing -- 1.2 ms per appended frame at 200 cameras either way --
  // and their burnt quota came back as 5 ms throttling stalls in one frame out of ten.
  void loop() {
    unsigned long long seen = 0;
    for (;;) {
      const auto t0 = std::chrono::steady_clock::now();
      for (int spins = 0; gen_.load(std::memory_order_acquire) == seen; spins++) {
        cpu_relax();
        if ((spins & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(SPIN_US)) {
          std::unique_lock<std::mutex> lk(m_);
          sleepers_.fetch_add(1);                        // (seq_cst against try_run's gen_ increment + sleepers_ read: one of the two sees the other)
          cv_.wait(lk, [&] { return gen_.load() != seen; });
          sleepers_.fetch_sub(1);
          break;
        }
      }
      seen = gen_.load(std::memory_order_acquire);
      if (stop_.load()) return;
      work();
      pending_.fetch_sub(1, std::memory_order_release);
    }
  }
  const int SPIN_US = [] { const char* e = getenv("CS_BA_POOL_SPIN_US"); return e ? atoi(e) : 0; }();
  std::vector<std::thread> th_;
  std::mutex use_, m_;
  std::condition_variable cv_;
  const std::function<void(int)>* fn_ = nullptr;
  std::atomic<int> next_{0}, pending_{0}, sleepers_{0};
  int n_ = 0;
  std::atomic<unsigned long long> gen_{0};
  std::atomic<bool> stop_{false};
};
// threads of a structure-phase burst: min(8, hardware threads), or fewer with CS_BA_STRUCT_THREADS (= 1: every loop on the calling thread --
// tests hold the threaded tables to the sequential ones, cs_ba_structure_digest)
inline int struct_threads() {
  static const int cap = [] { const char* e = getenv("CS_BA_STRUCT_THREADS"); const int v = e ? atoi(e) : 0; return v > 0 ? v : 8; }();
  return (int)std::max(1u, std::min((unsigned)cap, std::thread::hardware_concurrency()));
}
// items 0 .. n - 1 side by side (n <= 8 in the structure phase)
inline void run_items(int n, const std::function<void(int)>& fn) {
  if (n <= 1) { if (n == 1) fn(0); return; }
  if (StructPool::get().try_run(n, fn)) return;
  std::vector<std::thread> th;
  for (int t = 0; t < n; t++) th.emplace_back(fn, t);
  for (auto& t : th) t.join();
}

// ---- what the passes read
struct Vertices { int nc = 0, no = 0, np = 0; const int* cam_fixed = nullptr; const int* cub_fixed = nullptr; const int* pt_fixed = nullptr; };
// the pose edges' ends: camera-cuboid edges (EdgeSE3Cuboid list, then EdgeSE3CuboidProj list), odometry edges, and the host-evaluated external
// edges' (class_i, idx_i, class_j, idx_j) records
struct PoseEdgeEnds { int n_cub = 0; const int* ce_cam = nullptr; const int* ce_cub = nullptr; int n_odom = 0; const int* oe_i = nullptr; const int* oe_j = nullptr; int ext_n = 0; const int* ext_e4 = nullptr; };
// the sharding: this rank of n, and -- separator mode -- the column cut (empty otherwise)
struct Sharding { int rank = 0, n = 1; const std::vector<int>* cut = nullptr; bool sep_mode() const { return cut && !cut->empty(); } };

// ---- the landmarks' camera lists.  Landmark p's projection edges are [cam_cnt[p], cam_cnt[p + 1]) of cams_of (the camera, sorted by id) and
// edge_of (the caller's edge index; caller order among equal cameras).  cams_of / edge_of: n_proj ints each, the caller's storage.
struct CameraLists {
  std::vector<int> cam_cnt;
  int* cams_of = nullptr; int* edge_of = nullptr;
  int count(int p) const { return cam_cnt[p + 1] - cam_cnt[p]; }
  const int* begin(int p) const { return cams_of + cam_cnt[p]; }
  const int* end(int p) const { return cams_of + cam_cnt[p + 1]; }
};
// the lists of the phase before, of a graph that has only been appended to since: its first n_edges edges and cam_cnt.size() - 1 landmarks
struct PrevLists { int n_edges = 0; const std::vector<int>* cam_cnt = nullptr; const int* cams_of = nullptr; const int* edge_of = nullptr; };

// stable insertion sort of one camera list by key(camera), the edges with it (a handful of entries; stable: caller order among equal keys)
template <class Key>
inline void sort_camera_list(int* cam, int* edge, int n, Key key) {
  for (int a = 1; a < n; a++) {
    const int c = cam[a], e = edge[a];
    const auto kc = key(c);
    int q = a;
    while (q > 0 && key(cam[q - 1]) > kc) { cam[q] = cam[q - 1]; edge[q] = edge[q - 1]; q--; }
    cam[q] = c; edge[q] = e;
  }
}
inline void sort_camera_list(int* cam, int* edge, int n) { sort_camera_list(cam, edge, n, [](int c) { return c; }); }

// A counting sort of the edges by landmark (the edge order inside a landmark stays the caller's), then every landmark's camera list
// sorted, its edges with it.  Threaded (nt > 1) in two levels: the edges are first dealt into landmark ranges (thread t walks its share of the
// edges and appends to its own list per range), then range r's thread counts, fills and sorts from the lists of its range only --
// every edge is read three times in all, every write (and the page faults of the two fresh arrays) is partitioned.  (First form: one
// thread counted all edges, then every thread scanned ALL edges for those of its landmarks -- 5.9 ms at a million edges.)
// A graph that was only APPENDED to since the last structure phase (prev != nullptr; cs_ba_append_*): every landmark's old list is copied,
// its new edges follow in the caller's order, and the same stable insertion sort runs over the landmarks
// that got edges -- the same lists as the counting sort gives (old edges precede new ones in the caller's order), in one linear
// pass instead of three (200 cameras / 100 k edges, a frame of 500 edges appended: 0.28 -> 0.08 ms).
// Every e_pt is in [0, np) (the caller has checked).
inline void landmark_camera_lists(int np, int n_proj, const int* e_pt, const int* e_cam, const PrevLists* prev, int nt, CameraLists& L) {
  std::vector<int>& cam_cnt = L.cam_cnt;
  int* const cams_of = L.cams_of; int* const edge_of = L.edge_of;
  cam_cnt.assign((size_t)np + 1, 0);
  if (prev) {
    const int E0 = prev->n_edges, np0 = (int)prev->cam_cnt->size() - 1;
    const std::vector<int>& cnt0 = *prev->cam_cnt;
    std::vector<int> add(np + 1, 0), used(np, 0);
    for (int k = E0; k < n_proj; k++) add[e_pt[k] + 1]++;
    for (int p = 0; p < np; p++) add[p + 1] += add[p];                          // new edges of the landmarks before p
    for (int p = 0; p <= np; p++) cam_cnt[p] = (p <= np0 ? cnt0[p] : E0) + add[p];
    const int* oc = prev->cams_of; const int* oe = prev->edge_of;
    run_items(nt, [&](int t) {                                                  // (the old lists are out of cache by now: the copy is a burst of misses)
      const int p0 = (int)((long long)np0 * t / nt), p1 = (int)((long long)np0 * (t + 1) / nt);
      if (p1 <= p0) return;
      // (the landmarks of a range that got no edge in between move as one block: runs are copied whole)
      int p = p0;
      while (p < p1) {
        int q = p + 1;
        while (q < p1 && add[q] == add[p]) q++;                                 // landmarks p .. q - 1: the same shift (only the last may have new edges)
        const int a0 = cnt0[p], a1 = cnt0[q], d0 = cam_cnt[p];
        std::memcpy(cams_of + d0, oc + a0, sizeof(int) * (size_t)(a1 - a0));
        std::memcpy(edge_of + d0, oe + a0, sizeof(int) * (size_t)(a1 - a0));
        p = q;
      }
    });
    for (int k = E0; k < n_proj; k++) {
      const int p = e_pt[k], m_old = p < np0 ? cnt0[p + 1] - cnt0[p] : 0, q = cam_cnt[p] + m_old + used[p]++;
      cams_of[q] = e_cam[k]; edge_of[q] = k;
    }
    for (int k = E0; k < n_proj; k++) { const int p = e_pt[k]; sort_camera_list(cams_of + cam_cnt[p], edge_of + cam_cnt[p], cam_cnt[p + 1] - cam_cnt[p]); }
  } else if (nt <= 1 || np == 0) {
    for (int k = 0; k < n_proj; k++) cam_cnt[e_pt[k] + 1]++;
    for (int i = 0; i < np; i++) cam_cnt[i + 1] += cam_cnt[i];
    std::vector<int> fill(cam_cnt.begin(), cam_cnt.end() - 1);
    for (int k = 0; k < n_proj; k++) { const int q = fill[e_pt[k]]++; cams_of[q] = e_cam[k]; edge_of[q] = k; }
    for (int p = 0; p < np; p++) sort_camera_list(cams_of + cam_cnt[p], edge_of + cam_cnt[p], cam_cnt[p + 1] - cam_cnt[p]);
  } else {
    const int NT = nt;
    auto range_of = [&](int p) { return (int)(((long long)p * NT) / np); };                    // landmark -> range
    auto range_lo = [&](int r) { return (int)(((long long)r * np + NT - 1) / NT); };            // first landmark of range r (inverse of range_of)
    std::vector<std::vector<int>> dealt((size_t)NT * NT);                                      // [dealing thread][range]: edge indices, ascending
    run_items(NT, [&](int t) {
      const int k0 = (int)((long long)n_proj * t / NT), k1 = (int)((long long)n_proj * (t + 1) / NT);
      for (int r = 0; r < NT; r++) dealt[(size_t)t * NT + r].reserve((size_t)(k1 - k0) / NT + 64);
      for (int k = k0; k < k1; k++) dealt[(size_t)t * NT + range_of(e_pt[k])].push_back(k);
    });
    std::vector<int> range_edges(NT + 1, 0);       // where a range's edges start in the grouped arrays
    for (int r = 0; r < NT; r++) { size_t m = 0; for (int t = 0; t < NT; t++) m += dealt[(size_t)t * NT + r].size(); range_edges[r + 1] = range_edges[r] + (int)m; }
    run_items(NT, [&](int r) {       // (cam_cnt[p + 1] of the range's landmarks is this thread's alone: count, then end offset)
      const int p0 = range_lo(r), p1 = r + 1 < NT ? range_lo(r + 1) : np;
      for (int t = 0; t < NT; t++) for (int k : dealt[(size_t)t * NT + r]) cam_cnt[e_pt[k] + 1]++;
      std::vector<int> fill((size_t)(p1 - p0));
      int at = range_edges[r];
      for (int p = p0; p < p1; p++) { fill[p - p0] = at; at += cam_cnt[p + 1]; cam_cnt[p + 1] = at; }
      for (int t = 0; t < NT; t++) for (int k : dealt[(size_t)t * NT + r]) { const int q = fill[e_pt[k] - p0]++; cams_of[q] = e_cam[k]; edge_of[q] = k; }
      // (the lists' bounds: cam_cnt[p0] belongs to the range before -- its value is range_edges[r])
      for (int p = p0; p < p1; p++) {
        const int a0 = p == p0 ? range_edges[r] : cam_cnt[p], a1 = cam_cnt[p + 1];
        sort_camera_list(cams_of + a0, edge_of + a0, a1 - a0);
      }
    });
  }
}
// The duplicate-edge check: false when two edges join the same landmark and camera.  `seen` takes the free landmarks with at least one edge,
// in landmark order (what group_by_camera_set orders).
inline bool check_lists_collect_seen(const CameraLists& L, int np, const int* pt_fixed, std::vector<int>& seen) {
  for (int p = 0; p < np; p++) {
    for (int a = L.cam_cnt[p] + 1; a < L.cam_cnt[p + 1]; a++) if (L.cams_of[a] == L.cams_of[a - 1]) return false;
    if (!pt_fixed[p] && L.cam_cnt[p + 1] > L.cam_cnt[p]) seen.push_back(p);
  }
  return true;
}

// ---- the free landmarks grouped by the set of cameras that see them.  gorder: free landmarks with >= 1 edge sorted by (number of cameras,
// camera list), in landmark order inside a set; run_first: where each distinct set starts (+ the end).
struct CameraSets { std::vector<int> gorder, run_first; size_t runs() const { return run_first.empty() ? 0 : run_first.size() - 1; } };

// open-addressing table of the distinct camera sets met so far, each known by a representative landmark; `Item`: what a group collects
template <class Item>
struct CameraSetTable {
  const CameraLists& L;
  size_t cap;
  std::vector<int> table, rep;
  std::vector<std::vector<Item>> items;
  CameraSetTable(const CameraLists& lists, size_t cap0) : L(lists), cap(cap0), table(cap0, -1) {}
  unsigned long long hash(int p) const {
    unsigned long long h = 1469598103934665603ull;
    for (const int* c = L.begin(p); c != L.end(p); c++) { h ^= (unsigned)*c + 0x9e3779b9u; h *= 1099511628211ull; }
    return h ^ (h >> 29);
  }
  bool same(int p, int q) const { return L.count(p) == L.count(q) && std::equal(L.begin(p), L.end(p), L.begin(q)); }
  void add(int p, Item item) {       // to the group of p's camera set (a new one: p is its representative)
    if ((rep.size() + 1) * 2 > cap) {            // grow: re-insert the groups' representatives
      cap *= 4; table.assign(cap, -1);
      for (size_t g = 0; g < rep.size(); g++) { size_t s = hash(rep[g]) & (cap - 1); while (table[s] >= 0) s = (s + 1) & (cap - 1); table[s] = (int)g; }
    }
    size_t s = hash(p) & (cap - 1);
    while (table[s] >= 0 && !same(rep[table[s]], p)) s = (s + 1) & (cap - 1);
    if (table[s] < 0) { table[s] = (int)rep.size(); rep.push_back(p); items.emplace_back(); }
    items[table[s]].push_back(item);
  }
};
// A KITTI-shaped problem has ~70x fewer distinct sets than landmarks (2 862 for 200 k at C4), so
// instead of sorting the landmarks (9.6 ms of comparisons at C4) every thread hashes its range of landmarks into its own table of
// sets, the tables are merged, the few DISTINCT sets are sorted by (number of cameras, camera list), and the landmarks are laid
// out group by group -- in landmark order inside a group, because every thread walks its range in order and the ranges are laid
// down in order.  Same gorder / run_first as the sort produced.  `seen`: check_lists_collect_seen's.
inline CameraSets group_by_camera_set(const CameraLists& L, const std::vector<int>& seen, int nt) {
  nt = std::max(1, nt);
  std::vector<CameraSetTable<int>> local;                      // per thread: the sets of its range, each with its landmarks
  local.reserve(nt);
  for (int t = 0; t < nt; t++) local.emplace_back(L, 1024);
  run_items(nt, [&](int t) { for (size_t i = seen.size() * t / nt, i1 = seen.size() * (t + 1) / nt; i < i1; i++) local[t].add(seen[i], seen[i]); });
  // merge: global groups = distinct sets over all threads, each with its (thread, local group) parts -- thread order = landmark order
  CameraSetTable<std::pair<int, int>> GG(L, 4096);
  for (int t = 0; t < nt; t++) for (size_t g = 0; g < local[t].rep.size(); g++) GG.add(local[t].rep[g], {t, (int)g});
  std::vector<int> gidx(GG.rep.size());
  for (size_t q = 0; q < gidx.size(); q++) gidx[q] = (int)q;
  std::sort(gidx.begin(), gidx.end(), [&](int x, int y) {
    const int p = GG.rep[x], q = GG.rep[y];
    if (L.count(p) != L.count(q)) return L.count(p) < L.count(q);
    return std::lexicographical_compare(L.begin(p), L.end(p), L.begin(q), L.end(q));
  });
  CameraSets S;
  S.gorder.reserve(seen.size());
  for (int q : gidx) {
    S.run_first.push_back((int)S.gorder.size());
    for (auto& pt : GG.items[q]) { const std::vector<int>& m = local[pt.first].items[pt.second]; S.gorder.insert(S.gorder.end(), m.begin(), m.end()); }
  }
  S.run_first.push_back((int)S.gorder.size());
  return S;
}

// free cameras observing a free cuboid, distinct, by camera id
inline std::vector<std::vector<int>> cuboid_camera_lists(const Vertices& V, const PoseEdgeEnds& P) {
  std::vector<std::vector<int>> cub_cams(V.no);
  for (int k = 0; k < P.n_cub; k++) if (!V.cub_fixed[P.ce_cub[k]] && !V.cam_fixed[P.ce_cam[k]]) cub_cams[P.ce_cub[k]].push_back(P.ce_cam[k]);
  for (auto& c : cub_cams) { std::sort(c.begin(), c.end()); c.erase(std::unique(c.begin(), c.end()), c.end()); }
  return cub_cams;
}

// ---- solver ordering of the pose vertices: reverse Cuthill-McKee on the block graph of the reduced system
// (camera-camera through shared landmarks and odometry edges, camera-cuboid through cuboid edges), so that S is
// banded for trajectory-shaped graphs.  elim: the free cuboids are eliminated like landmarks -- they leave the graph, couple the cameras
// that observe them, and their columns follow the reduced system's.
struct Ordering { std::vector<int> cam_col, cub_col; int n_red = 0, bw = 0; std::vector<std::vector<int>> adj; std::vector<int> free_ids; };
struct PoseGraph {
  Vertices V;
  const CameraLists* L = nullptr; const CameraSets* S = nullptr;
  PoseEdgeEnds P;
  const std::vector<std::vector<int>>* cub_cams = nullptr;
  int bits_max = 8192;          // up to this many vertices the links are collected as bits
};
inline Ordering rcm_ordering(const PoseGraph& G, bool elim) {
  const int nc = G.V.nc, no = G.V.no;
  const CameraLists& L = *G.L; const PoseEdgeEnds& P = G.P;
  Ordering O;
  O.cam_col.assign(nc, -1); O.cub_col.assign(no, -1);
  const int NV = nc + no;
  std::vector<std::vector<int>> adj(NV);
  auto is_free = [&](int v) { return v < nc ? !G.V.cam_fixed[v] : (!elim && !G.V.cub_fixed[v - nc]); };
  // (up to 8 192 vertices the links are collected as bits -- a camera pair is linked by many camera sets and, cuboids eliminated, by
  // every cuboid both see: 0.2 M pushes + a sort and unique per vertex were 4 ms of this phase at 1 000 cameras -- and read out in order)
  const bool as_bits = NV <= G.bits_max;
  const size_t Wd = as_bits ? (size_t)(NV + 63) / 64 : 0;
  std::vector<unsigned long long> bits(as_bits ? (size_t)NV * Wd : 0, 0ull);
  auto link = [&](int a, int b) {
    if (a == b || !is_free(a) || !is_free(b)) return;
    if (as_bits) { bits[(size_t)a * Wd + (b >> 6)] |= 1ull << (b & 63); bits[(size_t)b * Wd + (a >> 6)] |= 1ull << (a & 63); }
    else { adj[a].push_back(b); adj[b].push_back(a); }
  };
  // landmarks couple the cameras that see them: one clique per DISTINCT camera set (the landmarks were grouped by camera set
  // above; KITTI-shaped problems have ~100x fewer sets than landmarks)
  for (size_t r = 0; r < G.S->runs(); r++) {
    const int p = G.S->gorder[G.S->run_first[r]];
    for (const int* a = L.begin(p); a != L.end(p); a++) for (const int* b = a + 1; b != L.end(p); b++) link(*a, *b);
  }
  for (int k = 0; k < P.n_odom; k++) link(P.oe_i[k], P.oe_j[k]);
  for (int k = 0; k < P.ext_n; k++) if (P.ext_e4[4 * k + 3] >= 0) link((P.ext_e4[4 * k] ? nc : 0) + P.ext_e4[4 * k + 1], (P.ext_e4[4 * k + 2] ? nc : 0) + P.ext_e4[4 * k + 3]);
  if (!elim) { for (int k = 0; k < P.n_cub; k++) link(P.ce_cam[k], nc + P.ce_cub[k]); }
  else for (int o = 0; o < no; o++) if (!G.V.cub_fixed[o]) { const std::vector<int>& cc = (*G.cub_cams)[o]; for (size_t a = 0; a < cc.size(); a++) for (size_t b = a + 1; b < cc.size(); b++) link(cc[a], cc[b]); }
  if (as_bits) {
    for (int v = 0; v < NV; v++) {
      const unsigned long long* r = bits.data() + (size_t)v * Wd;
      for (size_t w = 0; w < Wd; w++) for (unsigned long long m = r[w]; m; m &= m - 1) adj[v].push_back((int)(64 * w) + __builtin_ctzll(m));
    }
  } else {
    for (auto& a : adj) { std::sort(a.begin(), a.end()); a.erase(std::unique(a.begin(), a.end()), a.end()); }
  }
  std::vector<int> order;  // Cuthill-McKee, component by component, starting from a minimum-degree vertex
  std::vector<char> seen(NV, 0);
  std::vector<int> by_deg;
  for (int v = 0; v < NV; v++) if (is_free(v)) by_deg.push_back(v);
  std::stable_sort(by_deg.begin(), by_deg.end(), [&](int a, int b) { return adj[a].size() < adj[b].size(); });
  for (int s0 : by_deg) {
    if (seen[s0]) continue;
    // pseudo-peripheral start: two BFS sweeps from the minimum-degree vertex of the component
    int start = s0;
    for (int sweep = 0; sweep < 2; sweep++) {
      std::vector<int> q{start}, dist(NV, -1);
      dist[start] = 0;
      for (size_t h = 0; h < q.size(); h++) for (int w : adj[q[h]]) if (dist[w] < 0) { dist[w] = dist[q[h]] + 1; q.push_back(w); }
      int far = q.back();
      for (int v : q) if (dist[v] == dist[far] && adj[v].size() < adj[far].size()) far = v;
      start = far;
    }
    size_t head = order.size();
    order.push_back(start); seen[start] = 1;
    for (; head < order.size(); head++) {
      std::vector<int> nb;
      for (int w : adj[order[head]]) if (!seen[w]) { seen[w] = 1; nb.push_back(w); }
      std::stable_sort(nb.begin(), nb.end(), [&](int a, int b) { return adj[a].size() < adj[b].size(); });
      order.insert(order.end(), nb.begin(), nb.end());
    }
  }
  std::reverse(order.begin(), order.end());
  int col = 0;
  for (int v : order) { if (v < nc) { O.cam_col[v] = col; col += 6; } else { O.cub_col[v - nc] = col; col += 9; } }
  O.n_red = col;
  if (elim) for (int o = 0; o < no; o++) if (!G.V.cub_fixed[o]) { O.cub_col[o] = col; col += 9; }   // increments of the eliminated cuboids: behind the reduced system's
  auto vcol = [&](int v) { return v < nc ? O.cam_col[v] : O.cub_col[v - nc]; };
  auto vdim = [&](int v) { return v < nc ? 6 : 9; };
  int bw = 0;
  for (int v : order) {
    bw = std::max(bw, vdim(v) - 1);
    for (int w : adj[v]) { int lo = std::min(vcol(v), vcol(w)); int hi = (vcol(v) > vcol(w)) ? vcol(v) + vdim(v) - 1 : vcol(w) + vdim(w) - 1; bw = std::max(bw, hi - lo); }
  }
  O.bw = bw;
  O.free_ids = order;          // (for the sparse plan: the block graph of the free vertices)
  O.adj = std::move(adj);
  return O;
}

// ---- sharded: the column cut of the separator mode.  Rank r owns the columns [cut[r], cut[r + 1]) of the band, its first sepw[r] >= bandwidth
// columns are the separator (sepw[0] = 0), the rest its interior.  false: no cut (a separator cannot be filled, or an interior is not both
// >= 129 columns and wider than the band -- interiors further apart than the bandwidth, the regime the band kernels are tested in).
inline bool separator_cut(const std::vector<int>& cam_col, const std::vector<int>& cub_col, int n_red, int band_ld, int R, std::vector<int>& cut, std::vector<int>& sepw) {
  struct Blk { int col, dim; };
  std::vector<Blk> blks;
  for (int c : cam_col) if (c >= 0) blks.push_back(Blk{c, 6});
  for (int c : cub_col) if (c >= 0 && c < n_red) blks.push_back(Blk{c, 9});
  std::sort(blks.begin(), blks.end(), [](const Blk& a, const Blk& b) { return a.col < b.col; });
  const int bw = band_ld - 1;
  cut.assign(R + 1, 0); sepw.assign(R, 0);
  cut[R] = n_red;
  for (int r = 1; r < R; r++) {
    const long long target = (long long)n_red * r / R;
    size_t q = 0;
    while (q < blks.size() && blks[q].col < target) q++;
    if (q >= blks.size()) return false;
    cut[r] = blks[q].col;
    int w = 0;
    while (q < blks.size() && w < bw) { w += blks[q].dim; q++; }
    if (w < bw) return false;
    sepw[r] = w;
  }
  for (int r = 0; r < R; r++) {
    const int ni = cut[r + 1] - cut[r] - sepw[r];
    if (ni < 129 || ni <= band_ld) return false;
  }
  return true;
}

// ---- who owns what.  Without a cut: camera -> rank (contiguous subsequences), landmark -> rank of the subsequence of its lowest-index
// observing camera.  With one: everything goes to the rank that owns the lowest column among the free vertices involved (none: rank 0).
inline int cam_rank(int cam, int n_cams, int n_ranks) { return (int)(((long long)cam * n_ranks) / std::max(1, n_cams)); }
inline void landmark_owners(int n_ranks, int n_cams, int n_points, int n_proj, const int* e_pt, const int* e_cam, std::vector<int>& owner) {
  std::vector<int> first(n_points, 0x7fffffff);
  for (int k = 0; k < n_proj; k++) if (e_pt[k] >= 0 && e_pt[k] < n_points) first[e_pt[k]] = std::min(first[e_pt[k]], e_cam[k]);
  owner.assign(n_points, 0);
  for (int p = 0; p < n_points; p++) owner[p] = (first[p] == 0x7fffffff) ? 0 : cam_rank(first[p], n_cams, n_ranks);
}
// rank of the lowest column among col_of(*it), it in [first, last); negative columns (fixed vertices) do not count
template <class It, class ColOf>
inline int rank_of_lowest_column(const std::vector<int>& cut, It first, It last, ColOf col_of) {
  int lo = 0x7fffffff;
  for (; first != last; ++first) { const int c = col_of(*first); if (c >= 0) lo = std::min(lo, c); }
  if (lo == 0x7fffffff) return 0;
  int r = 0;
  while (r + 2 < (int)cut.size() && lo >= cut[r + 1]) r++;
  return r;
}
inline std::vector<int> landmark_owners_by_column(const CameraLists& L, int np, const std::vector<int>& cam_col, const std::vector<int>& cut) {
  std::vector<int> owner(np, 0);
  for (int p = 0; p < np; p++) owner[p] = rank_of_lowest_column(cut, L.begin(p), L.end(p), [&](int c) { return cam_col[c]; });
  return owner;
}
// cuboid edges: with their camera's rank, or -- cuboids eliminated -- all edges of a cuboid with the rank of its lowest-index camera.
// Separator mode: by the lowest column among the free vertices involved (an eliminated cuboid: among its observing cameras).
// ca / oa: 1 = this rank evaluates the cuboid / odometry edge.
struct PoseEdgeOwners { std::vector<int> cub_owner, ca, oa; };
inline PoseEdgeOwners pose_edge_owners(const Vertices& V, const PoseEdgeEnds& P, const std::vector<std::vector<int>>& cub_cams, const std::vector<int>& cam_col,
                                       const std::vector<int>& cub_col, int n_red, bool elim, const Sharding& sh) {
  const int nc = V.nc, no = V.no;
  PoseEdgeOwners W;
  W.cub_owner.assign(no, 0); W.ca.resize(P.n_cub); W.oa.resize(P.n_odom);
  if (sh.sep_mode()) {
    const std::vector<int>& cut = *sh.cut;
    auto col_of_cam = [&](int c) { return cam_col[c]; };
    for (int o = 0; o < no; o++) W.cub_owner[o] = rank_of_lowest_column(cut, cub_cams[o].begin(), cub_cams[o].end(), col_of_cam);
    for (int k = 0; k < P.n_cub; k++) {
      const int o = P.ce_cub[k];
      const int cols[2] = {cam_col[P.ce_cam[k]], cub_col[o] < n_red ? cub_col[o] : -1};
      const int own = (elim && !V.cub_fixed[o]) ? W.cub_owner[o] : rank_of_lowest_column(cut, cols, cols + 2, [](int c) { return c; });
      W.ca[k] = own == sh.rank;
    }
    for (int k = 0; k < P.n_odom; k++) {
      const int ends[2] = {P.oe_i[k], P.oe_j[k]};
      W.oa[k] = rank_of_lowest_column(cut, ends, ends + 2, col_of_cam) == sh.rank;
    }
  } else {
    std::vector<int> first(no, 0x7fffffff);
    for (int k = 0; k < P.n_cub; k++) first[P.ce_cub[k]] = std::min(first[P.ce_cub[k]], P.ce_cam[k]);
    for (int o = 0; o < no; o++) W.cub_owner[o] = first[o] == 0x7fffffff ? 0 : cam_rank(first[o], nc, sh.n);
    for (int k = 0; k < P.n_cub; k++) W.ca[k] = (elim ? W.cub_owner[P.ce_cub[k]] : cam_rank(P.ce_cam[k], nc, sh.n)) == sh.rank;
    for (int k = 0; k < P.n_odom; k++) W.oa[k] = cam_rank(P.oe_j[k], nc, sh.n) == sh.rank;
  }
  return W;
}

// ---- projection edges: point-major order (sorted by pose column inside a point), camera-major copy.  The edges are already
// grouped by landmark with their cameras sorted by id (CameraLists); a rank's point-major table is its own landmarks'
// groups, each re-ordered by (column, camera id) -- k <= a handful of entries -- in a few host threads on disjoint ranges.
// The five per-slot arrays (E = pt_ptr[np] ints each) are the caller's storage.
struct EdgeOrders {
  std::vector<int> pt_ptr, cam_ptr;
  int E = 0;                                              // this rank's edges
  int* pm_pt = nullptr; int* pm_cam = nullptr; int* src_of_slot = nullptr;   // point-major slot -> landmark, camera, caller edge
  int* cm_pm = nullptr; int* cm_pt = nullptr;                                // camera-major slot -> point-major slot, landmark
};
inline void landmark_slot_ranges(const CameraLists& L, int np, const std::vector<int>& owner, int rank, EdgeOrders& O) {
  O.pt_ptr.assign((size_t)np + 1, 0);
  for (int p = 0; p < np; p++) O.pt_ptr[p + 1] = O.pt_ptr[p] + (owner[p] == rank ? L.count(p) : 0);
  O.E = O.pt_ptr[np];
}
inline void point_major_order(const CameraLists& L, int np, const std::vector<int>& owner, int rank, const std::vector<int>& cam_col, int nt, EdgeOrders& O) {
  nt = std::max(1, nt);
  const int* col = cam_col.data();
  run_items(nt, [&](int t) {
    for (int p = (int)((long long)np * t / nt), p1 = (int)((long long)np * (t + 1) / nt); p < p1; p++) {
      if (owner[p] != rank) continue;
      const int a0 = L.cam_cnt[p], k = L.count(p), s0 = O.pt_ptr[p];
      for (int a = 0; a < k; a++) { O.pm_cam[s0 + a] = L.cams_of[a0 + a]; O.src_of_slot[s0 + a] = L.edge_of[a0 + a]; O.pm_pt[s0 + a] = p; }
      // by (column, camera id): fixed cameras (column -1) first, by id; stable
      sort_camera_list(O.pm_cam + s0, O.src_of_slot + s0, k, [col](int c) { return (long long)col[c] * 4294967296ll + c; });
    }
  });
}
// camera-major: a stable counting sort of the point-major slots by camera, the slots cut into nt ranges (per-range histograms)
inline void camera_major_order(int nc, int nt, EdgeOrders& O) {
  nt = std::max(1, nt);
  const int E = O.E;
  O.cam_ptr.assign((size_t)nc + 1, 0);
  std::vector<std::vector<int>> hist(nt, std::vector<int>(nc, 0));
  run_items(nt, [&](int t) { for (int sl = (int)((long long)E * t / nt), s1 = (int)((long long)E * (t + 1) / nt); sl < s1; sl++) hist[t][O.pm_cam[sl]]++; });
  int run = 0;
  for (int c = 0; c < nc; c++) {
    O.cam_ptr[c] = run;
    for (int t = 0; t < nt; t++) { const int v = hist[t][c]; hist[t][c] = run; run += v; }    // where range t starts writing camera c
  }
  O.cam_ptr[nc] = run;
  run_items(nt, [&](int t) { std::vector<int>& h = hist[t]; for (int sl = (int)((long long)E * t / nt), s1 = (int)((long long)E * (t + 1) / nt); sl < s1; sl++) { const int q = h[O.pm_cam[sl]]++; O.cm_pm[q] = sl; O.cm_pt[q] = O.pm_pt[sl]; } });
}
// one per-edge attribute of the projection edges in both orders: kind_of(caller edge) per point-major slot, and its camera-major copy
template <class KindOf>
inline void proj_kind_tables(const EdgeOrders& O, KindOf kind_of, std::vector<int>& pk, std::vector<int>& ck) {
  pk.assign(std::max(1, O.E), 0); ck.assign(std::max(1, O.E), 0);
  for (int sl = 0; sl < O.E; sl++) pk[sl] = kind_of(O.src_of_slot[sl]);
  for (int q = 0; q < O.E; q++) ck[q] = pk[O.cm_pm[q]];
}

// ---- Schur pattern (block_solver.hpp:262-292), fused path: segments of landmarks with one camera set + the destination
// schedule of their partial blocks (BaView::fused); with `elim` the eliminated cuboids join it.  A FusedSchedule as constructed is the
// placeholder the device gets when the pair-major path is taken (one element per table, no + 1 for cubS_ptr).
struct FusedSchedule {
  std::vector<int> run_lm{0}, seg_ptr{0}, seg_k{0}, seg_tile{0}, seg_slot{0}, run_e0{0}, seg_cam{0};
  std::vector<int> gp_ptr{0}, gp_i1{0}, gp_i2{0}, gtile{0}, gcam_ptr{0}, gslot{0};
  std::vector<int> cubS_ptr, cubS_cam{0}, ce_slot{0}, cub_tile{0}, cub_coef{0}, slotE_ptr{0}, slotE_idx{0};
  int n_seg = 0, n_gpairs = 0, n_tiles = 0, n_slots = 0, seg_class[5] = {0, 0, 0, 0, 0};
  // work lists of the build: (destination block = its two columns, partial block id) and (camera, partial vector id), in creation order: ids grow
  struct Dst { int a, b, id; };
  std::vector<Dst> dst;
  std::vector<std::pair<int, int>> cdst;
  explicit FusedSchedule(int no) : cubS_ptr((size_t)no + 1, 0) {}
};
struct SchurInput {
  Vertices V;
  const CameraLists* L = nullptr; const CameraSets* S = nullptr;
  const std::vector<int>* owner = nullptr; int rank = 0;
  const std::vector<int>* cam_col = nullptr; const std::vector<int>* pt_ptr = nullptr;
  int n_pose = 0;
  bool elim = false; const std::vector<std::vector<int>>* cub_cams = nullptr; PoseEdgeEnds P;
  int seg_lm = 32, fused_kmax = 13;        // BA_SEG_LM, BA_FUSED_KMAX (ba_types.h)
};
// The build is four steps, so that the caller can put its phase marks (and the eliminated cuboids' uploads) between them; schur_schedule_fused
// below is all four.
// 1. Segments.  Two passes over the runs (camera sets), both threaded: what a run contributes to every table is a function of its size and its cameras
// alone -- count, prefix over the runs, then every run writes its own ranges.  (One thread appending to ten vectors was 2.5-3.3 ms
// at C4.  Same tables, entry for entry: the no-GPU digest test holds the threaded build to the sequential one.)
inline void fused_segments(const SchurInput& in, int nt, FusedSchedule& F) {
  nt = std::max(1, nt);
  const CameraLists& L = *in.L; const std::vector<int>& gorder = in.S->gorder; const std::vector<int>& run_first = in.S->run_first;
  const std::vector<int>& owner = *in.owner; const int* cam_col = in.cam_col->data(); const std::vector<int>& pt_ptr = *in.pt_ptr;
  const int seg_lm = in.seg_lm, rank = in.rank;
  const size_t R = in.S->runs();
  struct RunCnt { int m, k, f, dps; };       // owned landmarks, cameras, free cameras, destination blocks per segment
  std::vector<RunCnt> rc_(R);
  std::vector<int> slot_cam_all;             // every run's cameras in slot order (by column, then id), run after run
  std::vector<size_t> sc_off(R + 1, 0);
  for (size_t r = 0; r < R; r++) sc_off[r + 1] = sc_off[r] + (size_t)L.count(gorder[run_first[r]]);
  slot_cam_all.resize(sc_off[R]);
  run_items(nt, [&](int t) {
    for (size_t r = R * t / nt, r1 = R * (t + 1) / nt; r < r1; r++) {
      const int p0 = gorder[run_first[r]], k = L.count(p0);
      int* sc = slot_cam_all.data() + sc_off[r];
      std::copy(L.begin(p0), L.end(p0), sc);
      std::sort(sc, sc + k, [&](int x, int y) { return cam_col[x] != cam_col[y] ? cam_col[x] < cam_col[y] : x < y; });
      int m = 0, f = 0, dps = 0;
      for (int q = run_first[r]; q < run_first[r + 1]; q++) m += owner[gorder[q]] == rank ? 1 : 0;
      for (int a2 = 0; a2 < k; a2++) if (cam_col[sc[a2]] >= 0) { f++; dps += k - a2; }
      rc_[r] = RunCnt{m, k, f, dps};
    }
  });
  // where every run starts in every table
  std::vector<size_t> o_lm(R + 1, 0), o_seg(R + 1, 0), o_cam(R + 1, 0), o_dst(R + 1, 0), o_cd(R + 1, 0);
  std::vector<int> o_tile(R + 1, 0), o_slot(R + 1, 0);
  for (size_t r = 0; r < R; r++) {
    const int ns = (rc_[r].m + seg_lm - 1) / seg_lm, k = rc_[r].k;
    o_lm[r + 1] = o_lm[r] + rc_[r].m; o_seg[r + 1] = o_seg[r] + ns; o_cam[r + 1] = o_cam[r] + (size_t)ns * k;
    o_dst[r + 1] = o_dst[r] + (size_t)ns * rc_[r].dps; o_cd[r + 1] = o_cd[r] + (size_t)ns * rc_[r].f;
    o_tile[r + 1] = o_tile[r] + ns * (k * (k + 1) / 2); o_slot[r + 1] = o_slot[r] + ns * k;
  }
  F.run_lm.resize(o_lm[R]); F.run_e0.resize(o_lm[R]); F.seg_ptr.assign(o_seg[R] + 1, 0); F.seg_k.resize(o_seg[R]); F.seg_tile.resize(o_seg[R]); F.seg_slot.resize(o_seg[R]);
  F.seg_cam.resize(o_cam[R]);
  {   // (room for what the eliminated cuboids append: without it their first push_back copies the whole table)
    size_t cub_dst = 0, cub_cd = 0;
    if (in.elim) for (int o = 0; o < in.V.no; o++) if (!in.V.cub_fixed[o]) { const size_t kc = (*in.cub_cams)[o].size(); cub_dst += kc * (kc + 1) / 2; cub_cd += kc; }
    F.dst.clear(); F.cdst.clear();
    F.dst.reserve(o_dst[R] + cub_dst); F.cdst.reserve(o_cd[R] + cub_cd);
  }
  F.dst.resize(o_dst[R]); F.cdst.resize(o_cd[R]);
  run_items(nt, [&](int t) {
    for (size_t r = R * t / nt, r1 = R * (t + 1) / nt; r < r1; r++) {
      const int k = rc_[r].k;
      const int* sc = slot_cam_all.data() + sc_off[r];
      size_t lm = o_lm[r], sg = o_seg[r], cm = o_cam[r], ds = o_dst[r], cd = o_cd[r];
      int tiles = o_tile[r], slots = o_slot[r], in_seg = 0;
      for (int q = run_first[r]; q < run_first[r + 1]; q++) {
        const int p = gorder[q];
        if (owner[p] != rank) continue;
        if (in_seg == 0) {   // open a segment
          F.seg_k[sg] = k; F.seg_tile[sg] = tiles; F.seg_slot[sg] = slots;
          for (int a2 = 0; a2 < k; a2++) F.seg_cam[cm++] = sc[a2];      // (= pm_cam[pt_ptr[p] + a]: the point-major order of a landmark's edges is this slot order)
          for (int a2 = 0; a2 < k; a2++) {
            const int ca = cam_col[sc[a2]];
            if (ca < 0) continue;
            F.cdst[cd++] = {sc[a2], slots + a2};
            for (int b2 = a2; b2 < k; b2++) F.dst[ds++] = FusedSchedule::Dst{ca, cam_col[sc[b2]], tiles + a2 * k - a2 * (a2 - 1) / 2 + (b2 - a2)};
          }
          tiles += k * (k + 1) / 2; slots += k;
        }
        F.run_lm[lm] = p; F.run_e0[lm] = pt_ptr[p]; lm++;
        if (++in_seg == seg_lm) { F.seg_ptr[++sg] = (int)lm; in_seg = 0; }
      }
      if (in_seg) F.seg_ptr[++sg] = (int)lm;
    }
  });
  F.n_tiles = R ? o_tile[R] : 0; F.n_slots = R ? o_slot[R] : 0;
  F.n_seg = (int)F.seg_k.size();
  for (int q = 0; q < 5; q++) F.seg_class[q] = 0;
  for (int sgi = 0; sgi < F.n_seg; sgi++) {   // segments are sorted by k
    if (F.seg_k[sgi] <= 2) F.seg_class[0] = sgi + 1;
    if (F.seg_k[sgi] <= 5) F.seg_class[1] = sgi + 1;
    if (F.seg_k[sgi] <= 7) F.seg_class[2] = sgi + 1;
    if (F.seg_k[sgi] <= 10) F.seg_class[3] = sgi + 1;
    if (F.seg_k[sgi] <= in.fused_kmax) F.seg_class[4] = sgi + 1;
  }
}
// 2. The eliminated cuboids join the destination schedule: per free cuboid one slot per observing camera (by column), the upper
// triangle of slot pairs as partial blocks, one partial vector per slot; then the edges of a slot, in edge order (a camera may hold an
// EdgeSE3Cuboid and an EdgeSE3CuboidProj to one cuboid).
inline void fused_cuboid_slots(const SchurInput& in, FusedSchedule& F) {
  const int no = in.V.no, n_cub = in.P.n_cub;
  const int* cam_col = in.cam_col->data();
  F.cubS_ptr.assign((size_t)no + 1, 0); F.cubS_cam.clear(); F.ce_slot.assign(n_cub, -1); F.cub_tile.assign(no, 0); F.cub_coef.assign(no, 0);
  if (in.elim) {
    for (int o = 0; o < no; o++) {
      F.cubS_ptr[o] = (int)F.cubS_cam.size();
      if (in.V.cub_fixed[o]) continue;
      std::vector<int> sc = (*in.cub_cams)[o];
      std::sort(sc.begin(), sc.end(), [&](int a, int b) { return cam_col[a] != cam_col[b] ? cam_col[a] < cam_col[b] : a < b; });
      const int k = (int)sc.size();
      F.cub_tile[o] = F.n_tiles; F.cub_coef[o] = F.n_slots;
      for (int a = 0; a < k; a++) {
        F.cubS_cam.push_back(sc[a]);
        F.cdst.push_back({sc[a], F.n_slots + a});
        for (int b = a; b < k; b++) F.dst.push_back(FusedSchedule::Dst{cam_col[sc[a]], cam_col[sc[b]], F.n_tiles + a * k - a * (a - 1) / 2 + (b - a)});
      }
      F.n_tiles += k * (k + 1) / 2; F.n_slots += k;
    }
    F.cubS_ptr[no] = (int)F.cubS_cam.size();
    for (int k = 0; k < n_cub; k++) {
      const int o = in.P.ce_cub[k], c = in.P.ce_cam[k];
      if (in.V.cub_fixed[o] || in.V.cam_fixed[c]) continue;
      for (int q = F.cubS_ptr[o]; q < F.cubS_ptr[o + 1]; q++) if (F.cubS_cam[q] == c) { F.ce_slot[k] = q; break; }
    }
  }
  F.slotE_ptr.assign(F.cubS_cam.size() + 1, 0);
  for (int k = 0; k < n_cub; k++) if (F.ce_slot[k] >= 0) F.slotE_ptr[F.ce_slot[k] + 1]++;
  for (size_t q = 0; q < F.cubS_cam.size(); q++) F.slotE_ptr[q + 1] += F.slotE_ptr[q];
  F.slotE_idx.assign(std::max(1, F.slotE_ptr.back()), 0);
  std::vector<int> fill(F.slotE_ptr.begin(), F.slotE_ptr.end() - 1);
  for (int k = 0; k < n_cub; k++) if (F.ce_slot[k] >= 0) F.slotE_idx[fill[F.ce_slot[k]]++] = k;
  // (no table goes to the device empty)
  if (F.cubS_cam.empty()) F.cubS_cam.push_back(0);
  if (F.ce_slot.empty()) F.ce_slot.push_back(-1);
  if (F.cub_tile.empty()) { F.cub_tile.push_back(0); F.cub_coef.push_back(0); }
}
// 3. By destination block, the partial blocks of one destination in creation (= segment) order: ids grow with creation, so (key, id) is the stable order
// (two stable counting passes over the columns -- second column, then first -- instead of a comparison sort: 0.66 -> 0.06 ms at 200 cameras,
// a third of this phase at 1 000)
inline void fused_destination_sort(const SchurInput& in, FusedSchedule& F) {
  using Dst = FusedSchedule::Dst;
  std::vector<Dst> tmp(F.dst.size());
  std::vector<int> cnt((size_t)std::max(1, in.n_pose) + 2);
  auto pass = [&](const std::vector<Dst>& src, std::vector<Dst>& out, bool by_b) {
    std::fill(cnt.begin(), cnt.end(), 0);
    for (const Dst& e : src) cnt[(by_b ? e.b : e.a) + 1]++;
    for (size_t c = 0; c + 1 < cnt.size(); c++) cnt[c + 1] += cnt[c];
    for (const Dst& e : src) out[cnt[by_b ? e.b : e.a]++] = e;
  };
  pass(F.dst, tmp, true);
  pass(tmp, F.dst, false);
}
// 4. The destination lists: per destination block its partial blocks, per camera its partial vectors (creation order)
inline void fused_destination_lists(const SchurInput& in, FusedSchedule& F) {
  const std::vector<FusedSchedule::Dst>& dst = F.dst;
  F.gp_ptr.clear(); F.gp_i1.clear(); F.gp_i2.clear(); F.gtile.resize(dst.size());
  for (size_t i = 0; i < dst.size(); i++) {
    if (i == 0 || dst[i].a != dst[i - 1].a || dst[i].b != dst[i - 1].b) { F.gp_ptr.push_back((int)i); F.gp_i1.push_back(dst[i].a); F.gp_i2.push_back(dst[i].b); }
    F.gtile[i] = dst[i].id;
  }
  F.gp_ptr.push_back((int)dst.size());
  F.n_gpairs = (int)F.gp_i1.size();
  F.gcam_ptr.assign((size_t)in.V.nc + 1, 0); F.gslot.resize(F.cdst.size());
  for (auto& e : F.cdst) F.gcam_ptr[e.first + 1]++;
  for (int i = 0; i < in.V.nc; i++) F.gcam_ptr[i + 1] += F.gcam_ptr[i];
  std::vector<int> fill(F.gcam_ptr.begin(), F.gcam_ptr.end() - 1);
  for (auto& e : F.cdst) F.gslot[fill[e.first]++] = e.second;
}
inline FusedSchedule schur_schedule_fused(const SchurInput& in, int nt) {
  FusedSchedule F(in.V.no);
  fused_segments(in, nt, F); fused_cuboid_slots(in, F); fused_destination_sort(in, F); fused_destination_lists(in, F);
  return F;
}

// ---- pair-major path: (landmark, i1 <= i2) entries grouped by camera pair.  As constructed: the placeholder of the fused path.
struct PairSchedule { std::vector<int> pair_ptr{0}, pair_i1{0}, pair_i2{0}, ent_a{0}, ent_b{0}; int n_pairs = 0; };
inline PairSchedule schur_pairs(int np, const std::vector<int>& pt_free, const EdgeOrders& O, const std::vector<int>& cam_col, int n_pose) {
  struct Ent { long long key; int a, b; };
  std::vector<Ent> ents;
  const long long NP = std::max(1, n_pose);
  for (int p = 0; p < np; p++) {
    if (!pt_free[p]) continue;
    for (int a = O.pt_ptr[p]; a < O.pt_ptr[p + 1]; a++) {
      int ca = cam_col[O.pm_cam[a]];
      if (ca < 0) continue;
      for (int b = a; b < O.pt_ptr[p + 1]; b++) {
        int cb = cam_col[O.pm_cam[b]];
        if (cb < 0) continue;
        ents.push_back(Ent{(long long)ca * NP + cb, a, b});
      }
    }
  }
  std::stable_sort(ents.begin(), ents.end(), [](const Ent& x, const Ent& y) { return x.key < y.key; });
  PairSchedule Q;
  Q.pair_ptr.clear(); Q.pair_i1.clear(); Q.pair_i2.clear(); Q.ent_a.resize(ents.size()); Q.ent_b.resize(ents.size());
  for (size_t i = 0; i < ents.size(); i++) {
    if (i == 0 || ents[i].key != ents[i - 1].key) {
      Q.pair_ptr.push_back((int)i);
      Q.pair_i1.push_back((int)(ents[i].key / NP));
      Q.pair_i2.push_back((int)(ents[i].key % NP));
    }
    Q.ent_a[i] = ents[i].a; Q.ent_b[i] = ents[i].b;
  }
  Q.pair_ptr.push_back((int)ents.size());
  Q.n_pairs = (int)Q.pair_i1.size();
  return Q;
}

// ---- a vertex's edges: idx[ptr[v] .. ptr[v + 1]) = the edges k with end[k] == v, ascending
struct VertexEdges { std::vector<int> ptr, idx; };
inline VertexEdges vertex_edge_csr(int nv, const int* end, int n_edges) {
  VertexEdges C;
  C.ptr.assign((size_t)nv + 1, 0);
  for (int k = 0; k < n_edges; k++) C.ptr[end[k] + 1]++;
  for (int i = 0; i < nv; i++) C.ptr[i + 1] += C.ptr[i];
  C.idx.resize(n_edges);
  std::vector<int> fill(C.ptr.begin(), C.ptr.end() - 1);
  for (int k = 0; k < n_edges; k++) C.idx[fill[end[k]]++] = k;
  return C;
}

}  // namespace cs
