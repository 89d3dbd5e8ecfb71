// pgo_plan_check.cpp -- the sparse plan of a pose graph (cube_slam_wu_amd/csrc/ba_sparse.h on 7-wide blocks) without a GPU and without the
// library: reads a graph, builds the plan exactly as pgo_host.cpp's build_structure does (columns = the free vertices that have an edge, in
// vertex order, 7 each; adjacency over edges between two such vertices; dim = 7, max_panel_doubles = 16384, max_fill = 0.35, a tail of at most
// 9000 unknowns), prints what it chose and holds the plan to its definitions as tools/microbench/sparse_plan_check.cpp does on 6- and 9-wide
// blocks: the pattern is the fill of eliminating the vertices in the plan's order, the panels' offsets and row maps are consistent, the update
// lists complete, the processing order topological, the tail a suffix laid end to end.  tests/test_pgo_plan_cpu.py builds it with the host
// compiler and the sanitizers, over tools/hostonly/hip_standin, and runs it.
//   input (text): nv ne, then nv fixed flags, then ne vertex pairs
//   output: "plan: N <N> n <n> fill <fill> tail_start <c> n_tail <unknowns> tail_positions <N - c> levels <levels>", then "pgo_plan_check: ok"
#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>

#include "../../cube_slam_wu_amd/csrc/ba_sparse.h"

static int g_fail = 0;
#define CHECK(cond, ...) do { if (!(cond)) { g_fail++; std::printf("FAIL %s:%d %s | ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: pgo_plan_check <graph file>\n"); return 2; }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
  int nv = 0, ne = 0;
  if (std::fscanf(f, "%d %d", &nv, &ne) != 2 || nv < 1 || ne < 1 || nv > 100000 || ne > 1000000) { std::printf("bad header\n"); return 2; }
  std::vector<int> fixed(nv), vi(ne), vj(ne);
  for (int v = 0; v < nv; v++) if (std::fscanf(f, "%d", &fixed[v]) != 1) { std::printf("bad flags\n"); return 2; }
  for (int k = 0; k < ne; k++)
    if (std::fscanf(f, "%d %d", &vi[k], &vj[k]) != 2 || vi[k] < 0 || vi[k] >= nv || vj[k] < 0 || vj[k] >= nv || vi[k] == vj[k]) { std::printf("bad edge %d\n", k); return 2; }
  std::fclose(f);

  // ---- pgo_host.cpp: build_structure
  std::vector<int> deg(nv, 0), vcol(nv, -1), free_ids;
  for (int k = 0; k < ne; k++) { deg[vi[k]]++; deg[vj[k]]++; }
  int n = 0;
  for (int v = 0; v < nv; v++) if (!fixed[v] && deg[v] > 0) { vcol[v] = n; n += 7; free_ids.push_back(v); }
  std::vector<std::vector<int>> adj(nv);
  for (int k = 0; k < ne; k++) if (vcol[vi[k]] >= 0 && vcol[vj[k]] >= 0) { adj[vi[k]].push_back(vj[k]); adj[vj[k]].push_back(vi[k]); }
  std::vector<int> dim(nv, 0);
  for (int v : free_ids) dim[v] = 7;
  cs::SparsePlan P;
  if (!cs::sparse_plan_build(adj, free_ids, dim, vcol, 16384, 0.35, P, 9000)) { std::printf("plan: refused\n"); return 3; }
  const int N = P.N;
  std::printf("plan: N %d n %d fill %.4f tail_start %d n_tail %d tail_positions %d levels %d\n", N, n, (double)P.nvals / (0.5 * (double)n * (double)n), P.tail_start, P.n_tail,
              N - P.tail_start, P.levels);

  // ---- the positions are a permutation of the free vertices, 7 wide each
  CHECK(N == (int)free_ids.size(), "N %d", N);
  std::vector<int> pos(nv, -1);
  for (int j = 0; j < N; j++) {
    CHECK(P.ndim[j] == 7 && P.ncol[j] >= 0 && P.ncol[j] < n && P.ncol[j] % 7 == 0, "position %d: %d unknowns at column %d", j, P.ndim[j], P.ncol[j]);
    if (P.ncol[j] < 0 || P.ncol[j] >= n || P.ncol[j] % 7) return 1;
    const int v = free_ids[P.ncol[j] / 7];
    CHECK(pos[v] < 0, "vertex %d at two positions", v);
    pos[v] = j;
  }
  CHECK(P.ndim[N] == 1, "the right-hand side's pseudo-vertex");
  // ---- pattern = the fill of a dense boolean elimination in the plan's order; offsets; row -> entry map
  std::vector<std::set<int>> g(N);
  for (int v : free_ids) for (int w : adj[v]) g[pos[v]].insert(pos[w]);
  long long nvals = 0;
  for (int j = 0; j < N; j++) {
    std::set<int> below;
    for (int w : g[j]) if (w > j) below.insert(w);
    std::vector<int> rows(P.srow.begin() + P.sptr[j], P.srow.begin() + P.sptr[j + 1]);
    CHECK(!rows.empty() && rows.back() == N, "column %d lacks the right-hand side's entry", j);
    if (!rows.empty()) rows.pop_back();
    CHECK(rows == std::vector<int>(below.begin(), below.end()), "column %d: pattern differs from the fill", j);
    for (int a : below) for (int b : below) if (a != b) g[a].insert(b);
    int r = 7;
    for (int t = P.sptr[j]; t < P.sptr[j + 1]; t++) { CHECK(P.sroff[t] == r, "column %d: row offset of entry %d", j, t - P.sptr[j]); r += P.ndim[P.srow[t]]; }
    CHECK(r == P.prow[j] && r == 7 * (int)below.size() + 8, "column %d: %d panel rows", j, P.prow[j]);
    CHECK(P.poff[j] == nvals, "column %d: panel offset", j);
    CHECK(P.prow[j] * 7 <= 16384, "column %d: panel of %d doubles", j, P.prow[j] * 7);
    nvals += (long long)P.prow[j] * 7;
    for (int q = 0; q < P.prow[j]; q++) {
      const int t = P.rent[P.rbase[j] + q];
      CHECK(q < 7 ? t == -1 : (t >= 0 && t < P.sptr[j + 1] - P.sptr[j] && q >= P.sroff[P.sptr[j] + t] && q < P.sroff[P.sptr[j] + t] + P.ndim[P.srow[P.sptr[j] + t]]), "column %d: row %d -> entry %d", j, q, t);
    }
  }
  CHECK(nvals == P.nvals, "nvals");
  // ---- update lists and order
  std::vector<int> where(N, -1);
  for (int q = 0; q < N; q++) { CHECK(P.order[q] >= 0 && P.order[q] < N && where[P.order[q]] < 0, "order[%d]", q); if (P.order[q] >= 0 && P.order[q] < N) where[P.order[q]] = q; }
  for (int j = 0; j < N; j++) {
    std::set<int> want;
    for (int k = 0; k < j; k++) for (int t = P.sptr[k]; t < P.sptr[k + 1]; t++) if (P.srow[t] == j) want.insert(k);
    CHECK(std::vector<int>(P.rcol.begin() + P.rptr[j], P.rcol.begin() + P.rptr[j + 1]) == std::vector<int>(want.begin(), want.end()), "update list of %d", j);
    for (int u = P.rptr[j]; u < P.rptr[j + 1]; u++) {
      CHECK(P.srow[P.sptr[P.rcol[u]] + P.rpos[u]] == j, "entry index of %d in %d", j, P.rcol[u]);
      CHECK(P.rcol[u] >= P.tail_start || where[P.rcol[u]] < where[j], "order is not topological at %d", j);      // (tail columns do not wait for each other)
    }
  }
  // ---- the dense tail: a suffix of positions, its columns laid end to end, every row below a tail column inside the tail
  CHECK(P.tail_start >= 0 && P.tail_start <= N && (P.n_tail == 0) == (P.tail_start == N), "tail bounds");
  int t = 0;
  for (int j = P.tail_start; j < N; j++) {
    CHECK(P.tcol[j] == t, "tail column of %d", j);
    t += P.ndim[j];
    for (int q = P.sptr[j]; q < P.sptr[j + 1] - 1; q++) CHECK(P.srow[q] > j && P.srow[q] < N, "tail column %d: row %d", j, P.srow[q]);
  }
  CHECK(t == P.n_tail && t <= 9000 && (P.n_tail == 0 || N - P.tail_start >= 24), "tail of %d unknowns, %d positions", P.n_tail, N - P.tail_start);
  if (g_fail) { std::printf("pgo_plan_check: %d FAILED\n", g_fail); return 1; }
  std::printf("pgo_plan_check: ok\n");
  return 0;
}
