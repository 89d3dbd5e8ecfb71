// pgo_host.cpp -- the C ABI of the Sim(3) pose-graph optimisation (include/cubeslam_hip.h: cs_pgo_*).
//
// What an ORB-SLAM2-derived pipeline runs after a loop closure (Optimizer::OptimizeEssentialGraph): one VertexSim3Expmap per keyframe, one
// EdgeSim3 per spanning-tree / loop / covisibility link (types/types_seven_dof_expmap.h:48-126 over types/sim3.h), Levenberg-Marquardt
// (core/optimization_algorithm_levenberg.cpp:61-189).  No vertex is marginalised, so H + lambda I over the free vertices' 7-blocks is
// solved directly: assembled as a dense lower triangle (ba_types.h's S[r n + c]) and factorised by the general sparse Cholesky
// (cs_sparse_solver.h, ndim = 7) where its plan and grids accept the graph, by rocSOLVER potrf / potrs otherwise.  The host reads one pinned
// record per trial (chi2, scale term, pivot flags).  There is no CPU fallback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/cubeslam_hip.h"
#include "cs_hip_util.h"
#include "cs_lm.h"
#include "cs_sparse_solver.h"
#include "pgo_types.h"

// The dense system's budget: n x n doubles, n = 7 per free keyframe with an edge.  4 GiB -> n <= 23 170 -> 3 310 free keyframes.
static const size_t PGO_DENSE_BUDGET_BYTES = (size_t)4 << 30;

struct cs_pgo {
  int device = 0;
  cs::Stream st;            // (first: it dies last, after the BLAS handle bound to it and every buffer its work uses)
  cs::BlasHandle blas;
  int nv = 0, ne = 0, n = 0;
  bool have_vertices = false, have_edges = false, ran = false;
  std::vector<unsigned char> fixed, fix_scale;
  double user_lambda_init = 0.0;
  int max_trials = 10;
  cs::DevBuf<double> est, est_init, est_bak, meas, info, err, Ji, Jj, Hii, Hij, Hjj, bi, bj, chi2_each, S, b, x, diag, rec, io;
  cs::DevBuf<int> vcol, ei, ej, inc_ptr, inc_edge, d_info, io_i;
  cs::DevBuf<unsigned char> d_fix_scale, inc_side;
  cs::PinBuf<double> h_rec;     // [chi2, scale term, max |H_jj|]
  cs::PinBuf<int> h_status;     // cs::sparse_verdict's two words: the solver's, or [0, rocSOLVER's info] on the dense path
  // general sparse Cholesky (cs_sparse_solver.h)
  bool sparse = false, S_clean = false;     // this structure's solves go through `solver`; S holds nothing outside the graph's blocks
  cs::SparseSolver solver;
  double linearize_ms = 0, solve_ms = 0, total_ms = 0;
};

namespace {

using cs::now_ms;

cs::PgoView view_of(cs_pgo* G) {
  cs::PgoView v;
  v.nv = G->nv; v.ne = G->ne; v.n = G->n;
  v.est = G->est.p; v.fix_scale = G->d_fix_scale.p; v.vcol = G->vcol.p; v.ei = G->ei.p; v.ej = G->ej.p; v.meas = G->meas.p; v.info = G->info.p;
  v.err = G->err.p; v.Ji = G->Ji.p; v.Jj = G->Jj.p; v.Hii = G->Hii.p; v.Hij = G->Hij.p; v.Hjj = G->Hjj.p; v.bi = G->bi.p; v.bj = G->bj.p; v.chi2_each = G->chi2_each.p;
  v.inc_ptr = G->inc_ptr.p; v.inc_edge = G->inc_edge.p; v.inc_side = G->inc_side.p;
  v.S = G->S.p; v.b = G->b.p; v.x = G->x.p; v.diag = G->diag.p; v.rec = G->rec.p;
  return v;
}

template <class T>
int upload(cs::DevBuf<T>& d, const T* src, size_t n, hipStream_t st) {
  int rc = d.ensure(std::max<size_t>(n, 1)); if (rc) return rc;
  if (n) CS_HIP_TRY(hipMemcpyAsync(d.p, src, n * sizeof(T), hipMemcpyHostToDevice, st));
  return CS_OK;
}
template <class T>
int upload(cs::DevBuf<T>& d, const std::vector<T>& v, hipStream_t st) { return upload(d, v.data(), v.size(), st); }

int check_states(const char* fn, const double* sim8, int n, const char* what) {
  for (int i = 0; i < n; i++) {
    for (int c = 0; c < 8; c++)
      if (!std::isfinite(sim8[8 * (size_t)i + c])) { cs_set_error(std::string(fn) + ": " + what + " " + std::to_string(i) + " is not finite"); return CS_ERR_INVALID_ARG; }
    if (!(sim8[8 * (size_t)i + 7] > 0.0)) { cs_set_error(std::string(fn) + ": " + what + " " + std::to_string(i) + " has a non-positive scale"); return CS_ERR_INVALID_ARG; }
  }
  return CS_OK;
}

// e, J, the quadratic-form terms and chi2 of the current estimates: computeActiveErrors + linearizeOplus + constructQuadraticForm
int linearize(cs_pgo* G) {
  const cs::PgoView v = view_of(G);
  cs::pgo_launch_edges(v, G->st);
  cs::pgo_launch_chi2(v, G->st);
  CS_HIP_TRY(hipGetLastError());
  return CS_OK;
}

// one damped solve: S <- H + lambda I, (H + lambda I) x = b.  Nothing is waited for: the pivot flags travel with the trial's record.
int solve(cs_pgo* G, double lambda, std::unique_lock<std::mutex>* turn) {
  const cs::PgoView v = view_of(G);
  const size_t n = (size_t)G->n;
  if (!G->sparse || !G->S_clean) {      // (sparse: the factorisation reads S and writes L -- S keeps the zeros between the graph's blocks)
    CS_HIP_TRY(hipMemsetAsync(G->S.p, 0, n * n * sizeof(double), G->st));
    G->S_clean = G->sparse;
  }
  cs::pgo_launch_assemble(v, lambda, G->st);
  CS_HIP_TRY(hipGetLastError());
  if (G->sparse) {
    *turn = std::unique_lock<std::mutex>(cs::coop_mutex());     // (a persistent kernel whose workgroups wait for each other: one at a time per process)
    const int rs = G->solver.solve(G->blas, G->S.p, G->x.p, G->n, G->st);
    if (rs == cs::SparseSolver::CHOL_NOT_LAUNCHED) { cs_set_error("cs_pgo: the sparse factorisation could not be launched"); return CS_ERR_HIP; }
    if (rs == cs::SparseSolver::BACK_NOT_LAUNCHED) { cs_set_error("cs_pgo: the sparse substitution could not be launched"); return CS_ERR_HIP; }
    if (rs) return rs;
  } else {
    CS_HIP_TRY(hipMemsetAsync(G->d_info.p, 0, sizeof(int), G->st));
    // the lower triangle of the row-major S is the upper triangle of the column-major matrix rocSOLVER sees
    CS_ROC_TRY(rocsolver_dpotrf(G->blas, rocblas_fill_upper, G->n, G->S.p, G->n, G->d_info.p));
    CS_ROC_TRY(rocsolver_dpotrs(G->blas, rocblas_fill_upper, G->n, 1, G->S.p, G->n, G->x.p, G->n));
  }
  return CS_OK;
}

// the trial's record comes home: one synchronisation
int fetch_record(cs_pgo* G) {
  CS_HIP_TRY(hipMemcpyAsync(G->h_rec.p, G->rec.p, 3 * sizeof(double), hipMemcpyDeviceToHost, G->st));
  if (G->sparse) { const int rc = G->solver.queue_status(G->h_status.p, G->st); if (rc) return rc; }
  else { G->h_status.p[0] = 0; CS_HIP_TRY(hipMemcpyAsync(G->h_status.p + 1, G->d_info.p, sizeof(int), hipMemcpyDeviceToHost, G->st)); }
  CS_HIP_TRY(hipStreamSynchronize(G->st));
  return CS_OK;
}

int build_structure(cs_pgo* G, const std::vector<int>& vi, const std::vector<int>& vj) {
  const int nv = G->nv, ne = G->ne;
  // ---- columns: the free vertices that have an edge, in vertex order (sparse_optimizer.cpp:166-190)
  std::vector<int> deg(nv, 0), vcol(nv, -1);
  for (int k = 0; k < ne; k++) { deg[vi[k]]++; deg[vj[k]]++; }
  int n = 0;
  std::vector<int> free_ids;
  for (int v = 0; v < nv; v++) if (!G->fixed[v] && deg[v] > 0) { vcol[v] = n; n += 7; free_ids.push_back(v); }
  if ((size_t)n * (size_t)n * sizeof(double) > PGO_DENSE_BUDGET_BYTES) {
    cs_set_error("cs_pgo_set_edges: the dense system of " + std::to_string(n) + " unknowns (" + std::to_string(free_ids.size()) + " free keyframes) needs " +
                 std::to_string((size_t)n * n * 8 >> 20) + " MiB, above the budget of " + std::to_string(PGO_DENSE_BUDGET_BYTES >> 20) + " MiB (3310 free keyframes)");
    return CS_ERR_CAPACITY;
  }
  G->n = n;
  // ---- incident edges per vertex, by edge index: the gather's fixed order
  std::vector<int> inc_ptr(nv + 1, 0), inc_edge(2 * (size_t)ne);
  std::vector<unsigned char> inc_side(2 * (size_t)ne);
  for (int v = 0; v < nv; v++) inc_ptr[v + 1] = inc_ptr[v] + deg[v];
  {
    std::vector<int> fill(inc_ptr.begin(), inc_ptr.end() - 1);
    for (int k = 0; k < ne; k++) {
      inc_edge[fill[vi[k]]] = k; inc_side[fill[vi[k]]++] = 0;
      inc_edge[fill[vj[k]]] = k; inc_side[fill[vj[k]]++] = 1;
    }
  }
  int rc;
  hipStream_t st = G->st;
  if ((rc = upload(G->vcol, vcol, st)) || (rc = upload(G->ei, vi, st)) || (rc = upload(G->ej, vj, st)) || (rc = upload(G->inc_ptr, inc_ptr, st)) ||
      (rc = upload(G->inc_edge, inc_edge, st)) || (rc = upload(G->inc_side, inc_side, st))) return rc;
  const size_t E = std::max(ne, 1), N = std::max(n, 1);
  if ((rc = G->err.ensure(7 * E)) || (rc = G->Ji.ensure(49 * E)) || (rc = G->Jj.ensure(49 * E)) || (rc = G->Hii.ensure(49 * E)) || (rc = G->Hij.ensure(49 * E)) ||
      (rc = G->Hjj.ensure(49 * E)) || (rc = G->bi.ensure(7 * E)) || (rc = G->bj.ensure(7 * E)) || (rc = G->chi2_each.ensure(E)) || (rc = G->S.ensure(N * N)) ||
      (rc = G->b.ensure(N)) || (rc = G->x.ensure(N)) || (rc = G->diag.ensure(N)) || (rc = G->rec.ensure(4)) || (rc = G->d_info.ensure(1)) ||
      (rc = G->h_rec.ensure(4)) || (rc = G->h_status.ensure(2))) return rc;
  // ---- which factorisation: the general sparse Cholesky where its plan (fill at most 35 % of the dense triangle, panels within the LDS)
  // and its grid (co-resident on this device) accept the graph; rocSOLVER otherwise.  CS_PGO_FORCE_DENSE=1 (read per call): always rocSOLVER.
  G->sparse = false; G->S_clean = false;
  const char* fd = getenv("CS_PGO_FORCE_DENSE");
  if (!(fd && atoi(fd)) && n > 0) {
    std::vector<std::vector<int>> adj(nv);
    for (int k = 0; k < ne; k++) if (vcol[vi[k]] >= 0 && vcol[vj[k]] >= 0) { adj[vi[k]].push_back(vj[k]); adj[vj[k]].push_back(vi[k]); }
    std::vector<int> dim(nv, 0);
    for (int v : free_ids) dim[v] = 7;
    if (G->solver.build(adj, free_ids, dim, vcol, 0.35, 9000)) {      // (a plan that is refused is not uploaded, and G->sparse stays false)
      G->sparse = true;
      if ((rc = G->solver.upload(st))) return rc;
    }
  }
  CS_HIP_TRY(hipStreamSynchronize(st));      // (the uploads read host vectors that end with this call; the solver's asks for this wait too)
  return CS_OK;
}

int need(cs_pgo* G, const char* fn, bool edges) {
  if (!G) return CS_ERR_INVALID_ARG;
  if (!G->have_vertices) { cs_set_error(std::string(fn) + ": no vertices set"); return CS_ERR_NOT_RUN; }
  if (edges && !G->have_edges) { cs_set_error(std::string(fn) + ": no edges set"); return CS_ERR_NOT_RUN; }
  return CS_OK;
}

}  // namespace

extern "C" {

int cs_pgo_create(int device, cs_pgo** out) {
  if (!out) return CS_ERR_INVALID_ARG;
  *out = nullptr;
  { const int rc = cs::check_device(device); if (rc) return rc; }
  cs_pgo* G = new (std::nothrow) cs_pgo();
  if (!G) return CS_ERR_CAPACITY;
  cs::Guard<cs_pgo> guard(G, cs_pgo_destroy);
  G->device = device;
  CS_HIP_TRY(hipSetDevice(device));
  CS_TRY(G->st.create(hipStreamNonBlocking));
  CS_TRY(G->blas.create(G->st));
  *out = guard.disarm();
  return CS_OK;
}

void cs_pgo_destroy(cs_pgo* G) {
  if (!G) return;
  (void)hipSetDevice(G->device);
  if (G->st) (void)hipStreamSynchronize(G->st);
  delete G;
}

int cs_pgo_set_vertices(cs_pgo* G, int n, const double* sim8, const unsigned char* fixed, const unsigned char* fix_scale) {
  if (!G) return CS_ERR_INVALID_ARG;
  if (n < 1 || !sim8) { cs_set_error("cs_pgo_set_vertices: needs at least one vertex and its state"); return CS_ERR_INVALID_ARG; }
  int rc = check_states("cs_pgo_set_vertices", sim8, n, "vertex"); if (rc) return rc;
  CS_GUARD_BEGIN
  CS_HIP_TRY(hipSetDevice(G->device));
  G->have_vertices = G->have_edges = G->ran = false;
  G->fixed.assign(n, 0); G->fix_scale.assign(n, 0);
  for (int i = 0; i < n; i++) { G->fixed[i] = fixed && fixed[i] ? 1 : 0; G->fix_scale[i] = fix_scale && fix_scale[i] ? 1 : 0; }
  if ((rc = upload(G->est, sim8, 8 * (size_t)n, G->st)) || (rc = upload(G->est_init, sim8, 8 * (size_t)n, G->st)) || (rc = G->est_bak.ensure(8 * (size_t)n)) ||
      (rc = upload(G->d_fix_scale, G->fix_scale, G->st))) return rc;
  CS_HIP_TRY(hipStreamSynchronize(G->st));
  G->nv = n; G->ne = 0; G->n = 0;
  G->have_vertices = true;
  return CS_OK;
  CS_GUARD_END("cs_pgo_set_vertices")
}

int cs_pgo_set_estimates(cs_pgo* G, const double* sim8) {
  int rc = need(G, "cs_pgo_set_estimates", false); if (rc) return rc;
  if (!sim8) return CS_ERR_INVALID_ARG;
  rc = check_states("cs_pgo_set_estimates", sim8, G->nv, "vertex"); if (rc) return rc;
  CS_HIP_TRY(hipSetDevice(G->device));
  if ((rc = upload(G->est, sim8, 8 * (size_t)G->nv, G->st)) || (rc = upload(G->est_init, sim8, 8 * (size_t)G->nv, G->st))) return rc;
  CS_HIP_TRY(hipStreamSynchronize(G->st));
  return CS_OK;
}

int cs_pgo_set_edges(cs_pgo* G, int n, const int* vi, const int* vj, const double* meas8, const double* info49) {
  int rc = need(G, "cs_pgo_set_edges", false); if (rc) return rc;
  if (n < 1 || !vi || !vj || !meas8) { cs_set_error("cs_pgo_set_edges: needs at least one edge, its vertices and its measurement"); return CS_ERR_INVALID_ARG; }
  CS_GUARD_BEGIN
  std::vector<long long> keys((size_t)n);
  for (int k = 0; k < n; k++) {
    if (vi[k] < 0 || vi[k] >= G->nv || vj[k] < 0 || vj[k] >= G->nv) { cs_set_error("cs_pgo_set_edges: edge " + std::to_string(k) + " names a vertex out of range"); return CS_ERR_INVALID_ARG; }
    if (vi[k] == vj[k]) { cs_set_error("cs_pgo_set_edges: edge " + std::to_string(k) + " joins a vertex to itself"); return CS_ERR_INVALID_ARG; }
    keys[k] = (long long)std::min(vi[k], vj[k]) * G->nv + std::max(vi[k], vj[k]);
  }
  std::sort(keys.begin(), keys.end());
  for (int k = 1; k < n; k++)
    if (keys[k] == keys[k - 1]) {
      cs_set_error("cs_pgo_set_edges: two edges between vertices " + std::to_string(keys[k] / G->nv) + " and " + std::to_string(keys[k] % G->nv) + " (parallel edges are refused, in either orientation)");
      return CS_ERR_INVALID_ARG;
    }
  rc = check_states("cs_pgo_set_edges", meas8, n, "the measurement of edge"); if (rc) return rc;
  if (info49)
    for (size_t t = 0; t < 49 * (size_t)n; t++) if (!std::isfinite(info49[t])) { cs_set_error("cs_pgo_set_edges: the information of edge " + std::to_string(t / 49) + " is not finite"); return CS_ERR_INVALID_ARG; }
  CS_HIP_TRY(hipSetDevice(G->device));
  G->have_edges = false; G->ran = false;
  G->ne = n;
  std::vector<double> info(49 * (size_t)n, 0.0);
  if (info49) std::memcpy(info.data(), info49, info.size() * sizeof(double));
  else for (int k = 0; k < n; k++) for (int d = 0; d < 7; d++) info[49 * (size_t)k + 8 * d] = 1.0;
  if ((rc = upload(G->meas, meas8, 8 * (size_t)n, G->st)) || (rc = upload(G->info, info, G->st))) return rc;
  rc = build_structure(G, std::vector<int>(vi, vi + n), std::vector<int>(vj, vj + n)); if (rc) return rc;
  G->have_edges = true;
  return CS_OK;
  CS_GUARD_END("cs_pgo_set_edges")
}

int cs_pgo_set_lm_params(cs_pgo* G, double user_lambda_init, int max_trials_after_failure) {
  if (!G || max_trials_after_failure < 1 || !(user_lambda_init == user_lambda_init)) return CS_ERR_INVALID_ARG;
  G->user_lambda_init = user_lambda_init; G->max_trials = max_trials_after_failure;
  return CS_OK;
}

int cs_pgo_chi2(cs_pgo* G, double* chi2, double* chi2_each) {
  int rc = need(G, "cs_pgo_chi2", true); if (rc) return rc;
  CS_HIP_TRY(hipSetDevice(G->device));
  const cs::PgoView v = view_of(G);
  cs::pgo_launch_errors(v, G->st);
  cs::pgo_launch_chi2(v, G->st);
  CS_HIP_TRY(hipGetLastError());
  if (chi2_each) CS_HIP_TRY(hipMemcpyAsync(chi2_each, G->chi2_each.p, sizeof(double) * (size_t)G->ne, hipMemcpyDeviceToHost, G->st));
  rc = fetch_record(G); if (rc) return rc;
  if (chi2) *chi2 = G->h_rec.p[0];
  return CS_OK;
}

int cs_pgo_linearize_edges(cs_pgo* G, double* err7, double* Ji49, double* Jj49) {
  int rc = need(G, "cs_pgo_linearize_edges", true); if (rc) return rc;
  CS_HIP_TRY(hipSetDevice(G->device));
  rc = linearize(G); if (rc) return rc;
  const size_t E = (size_t)G->ne;
  if (err7) CS_HIP_TRY(hipMemcpyAsync(err7, G->err.p, 7 * E * sizeof(double), hipMemcpyDeviceToHost, G->st));
  if (Ji49) CS_HIP_TRY(hipMemcpyAsync(Ji49, G->Ji.p, 49 * E * sizeof(double), hipMemcpyDeviceToHost, G->st));
  if (Jj49) CS_HIP_TRY(hipMemcpyAsync(Jj49, G->Jj.p, 49 * E * sizeof(double), hipMemcpyDeviceToHost, G->st));
  CS_HIP_TRY(hipStreamSynchronize(G->st));
  return CS_OK;
}

int cs_pgo_edge_terms(cs_pgo* G, double* Hii49, double* Hij49, double* Hjj49, double* bi7, double* bj7, double* chi2_each) {
  int rc = need(G, "cs_pgo_edge_terms", true); if (rc) return rc;
  CS_HIP_TRY(hipSetDevice(G->device));
  rc = linearize(G); if (rc) return rc;
  const size_t E = (size_t)G->ne;
  const struct { double* dst; const double* src; size_t n; } out[6] = {{Hii49, G->Hii.p, 49 * E}, {Hij49, G->Hij.p, 49 * E}, {Hjj49, G->Hjj.p, 49 * E},
                                                                      {bi7, G->bi.p, 7 * E}, {bj7, G->bj.p, 7 * E}, {chi2_each, G->chi2_each.p, E}};
  for (const auto& o : out)
    if (o.dst) CS_HIP_TRY(hipMemcpyAsync(o.dst, o.src, o.n * sizeof(double), hipMemcpyDeviceToHost, G->st));
  CS_HIP_TRY(hipStreamSynchronize(G->st));
  return CS_OK;
}

// optimization_algorithm_levenberg.cpp:61-163 (the policy: cs_lm.h) + sparse_optimizer.cpp:354-419
int cs_pgo_optimize(cs_pgo* G, int iterations, int* iterations_done, double* chi2_hist, double* lambda_hist, int* trials_hist, int hist_cap) {
  int rc = need(G, "cs_pgo_optimize", true); if (rc) return rc;
  if (iterations < 0) return CS_ERR_INVALID_ARG;
  CS_HIP_TRY(hipSetDevice(G->device));
  const double t_begin = now_ms();
  G->linearize_ms = G->solve_ms = 0;
  int done = 0;
  cs::LmState lm;
  const cs::PgoView v = view_of(G);
  const size_t est_bytes = 8 * (size_t)G->nv * sizeof(double);
  for (int it = 0; it < iterations && G->n > 0; it++) {
    double t0 = now_ms();
    rc = linearize(G); if (rc) return rc;
    if (it == 0 && !(G->user_lambda_init > 0)) { cs::pgo_launch_assemble(v, 0.0, G->st); CS_HIP_TRY(hipGetLastError()); }   // (for max |H_jj|; S is cleared by the first solve)
    rc = fetch_record(G); if (rc) return rc;
    G->linearize_ms += now_ms() - t0;
    double currentChi = G->h_rec.p[0];
    const double iniChi = currentChi;
    if (it == 0) cs::lm_begin(lm, G->user_lambda_init, G->h_rec.p[2]);
    double rho = 0;
    int qmax = 0;
    do {
      t0 = now_ms();
      CS_HIP_TRY(hipMemcpyAsync(G->est_bak.p, G->est.p, est_bytes, hipMemcpyDeviceToDevice, G->st));       // push
      std::unique_lock<std::mutex> turn;
      rc = solve(G, lm.lambda, &turn); if (rc) return rc;
      cs::pgo_launch_scale(v, lm.lambda, G->st);
      cs::pgo_launch_update(v, G->st);
      cs::pgo_launch_errors(v, G->st);
      cs::pgo_launch_chi2(v, G->st);
      CS_HIP_TRY(hipGetLastError());
      rc = fetch_record(G); if (rc) return rc;
      if (turn.owns_lock()) turn.unlock();
      G->solve_ms += now_ms() - t0;
      const cs::SparseVerdict verdict = cs::sparse_verdict(G->h_status.p);
      if (verdict == cs::SPARSE_TIMEOUT) { cs_set_error("cs_pgo: sparse solver: grid not co-resident (wait timed out); set CS_PGO_FORCE_DENSE=1 on a shared device"); return CS_ERR_HIP; }
      if (!cs::lm_trial(lm, currentChi, G->h_rec.p[0], G->h_rec.p[1], verdict == cs::SPARSE_OK, rho))      // (a non-positive pivot: a failed trial)
        CS_HIP_TRY(hipMemcpyAsync(G->est.p, G->est_bak.p, est_bytes, hipMemcpyDeviceToDevice, G->st));     // pop
      qmax++;
    } while (cs::lm_again(rho, qmax, G->max_trials));
    if (done < hist_cap) {
      if (chi2_hist) chi2_hist[done] = currentChi;
      if (lambda_hist) lambda_hist[done] = lm.lambda;
      if (trials_hist) trials_hist[done] = qmax;
    }
    done++;
    if (cs::lm_stop(lm, rho, qmax, G->max_trials, iniChi, currentChi)) break;
  }
  CS_HIP_TRY(hipStreamSynchronize(G->st));
  if (iterations_done) *iterations_done = done;
  G->total_ms = now_ms() - t_begin;
  G->ran = true;
  return CS_OK;
}

int cs_pgo_get_vertices(cs_pgo* G, double* sim8) {
  int rc = need(G, "cs_pgo_get_vertices", false); if (rc) return rc;
  if (!sim8) return CS_ERR_INVALID_ARG;
  CS_HIP_TRY(hipSetDevice(G->device));
  CS_HIP_TRY(hipMemcpyAsync(sim8, G->est.p, 8 * (size_t)G->nv * sizeof(double), hipMemcpyDeviceToHost, G->st));
  CS_HIP_TRY(hipStreamSynchronize(G->st));
  return CS_OK;
}

int cs_pgo_get_se3(cs_pgo* G, double* Tcw7) {
  int rc = need(G, "cs_pgo_get_se3", false); if (rc) return rc;
  if (!Tcw7) return CS_ERR_INVALID_ARG;
  CS_HIP_TRY(hipSetDevice(G->device));
  rc = G->io.ensure(7 * (size_t)G->nv); if (rc) return rc;
  cs::pgo_launch_se3(G->est.p, G->nv, G->io.p, G->st);
  CS_HIP_TRY(hipGetLastError());
  CS_HIP_TRY(hipMemcpyAsync(Tcw7, G->io.p, 7 * (size_t)G->nv * sizeof(double), hipMemcpyDeviceToHost, G->st));
  CS_HIP_TRY(hipStreamSynchronize(G->st));
  return CS_OK;
}

int cs_pgo_correct_points(cs_pgo* G, int n, const int* ref_vertex, const double* xyz_in, double* xyz_out) {
  int rc = need(G, "cs_pgo_correct_points", false); if (rc) return rc;
  if (n < 0 || (n > 0 && (!ref_vertex || !xyz_in || !xyz_out))) return CS_ERR_INVALID_ARG;
  for (int p = 0; p < n; p++)
    if (ref_vertex[p] < 0 || ref_vertex[p] >= G->nv) { cs_set_error("cs_pgo_correct_points: point " + std::to_string(p) + " names a reference vertex out of range"); return CS_ERR_INVALID_ARG; }
  if (n == 0) return CS_OK;
  CS_HIP_TRY(hipSetDevice(G->device));
  if ((rc = G->io.ensure(6 * (size_t)n)) || (rc = upload(G->io_i, ref_vertex, (size_t)n, G->st))) return rc;
  CS_HIP_TRY(hipMemcpyAsync(G->io.p, xyz_in, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, G->st));
  cs::pgo_launch_correct_points(G->est_init.p, G->est.p, n, G->io_i.p, G->io.p, G->io.p + 3 * (size_t)n, G->st);
  CS_HIP_TRY(hipGetLastError());
  CS_HIP_TRY(hipMemcpyAsync(xyz_out, G->io.p + 3 * (size_t)n, 3 * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, G->st));
  CS_HIP_TRY(hipStreamSynchronize(G->st));
  return CS_OK;
}

int cs_pgo_solver_path(cs_pgo* G, int* path, double* sparse_fill) {
  int rc = need(G, "cs_pgo_solver_path", true); if (rc) return rc;
  if (path) *path = G->sparse ? CS_BA_PATH_SPARSE : CS_BA_PATH_DENSE;
  if (sparse_fill) *sparse_fill = G->sparse ? G->solver.fill(G->n) : 0.0;
  return CS_OK;
}

int cs_pgo_last_timing(cs_pgo* G, double* linearize_ms, double* solve_ms, double* total_ms) {
  if (!G) return CS_ERR_INVALID_ARG;
  if (!G->ran) return CS_ERR_NOT_RUN;
  if (linearize_ms) *linearize_ms = G->linearize_ms;
  if (solve_ms) *solve_ms = G->solve_ms;
  if (total_ms) *total_ms = G->total_ms;
  return CS_OK;
}

}  // extern "C"
