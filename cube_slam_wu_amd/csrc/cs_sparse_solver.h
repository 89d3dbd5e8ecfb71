// cs_sparse_solver.h -- the host side of the general sparse Cholesky (plan: ba_sparse.h, kernels: sparse_kernels.hip), owned once: the
// plan and its launch grids, the plan's tables on the device, the workspace, the status words, and the sequence a damped solve queues.
// The bundle adjustment's reduced system (ba_lm.cpp) and the pose graph's H + lambda I (pgo_host.cpp) each hold one.
#pragma once
#include <rocblas/rocblas.h>
#include <rocsolver/rocsolver.h>
#include <cstring>

#include "ba_sparse.h"
#include "cs_hip_util.h"

#define CS_ROC_TRY(expr) do { rocblas_status _s = (expr); if (_s != rocblas_status_success) { cs_set_error(std::string(#expr) + ": rocblas status " + std::to_string((int)_s)); return CS_ERR_HIP; } } while (0)

namespace cs {
// a rocBLAS handle bound to one stream, destroyed with its holder (which declares it behind that stream); not copyable
struct BlasHandle {
  rocblas_handle h = nullptr;
  BlasHandle() = default;
  BlasHandle(const BlasHandle&) = delete;
  BlasHandle& operator=(const BlasHandle&) = delete;
  ~BlasHandle() { if (h) (void)rocblas_destroy_handle(h); }
  int create(hipStream_t st) { CS_ROC_TRY(rocblas_create_handle(&h)); CS_ROC_TRY(rocblas_set_stream(h, st)); return CS_OK; }
  operator rocblas_handle() const { return h; }
};

struct SparseSolver {
  SparsePlan plan; SparseGrids grids{0, 0};
  enum { NDIM, NCOL, SPTR, SROW, SROFF, PROW, RBASE, RENT, RPTR, RCOL, RPOS, ORDER, TCOL, N_TABLES };
  size_t at[N_TABLES] = {};        // first entry of each table in `tab`, behind poff (long long: it sits first, 8-byte aligned)
  PinBuf<int> h_tab;
  DevBuf<int> tab, info;           // info: [first non-positive pivot + 1 or the time-out code, abort word, the tail's rocblas_int info]
  DevBuf<double> L, xs, T;         // panels; the solution by position; the tail's block and its right-hand side
  DevBuf<unsigned> done, xdone;
  static_assert(sizeof(rocblas_int) == sizeof(int), "the tail's info shares the status words' buffer");
  // sparse_plan_build, then sparse_grids (current device); false where either refuses.  Nothing is on the device before upload(): the caller may still decline.
  bool build(const std::vector<std::vector<int>>& adj, const std::vector<int>& verts, const std::vector<int>& dim, const std::vector<int>& col, double max_fill, int max_tail_unknowns) {
    grids = SparseGrids{0, 0};
    return sparse_plan_build(adj, verts, dim, col, sparse_max_panel_doubles(), max_fill, plan, max_tail_unknowns) && sparse_grids(sparse_max_panel_doubles(), plan.N, &grids);
  }
  // The plan's tables, packed into one pinned array, go to the device as ONE copy queued on st; the workspace is sized, without a fill (the
  // kernels write L and xs before they read them; the launcher clears done / xdone / T and solve() the status words, per solve).  The caller
  // waits for st before it builds or uploads again (both structure phases end with that wait): the next upload repacks the pinned array.
  int upload(hipStream_t st) {
    const std::vector<int>* tables[N_TABLES] = {&plan.ndim, &plan.ncol, &plan.sptr, &plan.srow, &plan.sroff, &plan.prow, &plan.rbase, &plan.rent, &plan.rptr, &plan.rcol, &plan.rpos, &plan.order, &plan.tcol};
    size_t total = 2 * plan.poff.size();
    for (int t = 0; t < N_TABLES; t++) { at[t] = total; total += tables[t]->size(); }
    const size_t N = (size_t)plan.N, nt = (size_t)plan.n_tail; int rc;
    if ((rc = h_tab.ensure(total)) || (rc = tab.ensure(total)) || (rc = info.ensure(3)) || (rc = L.ensure((size_t)plan.nvals)) || (rc = xs.ensure(9 * (N + 1))) ||
        (rc = T.ensure(nt * nt + nt + 1)) || (rc = done.ensure(N + 1)) || (rc = xdone.ensure(N + 2))) return rc;
    std::memcpy(h_tab.p, plan.poff.data(), plan.poff.size() * sizeof(long long));
    for (int t = 0; t < N_TABLES; t++) if (!tables[t]->empty()) std::memcpy(h_tab.p + at[t], tables[t]->data(), tables[t]->size() * sizeof(int));
    CS_HIP_TRY(hipMemcpyAsync(tab.p, h_tab.p, total * sizeof(int), hipMemcpyHostToDevice, st));
    return CS_OK;
  }
  SparseView view(const double* S, double* rhs, int n) const {
    SparseView V;
    const int* t = tab.p; V.N = plan.N; V.n = n; V.poff = reinterpret_cast<const long long*>(t);
    V.ndim = t + at[NDIM]; V.ncol = t + at[NCOL]; V.sptr = t + at[SPTR]; V.srow = t + at[SROW]; V.sroff = t + at[SROFF]; V.prow = t + at[PROW]; V.rbase = t + at[RBASE];
    V.rent = t + at[RENT]; V.rptr = t + at[RPTR]; V.rcol = t + at[RCOL]; V.rpos = t + at[RPOS]; V.order = t + at[ORDER]; V.tcol = t + at[TCOL];
    V.tail_start = plan.tail_start; V.n_tail = plan.n_tail; V.T = T.p; V.rhs_t = T.p + (size_t)V.n_tail * V.n_tail;
    V.S = S; V.rhs = rhs; V.L = L.p; V.xs = xs.p; V.done = done.p; V.xdone = xdone.p; V.info = info.p;
    return V;
  }
  // One damped solve of the n x n system S (dense, lower triangle, row-major), rhs in, solution out: the status clears, the factorisation,
  // the dense tail's potrf / potrs, the substitution -- queued on st (blas is bound to it), nothing waited for.  The persistent kernels'
  // turn (cs::coop_mutex) is the caller's, held until it has seen them finish.  Returns CS_OK, an error with its message set, or one of
  // these two where a launcher refused -- the caller words that message.
  enum { CHOL_NOT_LAUNCHED = 1, BACK_NOT_LAUNCHED = 2 };
  int solve(rocblas_handle blas, const double* S, double* rhs, int n, hipStream_t st) {
    const SparseView V = view(S, rhs, n);
    CS_HIP_TRY(hipMemsetAsync(info.p, 0, 3 * sizeof(int), st));
    if (!launch_sparse_cholesky(V, sparse_max_panel_doubles(), grids, st)) return CHOL_NOT_LAUNCHED;
    if (V.n_tail > 0) {   // (the lower triangle of the row-major T is the upper triangle of the column-major matrix rocSOLVER sees)
      CS_ROC_TRY(rocsolver_dpotrf(blas, rocblas_fill_upper, V.n_tail, V.T, V.n_tail, info.p + 2));
      CS_ROC_TRY(rocsolver_dpotrs(blas, rocblas_fill_upper, V.n_tail, 1, V.T, V.n_tail, V.rhs_t, V.n_tail));
    }
    return launch_sparse_backsolve(V, grids, st) ? CS_OK : BACK_NOT_LAUNCHED;
  }
  int queue_status(int* pinned2, hipStream_t st) {      // [the factorisation's status word, the tail's pivot], for sparse_verdict() once st has run
    CS_HIP_TRY(hipMemcpyAsync(pinned2, info.p, sizeof(int), hipMemcpyDeviceToHost, st));
    CS_HIP_TRY(hipMemcpyAsync(pinned2 + 1, info.p + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    return CS_OK;
  }
  double fill(int n) const { return (double)plan.nvals / (0.5 * (double)n * (double)n); }
};

// the two words of queue_status() (pgo_host.cpp's dense path feeds [0, rocSOLVER's info]); PIVOT: not positive definite, a failed trial; TIMEOUT: the grid was not co-resident
enum SparseVerdict { SPARSE_OK, SPARSE_PIVOT, SPARSE_TIMEOUT };
inline SparseVerdict sparse_verdict(const int* h) { return h[0] == 0x7fffffff ? SPARSE_TIMEOUT : (h[0] == 0 && h[1] == 0) ? SPARSE_OK : SPARSE_PIVOT; }

}  // namespace cs
