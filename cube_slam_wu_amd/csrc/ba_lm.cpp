// ba_lm.cpp -- the numeric half of the bundle adjustment's host side: the stepwise calls (cs_ba_compute_errors, _build_system, _solve, _update,
// _push, _pop), the damped solve of the reduced system in its four forms (banded / block cyclic reduction, sparse, dense, separator mode), the
// collectives of a sharded run, and cs_ba_optimize's Levenberg-Marquardt loop.  Every numeric step is a HIP kernel on resident data; the LM
// control flow is scalar host code (cs_lm.h) fed by one read-back per trial.  Which flow a trial takes is decided in ba_trial_plan.h; the handle
// and the structure phase that fills it are ba_handle.h's and ba_host.cpp's.  There is no CPU fallback.
#include "ba_handle.h"
#include "ba_trial_plan.h"

namespace {

using cs::now_ms;

int chi2_device(cs_ba* B, double* chi) {
  cs::ba_launch_chi2(B->view, B->nb_chi, B->st);
  CS_HIP_TRY(hipGetLastError());
  std::vector<double> part(B->n_chi_partials);
  CS_HIP_TRY(hipMemcpyAsync(part.data(), B->chi_partial.p, sizeof(double) * part.size(), hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  double s = 0;
  for (double p : part) s += p;  // fixed order
  *chi = s;
  return CS_OK;
}

// b (poses then landmarks) to the host: LM's scale term needs it (optimization_algorithm_levenberg.cpp:182-189)
int fetch_b(cs_ba* B) {
  B->h_b.assign(B->n_pose + 3 * (size_t)B->n_lm, 0.0);
  std::vector<double> bc(6 * (size_t)B->nc), bo(9 * (size_t)B->no), bl(3 * (size_t)B->np);
  if (B->nc) CS_HIP_TRY(hipMemcpyAsync(bc.data(), B->bcam.p, 8 * bc.size(), hipMemcpyDeviceToHost, B->st));
  if (B->no) CS_HIP_TRY(hipMemcpyAsync(bo.data(), B->bcub.p, 8 * bo.size(), hipMemcpyDeviceToHost, B->st));
  if (B->np) CS_HIP_TRY(hipMemcpyAsync(bl.data(), B->bl.p, 8 * bl.size(), hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  for (int i = 0; i < B->nc; i++) if (B->cam_col[i] >= 0) std::memcpy(&B->h_b[B->cam_col[i]], &bc[6 * (size_t)i], 48);
  for (int i = 0; i < B->no; i++) if (B->cub_col[i] >= 0) std::memcpy(&B->h_b[B->cub_col[i]], &bo[9 * (size_t)i], 72);
  for (int i = 0; i < B->np; i++) if (B->pt_lm[i] >= 0) std::memcpy(&B->h_b[B->n_pose + 3 * (size_t)B->pt_lm[i]], &bl[3 * (size_t)i], 24);
  return CS_OK;
}

int fetch_x(cs_ba* B) {
  B->h_x.assign(B->n_pose + 3 * (size_t)B->n_lm, 0.0);
  std::vector<double> xl(3 * (size_t)B->np);
  if (B->n_pose) CS_HIP_TRY(hipMemcpyAsync(B->h_x.data(), B->view.rhs, 8 * (size_t)B->n_pose, hipMemcpyDeviceToHost, B->st));
  if (B->np) CS_HIP_TRY(hipMemcpyAsync(xl.data(), B->xl.p, 8 * xl.size(), hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  for (int i = 0; i < B->np; i++) if (B->pt_lm[i] >= 0) std::memcpy(&B->h_x[B->n_pose + 3 * (size_t)B->pt_lm[i]], &xl[3 * (size_t)i], 24);
  return CS_OK;
}

// phase times come from events read after the next stream synchronisation, so that no phase boundary stalls the host
int collect_lin_time(cs_ba* B) {
  if (!B->stage_timing) { B->lin_pending = false; return CS_OK; }
  if (!B->lin_pending) return CS_OK;
  float ms = 0;
  CS_HIP_TRY(hipEventElapsedTime(&ms, B->ev[0], B->ev[1]));
  B->tm.linearize_ms += ms;
  B->lin_pending = false;
  return CS_OK;
}

int build_system_device(cs_ba* B, hipEvent_t ev_pre = nullptr) {
  BA_MARK(B, B->ev[0]);
  cs::ba_launch_linearize(B->view, B->st, B->st2, B->ev_fork, B->ev_join, B->st3, B->ev_join3, ev_pre);
  if (B->ext_terms_set) {
    if (B->ext_cam36.n != 36 * (size_t)B->nc || B->ext_cub81.n != 81 * (size_t)B->no || B->ext_pt9.n != 9 * (size_t)B->np) { cs_set_error("external terms were set for a graph of another size: call cs_ba_set_external_terms again"); return CS_ERR_INVALID_ARG; }
    cs::ba_launch_ext_add(B->view, B->ext_has_cam ? B->ext_cam36.p : nullptr, B->ext_cam6.p, B->ext_has_cub ? B->ext_cub81.p : nullptr, B->ext_cub9.p,
                          B->ext_has_pt ? B->ext_pt9.p : nullptr, B->ext_pt3.p, B->st);
  }
  CS_HIP_TRY(hipGetLastError());
  BA_MARK(B, B->ev[1]);
  B->lin_pending = true;
  B->tm.n_linearizations++;
  B->have_system = true;
  return CS_OK;
}

// The banded factorisation is a persistent kernel whose workgroups wait for each other: all of them must be resident.
// One such kernel fits many times over, but an unbounded number of concurrent solves (handles on different streams of
// one process) would not; they take turns.
static std::mutex& g_coop_mutex = cs::coop_mutex();   // (cs_hip_util.h: the pose-graph handle's sparse solve takes the same turn)

// What ba_trial_plan.h's switches are decided from: the handle, the environment and the callback a call came with, read HERE and nowhere else.
cs::TrialFacts trial_facts(const cs_ba* B, cs_allreduce_fn fn) {
  cs::TrialFacts f;
  f.callback_given = fn != nullptr; f.comm_present = B->comm != nullptr;
  f.shard_n = B->shard_n; f.band_ld = B->band_ld; f.n_red = B->n_red;
  f.sparse = B->sparse; f.use_bcr = B->use_bcr; f.sep_mode = B->sep_mode; f.elim = B->elim; f.fused = B->fused;
  f.has_proj = B->n_proj > 0;
  f.seg_classes_full = B->n_seg == *std::max_element(B->seg_class, B->seg_class + 5);
  f.ext_edges = B->ext_n > 0; f.ext_terms_set = B->ext_terms_set; f.ext_fn_set = B->ext_fn != nullptr;
  f.stage_timing = B->stage_timing;
  f.h_trial_present = B->h_trial.p != nullptr;
  { const char* e = getenv("CS_BA_FUSE_LIN"); f.fuse_lin_env = !e || atoi(e) != 0; }     // (read per call: the tests hold the two paths to each other in one process)
  f.nan_env_present = getenv("CS_BA_DEBUG_NAN") != nullptr;
  f.nan_scans_on = debug_nan_enabled();
  return f;
}

// phase times of the last solve, read once the stream has been synchronised (sharded_sep: the separator-mode solve's own marks too)
int collect_solve_times(cs_ba* B, bool sharded_sep) {
  if (!B->stage_timing) { B->lin_pending = false; return CS_OK; }
  float ms = 0;
  CS_HIP_TRY(hipEventElapsedTime(&ms, B->ev[2], B->ev[3])); B->tm.reduce_ms += ms;
  CS_HIP_TRY(hipEventElapsedTime(&ms, B->ev[3], B->ev[4])); B->tm.factor_ms += ms;
  CS_HIP_TRY(hipEventElapsedTime(&ms, B->ev[4], B->ev[5])); B->tm.backsub_ms += ms;
  if (sharded_sep) {
    hipEvent_t seq[6] = {B->ev[3], B->sev[0], B->sev[1], B->sev[2], B->sev[3], B->ev[4]};
    for (int i = 0; i < 5; i++) { CS_HIP_TRY(hipEventElapsedTime(&ms, seq[i], seq[i + 1])); B->sep_ms[i] += ms; }
  }
  return collect_lin_time(B);
}

// Collectives of a sharded run, as one call received them: the caller's callback (host-synchronous: the stream is drained first), or RCCL on
// the handle's stream (queued, no host round trip) when no callback came and the handle holds a communicator.  Which of the two counts is
// ba_trial_plan.h's coll_kind.  Every failure text of a collective is set here and nowhere else.
struct Collectives {
  cs_ba* B; cs_allreduce_fn fn; void* ctx;
  cs::CollKind kind;
  Collectives(cs_ba* B_, cs_allreduce_fn fn_, void* ctx_) : B(B_), fn(fn_), ctx(ctx_), kind(cs::coll_kind(trial_facts(B_, fn_))) {}
  bool active() const { return kind != cs::CollKind::none; }
  // host scalars: sum (op 0) / max (op 1) over the ranks
  int host_reduce(double* v, size_t n, int op) {
    if (reduce_scalars(v, n, op) == 0) return CS_OK;
    cs_set_error("all-reduce failed");
    return CS_ERR_HIP;
  }
  // device memory, in place, summed over the ranks
  int device_allreduce(double* d, size_t n) {
    if (kind == cs::CollKind::callback) return through_callback(d, n);
    if (kind == cs::CollKind::rccl) BA_NCCL(ncclAllReduce(d, d, n, ncclDouble, ncclSum, B->comm, B->st));
    return CS_OK;
  }
  // in place: rank r's part sits at buf + r * per_rank.  Through the callback an all-gather is the sum of the zero-padded buffers
  // (the caller zeroes the other ranks' slots first).
  int device_allgather(double* buf, size_t per_rank) {
    if (kind == cs::CollKind::callback) return through_callback(buf, per_rank * (size_t)B->shard_n);
    if (kind == cs::CollKind::rccl) BA_NCCL(ncclAllGather(buf + (size_t)B->shard_rank * per_rank, buf, per_rank, ncclDouble, B->comm, B->st));
    return CS_OK;
  }

 private:
  int through_callback(double* d, size_t n) {
    CS_HIP_TRY(hipStreamSynchronize(B->st));
    if (fn(ctx, d, n, 1, 0) != 0) { cs_set_error("all-reduce callback failed"); return CS_ERR_HIP; }
    return CS_OK;
  }
  int reduce_scalars(double* v, size_t n, int op) {      // 0: done
    if (kind == cs::CollKind::callback) return fn(ctx, v, n, 0, op);
    if (kind == cs::CollKind::rccl) {
      if (n > B->h_scalars.cap) return 1;
      std::memcpy(B->h_scalars.p, v, n * sizeof(double));
      if (hipMemcpyAsync(B->d_scalars.p, B->h_scalars.p, n * sizeof(double), hipMemcpyHostToDevice, B->st) != hipSuccess) return 1;
      if (ncclAllReduce(B->d_scalars.p, B->d_scalars.p, n, ncclDouble, op == 0 ? ncclSum : ncclMax, B->comm, B->st) != ncclSuccess) return 1;
      if (hipMemcpyAsync(B->h_scalars.p, B->d_scalars.p, n * sizeof(double), hipMemcpyDeviceToHost, B->st) != hipSuccess) return 1;
      if (hipStreamSynchronize(B->st) != hipSuccess) return 1;
      std::memcpy(v, B->h_scalars.p, n * sizeof(double));
    }
    return 0;
  }
};

// Sharded with the cuboids eliminated: a cuboid's increment is computed by the rank that owns it (zero elsewhere); every rank updates
// all vertices, so the increments (9 doubles per free cuboid, behind the reduced system's in `rhs`) are summed over the ranks.
int share_cuboid_increments(cs_ba* B, Collectives& coll) {
  if (!B->elim || B->shard_n <= 1 || B->n_pose <= B->n_red) return CS_OK;
  return coll.device_allreduce(B->view.rhs + B->n_red, (size_t)(B->n_pose - B->n_red));
}

// A workgroup of a persistent factorisation waited ~1 s for its team (band_wait_ge): the device is shared with another persistent kernel.
// h_status[0]: the band's / the interior's word; with_sep: h_status[2], the separator system's, counts too.
int check_band_timeout(const cs_ba* B, bool with_sep) {
  if (B->h_status.p[0] != cs::BAND_TIMEOUT_INFO && !(with_sep && B->h_status.p[2] == cs::BAND_TIMEOUT_INFO)) return CS_OK;
  cs_set_error("banded solver: team not co-resident (wait timed out); set CS_BA_FORCE_DENSE=1 on a shared device");
  return CS_ERR_HIP;
}

// The shared head of a damped solve outside separator mode: lambda, [S | rhs] and the failure words cleared, the Schur complement, the
// external edges' off-diagonal blocks, the ranks' partial systems summed.
int queue_reduce(cs_ba* B, Collectives& coll, const cs::SolveHead& head, double lambda) {
  cs::BaSidePrologue side_pro{};
  if (head.lean_head) {
    B->h_lam.p[0] = lambda; B->h_lam.p[1] = B->shard_rank == 0 ? lambda : 0.0;
    side_pro = cs::BaSidePrologue{B->d_lam.p, B->h_lam.p[0], B->h_lam.p[1], B->d_band_info.p, B->d_elim_fail.p, B->S.p, B->s_doubles + (size_t)B->n_pose};
    if (!head.pro_in_reduce) cs::ba_launch_trial_prologue(B->d_lam.p, B->h_lam.p[0], B->h_lam.p[1], B->d_band_info.p, B->d_elim_fail.p, B->S.p, B->s_doubles + (size_t)B->n_pose, B->st);   // (+ [S | rhs] cleared: no fill of its own)
  } else CS_TRY(put_lambda(B, lambda));
  BA_MARK(B, B->ev[2]);
  if (!head.lean_head) {
    if (B->sparse && B->S_clean) {
      // (sparse path: S was cleared by the structure phase and only the plan's pattern is ever written -- the pattern and the right-hand side)
      cs::launch_sparse_zero_pattern(B->solver.view(B->S.p, B->view.rhs, B->n_red), B->S.p, B->st);
      CS_HIP_TRY(hipMemsetAsync(B->S.p + B->s_doubles, 0, sizeof(double) * B->n_pose, B->st));
    } else {
      CS_HIP_TRY(hipMemsetAsync(B->S.p, 0, sizeof(double) * (B->s_doubles + B->n_pose), B->st));
      B->S_clean = B->sparse;
    }
    CS_HIP_TRY(hipMemsetAsync(B->d_elim_fail.p, 0, sizeof(int), B->st));
  }
  cs::ba_launch_reduce(B->view, B->d_lam.p, B->st, B->st2, B->ev_fork, B->ev_join, head.pro_in_reduce ? &side_pro : nullptr);
  if (B->ext_n > 0 && B->ext_terms_set) cs::ba_launch_ext_offdiag(B->view, B->ext_groups, B->d_ext_gptr.p, B->d_ext_order.p, B->d_ext_e4.p, B->ext_Hij.p, B->st);
  if (head.status_in_scalars) { B->h_status.p[0] = 0; B->h_status.p[1] = 0; }
  else CS_HIP_TRY(hipMemcpyAsync(B->h_status.p + 1, B->d_elim_fail.p, sizeof(int), hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipGetLastError());
  if (head.sum_ranks) CS_TRY(coll.device_allreduce(B->S.p, B->s_doubles + B->n_pose));      // [S | rhs] in one message
  BA_MARK(B, B->ev[3]);
  return CS_OK;
}

// banded: factorisation, both substitutions and the landmark back-substitution are queued back to back; the pivot flag comes home with the
// single synchronisation (a failed factorisation just leaves garbage increments that the caller discards).
// turn_out (a deferred solve): everything is queued and the function returns WITHOUT synchronising; *turn_out then holds the persistent-kernel
// turn, and the caller synchronises, reads *h_status, calls collect_solve_times() and releases the turn.
int solve_banded(cs_ba* B, Collectives& coll, const cs::SolveHead& head, bool* ok, std::unique_lock<std::mutex>* turn_out) {
  const int n = B->n_red;
  std::unique_lock<std::mutex> coop_turn(g_coop_mutex);
  if (B->use_bcr) cs::ba_launch_bcr(B->S.p, B->band_linv.p, n, B->band_ld, 128, B->view.rhs, B->d_band_info.p, B->st);
  else cs::ba_launch_band_cholesky(B->S.p, B->band_linv.p, n, B->band_ld, B->view.rhs, B->d_band_info.p, true, B->st);
  CS_HIP_TRY(hipGetLastError());
  BA_MARK(B, B->ev[4]);
  // (Round 5 tried clearing the band for the NEXT trial on the side stream here -- block cyclic reduction is done with it after its first
  // level -- to take the 10 us fill off the head of a trial: the event record / wait / fill / record sequence stalled the host's enqueue of the
  // kernels behind it by 35-60 us each, profiles/r5_ba_timeline_prezero.txt; the fill stays at the head.)
  cs::ba_launch_backsub(B->view, B->st);
  CS_HIP_TRY(hipGetLastError());
  if (coll.kind == cs::CollKind::callback && B->elim) {   // the callback waits for the other ranks: the persistent kernel's turn must be free by then
    CS_HIP_TRY(hipStreamSynchronize(B->st));
    coop_turn.unlock();
  }
  CS_TRY(share_cuboid_increments(B, coll));
  BA_MARK(B, B->ev[5]);
  if (!head.status_in_scalars) CS_HIP_TRY(hipMemcpyAsync(B->h_status.p, B->d_band_info.p, sizeof(int), hipMemcpyDeviceToHost, B->st));
  if (turn_out) { *turn_out = std::move(coop_turn); return CS_OK; }   // (the caller's sum kernel folds the two status words into the trial's scalars)
  cs::ba_launch_fail_flag(B->d_band_info.p, B->d_elim_fail.p, nullptr, B->d_scalars.p + 2, B->st);
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  CS_TRY(check_band_timeout(B, false));
  if (B->h_status.p[0] != 0 || B->h_status.p[1] != 0) *ok = false;
  return CS_OK;
}

// general sparse: the pattern's blocks are gathered from the dense S by the factorisation itself (sparse_kernels.hip)
int solve_sparse(cs_ba* B, Collectives& coll, bool* ok) {
  std::unique_lock<std::mutex> coop_turn(g_coop_mutex);
  const cs::SparseSolver& sv = B->solver; const int rs = B->solver.solve(B->blas, B->S.p, B->view.rhs, B->n_red, B->st);
  if (rs == cs::SparseSolver::CHOL_NOT_LAUNCHED) { cs_set_error("sparse solver: the factorisation could not be launched (grid " + std::to_string(sv.grids.chol) + " for " + std::to_string(sv.plan.N) + " vertices)"); return CS_ERR_HIP; }
  if (rs == cs::SparseSolver::BACK_NOT_LAUNCHED) { cs_set_error("sparse solver: the substitution could not be launched (grid " + std::to_string(sv.grids.back) + " for " + std::to_string(sv.plan.N) + " vertices)"); return CS_ERR_HIP; }
  if (rs) return rs;
  BA_MARK(B, B->ev[4]);
  cs::ba_launch_backsub(B->view, B->st);
  CS_HIP_TRY(hipGetLastError());
  CS_TRY(share_cuboid_increments(B, coll));
  BA_MARK(B, B->ev[5]);
  CS_TRY(B->solver.queue_status(B->h_status.p + 2, B->st));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  const cs::SparseVerdict verdict = cs::sparse_verdict(B->h_status.p + 2);     // (the factorisation's word and the dense tail's pivot)
  if (verdict == cs::SPARSE_TIMEOUT) {
    cs_set_error("sparse solver: grid not co-resident (wait timed out); set CS_BA_SPARSE=0 on a shared device");
    return CS_ERR_HIP;
  }
  if (verdict != cs::SPARSE_OK || B->h_status.p[1] != 0) *ok = false;
  return CS_OK;
}

// dense: the lower triangle of the row-major S is the upper triangle of the column-major matrix rocSOLVER sees
int solve_dense(cs_ba* B, Collectives& coll, bool* ok) {
  const int n = B->n_red;
  CS_ROC_TRY(rocsolver_dpotrf(B->blas, rocblas_fill_upper, n, B->S.p, n, B->d_info.p));
  CS_HIP_TRY(hipMemcpyAsync(B->h_status.p, B->d_info.p, sizeof(int), hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  if (B->h_status.p[0] != 0 || B->h_status.p[1] != 0) *ok = false;
  else CS_ROC_TRY(rocsolver_dpotrs(B->blas, rocblas_fill_upper, n, 1, B->S.p, n, B->view.rhs, n));
  BA_MARK(B, B->ev[4]);
  // (sharded: the collective is issued whether or not THIS rank's factorisation went through -- the ranks decide together, in the loop)
  if (*ok || B->shard_n > 1) { cs::ba_launch_backsub(B->view, B->st); CS_HIP_TRY(hipGetLastError()); CS_TRY(share_cuboid_increments(B, coll)); }
  BA_MARK(B, B->ev[5]);
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  return CS_OK;
}

int solve_device_sep(cs_ba* B, Collectives& coll, double lambda, bool* ok, std::unique_lock<std::mutex>* turn_out);

// setLambda + solve + restoreDiagonal (block_solver.hpp:353-486, :563-604): lambda is applied while the reduced system is assembled, so the
// stored blocks are never modified and nothing needs restoring.  turn_out: see solve_banded.
int solve_device(cs_ba* B, Collectives& coll, double lambda, bool* ok, std::unique_lock<std::mutex>* turn_out = nullptr) {
  *ok = true;
  const cs::TrialFacts facts = trial_facts(B, coll.fn);
  if (cs::trial_plan(facts).sharded_sep) return solve_device_sep(B, coll, lambda, ok, turn_out);
  if (B->n_red > 0) {
    const cs::SolveHead head = cs::solve_head(facts, /*deferred=*/turn_out != nullptr);
    CS_TRY(queue_reduce(B, coll, head, lambda));
    if (B->band_ld) {
      CS_TRY(solve_banded(B, coll, head, ok, turn_out));
      if (turn_out) { B->tm.n_solves++; return CS_OK; }      // (queued only: the caller waits, then reads the status words and the phase marks)
    } else if (B->sparse) {
      CS_TRY(solve_sparse(B, coll, ok));
    } else {
      CS_TRY(solve_dense(B, coll, ok));
    }
    CS_TRY(collect_solve_times(B, false));
  }
  B->tm.n_solves++;
  return CS_OK;
}

// The damped solve in separator mode (cs_ba::sep_mode; kernels: "sharded reduced solve" in band_kernels.hip).  What is built here lies
// in this rank's columns and in the next separator's diagonal block; only the interior is factorised here.  Collectives per solve:
// one all-gather of the separator messages (3 w^2 + 2 w doubles per rank) and one all-reduce of the solution vector (n_pose doubles:
// every rank contributes its interior's increments and those of the cuboids it eliminated).  block_solver.hpp:385-485 for what a
// shard builds and solves.
int solve_device_sep(cs_ba* B, Collectives& coll, double lambda, bool* ok, std::unique_lock<std::mutex>* turn_out) {
  *ok = true;
  const bool through_callback = coll.kind == cs::CollKind::callback;
  // Without a collective the separator system would be assembled from the other ranks' stale / zero messages and "solve" to a
  // meaningless x that reports positive_definite = 1 (the low-level path cs_ba_solve -> solve_device has neither callback nor, possibly,
  // a communicator).  A sharded handle solves only through cs_ba_optimize_sharded or after cs_ba_comm_init.
  if (!coll.active()) { cs_set_error("sharded handle in separator mode: the damped solve needs the ranks' separator messages -- use cs_ba_optimize_sharded (callback) or cs_ba_comm_init (RCCL); cs_ba_solve alone cannot"); return CS_ERR_INVALID_ARG; }
  const int R = B->shard_n, LD = B->band_ld, ns = B->n_sep;
  double* rhs = B->view.rhs;
  const int LDs = 2 * B->w_max;
  double* rsep = B->sepS.p + (size_t)ns * LDs;
  CS_TRY(put_lambda(B, lambda));
  BA_MARK(B, B->ev[2]);
  CS_HIP_TRY(hipMemsetAsync(B->S.p, 0, sizeof(double) * (B->s_doubles + B->n_pose), B->st));
  CS_HIP_TRY(hipMemsetAsync(B->d_elim_fail.p, 0, sizeof(int), B->st));
  if (through_callback) CS_HIP_TRY(hipMemsetAsync(B->sep_msgs.p, 0, sizeof(double) * B->msg_doubles * (size_t)R, B->st));
  cs::ba_launch_reduce(B->view, B->d_lam.p, B->st, B->st2, B->ev_fork, B->ev_join);
  CS_HIP_TRY(hipMemcpyAsync(B->h_status.p + 1, B->d_elim_fail.p, sizeof(int), hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipGetLastError());
  BA_MARK(B, B->ev[3]);
  std::unique_lock<std::mutex> coop_turn(g_coop_mutex);
  CS_HIP_TRY(hipMemsetAsync(B->d_int_info.p, 0, cs::BAND_INFO_WORDS * sizeof(int), B->st));
  // the interior: L L^T = S(I, I), y = L^-1 b_I in place (one-sided order, right-hand side riding along)
  cs::ba_launch_band_cholesky(B->S.p + (size_t)B->int_c * LD, B->int_work.p, B->int_n, LD, rhs + B->int_c, B->d_int_info.p, false, B->st, true);
  CS_HIP_TRY(hipGetLastError());
  BA_MARK(B, B->sev[0]);
  if (through_callback) {   // the callback waits for the other ranks (threads of this process in the tests): the persistent kernel's turn must be free by then
    CS_HIP_TRY(hipStreamSynchronize(B->st));
    coop_turn.unlock();
  }
  cs::ba_launch_sep_reduce(B->S.p, LD, B->int_work.p, B->int_c, B->int_n, B->zl, B->wl, B->zr, B->wr, B->sepY.p, rhs, B->sep_msgs.p + (size_t)B->shard_rank * B->msg_doubles, B->w_max, B->st);
  CS_HIP_TRY(hipGetLastError());
  BA_MARK(B, B->sev[1]);
  CS_TRY(coll.device_allgather(B->sep_msgs.p, B->msg_doubles));
  BA_MARK(B, B->sev[2]);
  // every rank assembles and solves the (small) separator system: nothing to broadcast afterwards.  Block tridiagonal = a band of
  // 2 w_max: the persistent banded Cholesky again (two fronts at 7 separators: 18 dependent steps)
  if (cs::ba_bcr_sep_ok(B->w_max, R)) {
    // ... by block cyclic reduction, straight from the messages' blocks (bcr_kernels.hip): 7 separators = 3 levels instead of 18 dependent steps
    CS_HIP_TRY(hipMemsetAsync(B->d_sep_info.p, 0, cs::BAND_INFO_WORDS * sizeof(int), B->st));
    cs::ba_launch_bcr_sep(B->sep_msgs.p, B->msg_doubles, B->w_max, R, B->d_sep_off.p, B->d_sep_col.p, ns, B->sep_work.p, rhs, B->d_sep_info.p, B->st);
    CS_HIP_TRY(hipGetLastError());
  } else {
    cs::ba_launch_sep_assemble(B->sep_msgs.p, B->msg_doubles, B->w_max, R, B->d_sep_off.p, ns, LDs, B->sepS.p, rsep, B->st);
    CS_HIP_TRY(hipGetLastError());
    if (!coop_turn.owns_lock()) coop_turn.lock();
    CS_HIP_TRY(hipMemsetAsync(B->d_sep_info.p, 0, cs::BAND_INFO_WORDS * sizeof(int), B->st));
    cs::ba_launch_band_cholesky(B->sepS.p, B->sep_work.p, ns, LDs, rsep, B->d_sep_info.p, true, B->st);
    CS_HIP_TRY(hipGetLastError());
    if (through_callback) {
      CS_HIP_TRY(hipStreamSynchronize(B->st));
      coop_turn.unlock();
    }
    cs::ba_launch_sep_scatter(rsep, ns, R, B->d_sep_off.p, B->d_sep_col.p, rhs, B->st);
  }
  BA_MARK(B, B->sev[3]);
  cs::ba_launch_sep_backsolve(B->S.p, LD, B->int_work.p, B->int_c, B->int_n, B->zl, B->wl, B->zr, B->wr, B->sepY.p, rhs, B->d_int_info.p, B->st);
  CS_HIP_TRY(hipGetLastError());
  BA_MARK(B, B->ev[4]);
  cs::ba_launch_backsub(B->view, B->st);   // this rank's landmarks and cuboids see its own columns and the next separator only
  CS_HIP_TRY(hipGetLastError());
  // the solution vector: every rank contributes ITS columns (its separator as it solved it, its interior) and its cuboids' increments
  // behind the reduced system, zeros elsewhere -- every entry then has one source, so all ranks end with the same bits
  if (B->zl > 0) CS_HIP_TRY(hipMemsetAsync(rhs, 0, sizeof(double) * (size_t)B->zl, B->st));
  if (B->int_c + B->int_n < B->n_red) CS_HIP_TRY(hipMemsetAsync(rhs + B->int_c + B->int_n, 0, sizeof(double) * (size_t)(B->n_red - B->int_c - B->int_n), B->st));
  CS_TRY(coll.device_allreduce(rhs, (size_t)B->n_pose));
  BA_MARK(B, B->ev[5]);
  cs::ba_launch_fail_flag(B->d_int_info.p, B->d_elim_fail.p, B->d_sep_info.p, B->d_scalars.p + 2, B->st);
  // both persistent factorisations of the trial report their own time-out (a team that was not co-resident): the interior's and the
  // separator system's -- the latter must not be mistaken for "not positive definite" (LM would raise lambda and retry, ~1 s a trial)
  CS_HIP_TRY(hipMemcpyAsync(B->h_status.p, B->d_int_info.p, sizeof(int), hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipMemcpyAsync(B->h_status.p + 2, B->d_sep_info.p, sizeof(int), hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipGetLastError());
  B->tm.n_solves++;
  if (turn_out) { if (coop_turn.owns_lock()) *turn_out = std::move(coop_turn); return CS_OK; }
  CS_HIP_TRY(hipMemcpyAsync(B->h_scalars.p + 2, B->d_scalars.p + 2, sizeof(double), hipMemcpyDeviceToHost, B->st));
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  if (coop_turn.owns_lock()) coop_turn.unlock();
  CS_TRY(check_band_timeout(B, true));
  if (B->h_scalars.p[2] != 0.0) *ok = false;
  return collect_solve_times(B, true);
}

// The estimates into / out of the backup buffers, queued on the handle's stream: what cs_ba_push / cs_ba_pop do once their guards have passed, and
// what cs_ba_optimize's own trials use (its rollback of a rejected trial is not the caller's pop and goes through no guard).
static int save_estimates(cs_ba* B) {
  if (B->nc) CS_HIP_TRY(hipMemcpyAsync(B->cams_bak.p, B->cams.p, 56 * (size_t)B->nc, hipMemcpyDeviceToDevice, B->st));
  if (B->np) CS_HIP_TRY(hipMemcpyAsync(B->points_bak.p, B->points.p, 24 * (size_t)B->np, hipMemcpyDeviceToDevice, B->st));
  if (B->no) CS_HIP_TRY(hipMemcpyAsync(B->cubes_bak.p, B->cubes.p, 80 * (size_t)B->no, hipMemcpyDeviceToDevice, B->st));
  return CS_OK;
}
static int restore_estimates(cs_ba* B) {
  if (B->nc) CS_HIP_TRY(hipMemcpyAsync(B->cams.p, B->cams_bak.p, 56 * (size_t)B->nc, hipMemcpyDeviceToDevice, B->st));
  if (B->np) CS_HIP_TRY(hipMemcpyAsync(B->points.p, B->points_bak.p, 24 * (size_t)B->np, hipMemcpyDeviceToDevice, B->st));
  if (B->no) CS_HIP_TRY(hipMemcpyAsync(B->cubes.p, B->cubes_bak.p, 80 * (size_t)B->no, hipMemcpyDeviceToDevice, B->st));
  return CS_OK;
}

}  // namespace

// The guard of every call that reads the linear system (see cs_ba::have_system).
int need_system(cs_ba* B, const char* who) {
  if (!B->structure_dirty && B->have_system) return CS_OK;
  cs_set_error(std::string(who) + ": no linear system on the handle (none was built, or the graph, the estimates or the external terms changed, or cs_ba_optimize ran "
               "since): call cs_ba_compute_errors + cs_ba_build_system first");
  return CS_ERR_NOT_RUN;
}

// lambda of the damped solve that is about to be queued: into the pinned word and, queued on the stream, into device memory.
int put_lambda(cs_ba* B, double lambda) {
  B->h_lam.p[0] = lambda;
  B->h_lam.p[1] = B->shard_rank == 0 ? lambda : 0.0;      // x^T (lambda x + b): the poses' lambda x^2 is counted once, on rank 0
  CS_HIP_TRY(hipMemcpyAsync(B->d_lam.p, B->h_lam.p, 2 * sizeof(double), hipMemcpyHostToDevice, B->st));
  return CS_OK;
}

extern "C" {

int cs_ba_compute_errors(cs_ba* B, double* chi2) {
  CS_GUARD_BEGIN
  if (!B || !chi2) return CS_ERR_INVALID_ARG;
  CS_HIP_TRY(hipSetDevice(B->device));
  int rc = finalize_structure(B); if (rc) return rc;
  double t0 = now_ms();
  rc = chi2_device(B, chi2);
  if (B->ext_terms_set) *chi2 += B->ext_chi2;      // the host-evaluated edges' share (cs_ba_set_external_terms / _chi2)
  B->tm.errors_ms += now_ms() - t0;
  return rc;
  CS_GUARD_END("cs_ba_compute_errors")
}

int cs_ba_build_system(cs_ba* B) {
  CS_GUARD_BEGIN
  if (!B) return CS_ERR_INVALID_ARG;
  CS_HIP_TRY(hipSetDevice(B->device));
  int rc = finalize_structure(B); if (rc) return rc;
  rc = build_system_device(B); if (rc) return rc;
  rc = fetch_b(B); if (rc) return rc;
  debug_nan_scan(B, "after cs_ba_build_system");
  return CS_OK;
  CS_GUARD_END("cs_ba_build_system")
}

int cs_ba_solve(cs_ba* B, double lambda, int* pd) {
  CS_GUARD_BEGIN
  if (!B) return CS_ERR_INVALID_ARG;
  CS_HIP_TRY(hipSetDevice(B->device));
  if (int rn = need_system(B, "cs_ba_solve")) return rn;
  bool ok = false;
  Collectives own(B, nullptr, nullptr);      // (no callback here: the handle's communicator, if it has one)
  int rc = solve_device(B, own, lambda, &ok); if (rc) return rc;
  if (ok) debug_nan_scan(B, "after cs_ba_solve");
  if (pd) *pd = ok ? 1 : 0;
  return ok ? fetch_x(B) : CS_OK;
  CS_GUARD_END("cs_ba_solve")
}

int cs_ba_update(cs_ba* B) {
  if (!B) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  if (int rn = need_system(B, "cs_ba_update (no solution to apply; cs_ba_solve comes after them)")) return rn;
  CS_HIP_TRY(hipSetDevice(B->device));
  double t0 = now_ms();
  cs::ba_launch_update(B->view, B->st);
  CS_HIP_TRY(hipGetLastError());
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  B->tm.update_ms += now_ms() - t0;
  debug_nan_scan(B, "after cs_ba_update");
  return CS_OK;
  CS_GUARD_END("cs_ba_update")
}

int cs_ba_push(cs_ba* B) {
  if (!B) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  CS_HIP_TRY(hipSetDevice(B->device));
  int rc = finalize_structure(B); if (rc) return rc;
  rc = save_estimates(B); if (rc) return rc;
  B->backup_live = true;
  return CS_OK;
  CS_GUARD_END("cs_ba_push")
}

int cs_ba_pop(cs_ba* B) {
  if (!B) return CS_ERR_INVALID_ARG;
  CS_GUARD_BEGIN
  if (B->structure_dirty || !B->backup_live) {
    cs_set_error("cs_ba_pop: no backup to restore (cs_ba_push has not run since the graph changed, since cs_ba_set_estimates, since a cs_ba_optimize call or since the last cs_ba_pop)");
    return CS_ERR_NOT_RUN;
  }
  CS_HIP_TRY(hipSetDevice(B->device));
  int rc = restore_estimates(B); if (rc) return rc;
  B->backup_live = false;        // (one level, and spent once restored)
  return CS_OK;
  CS_GUARD_END("cs_ba_pop")
}

}  // extern "C"

// ---- cs_ba_optimize: optimization_algorithm_levenberg.cpp:61-163 + sparse_optimizer.cpp:354-419.  The LM arithmetic is cs_lm.h's; which flow a
// trial takes is ba_trial_plan.h's; what follows is what each step queues and waits for.
namespace {

// One cs_ba_optimize call.
struct LmRun {
  cs_ba* B;
  cs::TrialPlan plan;
  Collectives coll;        // as the call received them (the synchronising flow's solves and every host scalar)
  Collectives queued;      // what the stream flow's solve sees: never the call's callback (kept as found)
  cs::LmState lm;          // lambda, ni, the bad-iteration count: the policy is cs_lm.h's (set by the first iteration)
  double* chi_hist; double* lambda_hist; int* trials_hist; int cap;
};
struct Trial { bool solved = true; double chi = 0, scale = 0; };      // a factorisation went through everywhere; chi2 of the new state; LM's scale term
struct FuseLinGuard { cs_ba* b; ~FuseLinGuard() { b->view.fuse_lin = 0; } };   // (every other entry point linearises with the classic kernels)
// Once an iteration has started, whatever way the call returns: no linear system for the stepwise and inspection calls (see cs_ba::have_system), and
// the caller's pushed estimates are gone (the trials save theirs in the same buffers).  Two host flags: nothing is queued for them.
struct LeftoverGuard { cs_ba* b; bool ran; ~LeftoverGuard() { if (ran) { b->have_system = false; b->backup_live = false; } } };

// every rank decides the solver layout from its own structure phase (and device query): the collectives only match if they all decided alike
int check_ranks_agree(LmRun& R) {
  const cs_ba* B = R.B;
  const double q[5] = {(double)B->n_red, (double)B->band_ld, B->elim ? 1.0 : 0.0, B->sep_mode ? 1.0 : 0.0, (double)B->n_sep};
  double v[10];
  for (int i = 0; i < 5; i++) { v[i] = q[i]; v[5 + i] = -q[i]; }
  CS_TRY(R.coll.host_reduce(v, 10, 1));
  for (int i = 0; i < 5; i++)
    if (v[i] != q[i] || v[5 + i] != -q[i]) { cs_set_error("sharded BA: the ranks disagree on the solver layout (reduced size / bandwidth / cuboid elimination / separator mode); check CS_BA_* environment variables and devices"); return CS_ERR_INVALID_ARG; }
  return CS_OK;
}

// external (host-evaluated) edges: their terms depend on the state, so the caller's callback re-evaluates them before every
// linearisation (want_system = 1: cs_ba_set_external_terms) and after every trial's update (want_system = 0: cs_ba_set_external_chi2)
int ext_refresh(LmRun& R, int want_system) {
  cs_ba* B = R.B;
  if (!R.plan.ext_active) return CS_OK;
  CS_HIP_TRY(hipStreamSynchronize(B->st));
  if (B->ext_fn(B->ext_ctx, B, want_system) != 0) { cs_set_error("external-edge callback failed"); return CS_ERR_INVALID_ARG; }
  if (!B->ext_terms_set) { cs_set_error("external-edge callback did not call cs_ba_set_external_terms"); return CS_ERR_NOT_RUN; }
  return CS_OK;
}

// computeLambdaInit (:166-180): tau * max |H_jj| over all non-fixed vertices, landmarks included
int lambda_init(LmRun& R) {
  cs_ba* B = R.B;
  if (B->shard_n == 1) {
    // one rank: the maximum is taken where the blocks are (ba_max_diag_kernel) and eight bytes come back, instead of every H_cc / H_oo / H_ll
    // block (14 MB at C4, 0.6 ms of every cs_ba_optimize call)
    CS_HIP_TRY(hipMemsetAsync(B->d_scalars.p, 0, sizeof(double), B->st));
    cs::ba_launch_max_diag(B->view, B->d_scalars.p, B->st);
    CS_HIP_TRY(hipGetLastError());
    CS_HIP_TRY(hipMemcpyAsync(B->h_scalars.p, B->d_scalars.p, sizeof(double), hipMemcpyDeviceToHost, B->st));
    CS_HIP_TRY(hipStreamSynchronize(B->st));
    cs::lm_begin(R.lm, B->user_lambda_init, B->h_scalars.p[0]);
    return CS_OK;
  }
  CS_HIP_TRY(hipStreamSynchronize(B->st));   // the copies below run on the NULL stream, which B->st does not order with
  std::vector<double> hc(36 * (size_t)B->nc), ho(81 * (size_t)B->no), hl(9 * (size_t)B->np);
  if (B->nc) CS_HIP_TRY(hipMemcpy(hc.data(), B->Hcam.p, 8 * hc.size(), hipMemcpyDeviceToHost));
  if (B->no) CS_HIP_TRY(hipMemcpy(ho.data(), B->Hcub.p, 8 * ho.size(), hipMemcpyDeviceToHost));
  if (B->np) CS_HIP_TRY(hipMemcpy(hl.data(), B->Hll.p, 8 * hl.size(), hipMemcpyDeviceToHost));
  // pose diagonals are partial sums on every rank: sum them before taking the maximum
  std::vector<double> pd(std::max(1, B->n_pose), 0.0);
  for (int i = 0; i < B->nc; i++) if (B->cam_col[i] >= 0) for (int d = 0; d < 6; d++) pd[B->cam_col[i] + d] = hc[36 * (size_t)i + 7 * d];
  for (int i = 0; i < B->no; i++) if (B->cub_col[i] >= 0) for (int d = 0; d < 9; d++) pd[B->cub_col[i] + d] = ho[81 * (size_t)i + 10 * d];
  CS_TRY(R.coll.host_reduce(pd.data(), pd.size(), 0));
  double md = 0;
  for (int i = 0; i < B->n_pose; i++) md = std::max(std::fabs(pd[i]), md);
  for (int i = 0; i < B->np; i++) if (B->pt_lm[i] >= 0) for (int d = 0; d < 3; d++) md = std::max(std::fabs(hl[9 * (size_t)i + 4 * d]), md);
  CS_TRY(R.coll.host_reduce(&md, 1, 1));
  cs::lm_begin(R.lm, B->user_lambda_init, md);
  return CS_OK;
}

// One trial, queued: damped solve, scale term + update, chi2 of the new state, [chi2, scale term, "a factorisation failed somewhere"] summed into
// one message (and over the ranks: ONE RCCL all-reduce; every rank takes the same accept / reject branch).
// x^T (lambda x + b): b is a per-rank partial sum, x is replicated for the poses -- their lambda x^2 term is counted once (rank 0); a landmark's
// terms live on exactly one rank.  A failed factorisation leaves garbage in x; the update then writes garbage estimates, which the pop restores
// (the decision is taken after the synchronisation).  spec: the next linearisation will be queued behind this trial's update.
// (The sequence is the same ~30 launches, fills and copies for every trial of a structure -- lambda is read from device memory -- and was
// replayed as one hipGraph in round 4: measured no faster on MI355X / ROCm 7.0 and +0.8 ms of instantiation per structure, DESIGN.md section 3;
// removed in round 5.)
int queue_trial(LmRun& R, bool spec, std::unique_lock<std::mutex>* turn) {
  cs_ba* B = R.B;
  const bool direct = R.plan.direct_scalars;
  bool okq = true;
  CS_TRY(solve_device(B, R.queued, R.lm.lambda, &okq, turn));
  cs::ba_launch_scale_update(B->view, B->d_lam.p, B->scale_partial.p, B->st, B->cams_bak.p, B->points_bak.p, B->cubes_bak.p);
  if (spec) CS_HIP_TRY(hipEventRecord(B->ev_upd, B->st));      // the state the next linearisation reads is final from here
  BA_MARK(B, B->ev[6]);
  cs::ba_launch_chi2(B->view, B->nb_chi, B->st);
  if (R.plan.sharded_sep) cs::ba_launch_sum2(B->chi_partial.p, B->n_chi_partials, B->scale_partial.p, cs::ba_scale_blocks(), B->d_scalars.p, B->st);   // (separator mode set its flag itself: three status words)
  else cs::ba_launch_sum2_flag(B->chi_partial.p, B->n_chi_partials, B->scale_partial.p, cs::ba_scale_blocks(), B->d_band_info.p, B->d_elim_fail.p, B->d_scalars.p, B->st,
                               direct ? B->h_trial.p : nullptr, direct ? (B->trial_seq += 1.0) : 0.0);
  CS_HIP_TRY(hipGetLastError());
  if (R.plan.coll == cs::CollKind::rccl) BA_NCCL(ncclAllReduce(B->d_scalars.p, B->d_scalars.p, 3, ncclDouble, ncclSum, B->comm, B->st));
  if (!direct) CS_HIP_TRY(hipMemcpyAsync(B->h_scalars.p, B->d_scalars.p, 3 * sizeof(double), hipMemcpyDeviceToHost, B->st));
  BA_MARK(B, B->ev[7]);
  return CS_OK;
}

// the trial's scalars in pinned memory, written by its last kernel: polled, no runtime call
int await_trial(cs_ba* B, double seq) {
  volatile double* h = B->h_trial.p;
  const double t_w = now_ms();
  unsigned spins = 0;
  while (h[3] != seq) {
    if ((++spins & 0xfffu) == 0 && now_ms() - t_w > 5000.0) {      // five seconds without the word: ask the runtime what happened
      CS_HIP_TRY(hipStreamSynchronize(B->st));
      if (h[3] != seq) { cs_set_error("cs_ba_optimize: the trial's scalars never arrived in pinned memory"); return CS_ERR_HIP; }
      break;
    }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
  std::atomic_thread_fence(std::memory_order_acquire);
  return CS_OK;
}

// Stream flow: everything queued, one wait.  spec: the next iteration's linearisation (never iteration 0's: the fused form where the graph allows
// it) goes behind the trial, before the verdict.
int trial_on_stream(LmRun& R, bool spec, Trial& t) {
  cs_ba* B = R.B;
  std::unique_lock<std::mutex> turn;
  CS_TRY(queue_trial(R, spec, &turn));
  if (spec) {
    const int fl = B->view.fuse_lin;
    B->view.fuse_lin = R.plan.fuse_lin_ok ? 1 : 0;
    const int rc = build_system_device(B, B->ev_upd);      // (its numeric-Jacobian edges start behind the update, beside this trial's chi2 kernels)
    B->view.fuse_lin = fl;       // (a retry of THIS iteration reduces the way this iteration linearised)
    if (rc) return rc;
  }
  const double* hs = B->h_scalars.p;
  if (R.plan.direct_scalars) { CS_TRY(await_trial(B, B->trial_seq)); hs = B->h_trial.p; }
  else CS_HIP_TRY(hipStreamSynchronize(B->st));
  turn.unlock();
  CS_TRY(check_band_timeout(B, R.plan.sharded_sep));
  t.solved = hs[2] == 0.0;
  t.chi = hs[0];
  t.scale = hs[1];
  if (B->stage_timing) {
    if (R.plan.direct_scalars) CS_HIP_TRY(hipStreamSynchronize(B->st));     // (the phase marks are read below: the last one must have passed)
    CS_TRY(collect_solve_times(B, R.plan.sharded_sep));
    float ms = 0;
    CS_HIP_TRY(hipEventElapsedTime(&ms, B->ev[6], B->ev[7])); B->tm.errors_ms += ms;
  }
  if (R.plan.ext_active && t.solved) { CS_TRY(ext_refresh(R, 0)); t.chi += B->ext_chi2; }
  return CS_OK;
}

// Synchronising flow (dense and sparse solves, callback ranks): the solve waits inside, the host sums the scalars over the ranks.
int trial_synchronising(LmRun& R, Trial& t) {
  cs_ba* B = R.B;
  CS_TRY(solve_device(B, R.coll, R.lm.lambda, &t.solved));
  if (B->shard_n > 1) {   // a failed factorisation on one rank is everybody's rejected trial
    double ff = t.solved ? 0.0 : 1.0;
    CS_TRY(R.coll.host_reduce(&ff, 1, 1));
    t.solved = ff == 0.0;
  }
  if (t.solved) {
    const int nsb = cs::ba_scale_blocks();
    std::vector<double> sp(nsb);
    cs::ba_launch_scale(B->view, B->d_lam.p, B->scale_partial.p, B->st);     // (d_lam still holds this trial's lambda: put_lambda in the solve)
    CS_HIP_TRY(hipGetLastError());
    CS_HIP_TRY(hipMemcpyAsync(sp.data(), B->scale_partial.p, sizeof(double) * nsb, hipMemcpyDeviceToHost, B->st));
    CS_TRY(cs_ba_update(B));   // synchronises the stream
    for (double p : sp) t.scale += p;
  }
  const double t0 = now_ms();
  CS_TRY(chi2_device(B, &t.chi));
  if (R.plan.ext_active && t.solved) { CS_TRY(ext_refresh(R, 0)); t.chi += B->ext_chi2; }
  CS_TRY(R.coll.host_reduce(&t.chi, 1, 0));
  B->tm.errors_ms += now_ms() - t0;
  CS_TRY(R.coll.host_reduce(&t.scale, 1, 0));
  return CS_OK;
}

int lm_loop(LmRun& R, int iterations, LeftoverGuard& leftover, int* done_out) {
  cs_ba* B = R.B;
  const cs::TrialPlan& plan = R.plan;
  bool spec_lin = false;         // this iteration's system is already queued (speculated behind the last iteration's accepted trial)
  int done = 0;
  double currentChi = 0;
  bool have_chi = false;         // chi2 of the current state is known from the previous iteration's last trial
  for (int it = 0; it < iterations; it++) {
    leftover.ran = true;
    const double t0 = now_ms();
    CS_TRY(ext_refresh(R, 1));        // (the terms of this iteration's linearisation, and the chi2 share at the current state)
    // computeActiveErrors + activeRobustChi2 at the top of an iteration (:67-69) would re-evaluate the state the last trial left: the accepted
    // trial's chi2 (same kernels, same state, fixed-shape sums: the same bits), or -- after ten rejections -- the popped state's, which is the
    // previous currentChi.  Only the first iteration computes it.
    if (!have_chi) {
      CS_TRY(chi2_device(B, &currentChi));
      if (plan.ext_active) currentChi += B->ext_chi2;
      CS_TRY(R.coll.host_reduce(&currentChi, 1, 0));
      B->tm.errors_ms += now_ms() - t0;
    }
    const double iniChi = currentChi;
    // the first iteration needs H_ll for lambda's initial value before any trial: the fused linearisation from the second on
    B->view.fuse_lin = (it > 0 && plan.fuse_lin_ok) ? 1 : 0;
    if (!spec_lin) CS_TRY(build_system_device(B));
    spec_lin = false;
    debug_nan_scan(B, "cs_ba_optimize: after the linearisation");
    if (it == 0) CS_TRY(lambda_init(R));
    const bool spec = cs::spec_now(plan, it, iterations);
    double rho = 0;
    int qmax = 0;
    do {
      Trial t;
      if (plan.stream_flow) CS_TRY(trial_on_stream(R, spec, t));      // (its update kernel saves the estimates it replaces)
      else { CS_TRY(save_estimates(B)); CS_TRY(trial_synchronising(R, t)); }
      if (t.solved) debug_nan_scan(B, "cs_ba_optimize: after a trial's solve + update");
      if (cs::lm_trial(R.lm, currentChi, t.chi, t.scale, t.solved, rho)) {
        spec_lin = spec;           // the system of the state this trial left is already on the stream
      } else {
        CS_TRY(restore_estimates(B));
        if (spec) CS_TRY(build_system_device(B));      // the speculation linearised the rejected state: the restored one again, as this iteration linearises
      }
      qmax++;
    } while (cs::lm_again(rho, qmax, B->max_trials_after_failure));
    if (!spec_lin) CS_HIP_TRY(hipStreamSynchronize(B->st));
    if (done < R.cap) {
      if (R.chi_hist) R.chi_hist[done] = currentChi;
      if (R.lambda_hist) R.lambda_hist[done] = R.lm.lambda;
      if (R.trials_hist) R.trials_hist[done] = qmax;
    }
    done++;
    have_chi = true;
    if (cs::lm_stop(R.lm, rho, qmax, B->max_trials_after_failure, iniChi, currentChi)) break;
  }
  if (spec_lin) CS_HIP_TRY(hipStreamSynchronize(B->st));      // (a stopping rule ended the loop behind an accepted trial: its speculated system is the current state's)
  *done_out = done;
  return CS_OK;
}

}  // namespace

int cs_ba_optimize_sharded_impl(cs_ba* B, int iterations, cs_allreduce_fn fn, void* ctx, int* iterations_done, double* chi_hist, double* lambda_hist, int* trials_hist, int cap) {
  if (!B || iterations < 0) return CS_ERR_INVALID_ARG;
  if (B->shard_n > 1 && !fn && !B->comm) { cs_set_error("sharded problem needs cs_ba_comm_init() (RCCL) or an all-reduce callback"); return CS_ERR_INVALID_ARG; }
  CS_HIP_TRY(hipSetDevice(B->device));
  CS_TRY(finalize_structure(B));
  LmRun R{B, cs::trial_plan(trial_facts(B, fn)), Collectives(B, fn, ctx), Collectives(B, nullptr, nullptr), cs::LmState{}, chi_hist, lambda_hist, trials_hist, cap};
  const double t_begin = now_ms();
  if (B->shard_n > 1) CS_TRY(check_ranks_agree(R));
  if (R.plan.ext_active && !B->ext_fn) { cs_set_error("cs_ba_optimize: the graph has external (host-evaluated) edges but no cs_ba_set_external_callback; drive the stepwise calls instead"); return CS_ERR_NOT_RUN; }
  FuseLinGuard fuse_lin_guard{B};
  LeftoverGuard leftover_guard{B, false};
  int done = 0;
  CS_TRY(lm_loop(R, iterations, leftover_guard, &done));
  if (iterations_done) *iterations_done = done;
  B->tm.total_ms += now_ms() - t_begin;
  return CS_OK;
}

extern "C" {

int cs_ba_optimize(cs_ba* B, int iterations, int* iterations_done, double* chi_hist, double* lambda_hist, int* trials_hist, int cap) {
  return cs_ba_optimize_sharded(B, iterations, nullptr, nullptr, iterations_done, chi_hist, lambda_hist, trials_hist, cap);
}
int cs_ba_optimize_sharded(cs_ba* B, int iterations, cs_allreduce_fn fn, void* ctx, int* iterations_done, double* chi_hist, double* lambda_hist, int* trials_hist, int cap) {
  CS_GUARD_BEGIN
  return cs_ba_optimize_sharded_impl(B, iterations, fn, ctx, iterations_done, chi_hist, lambda_hist, trials_hist, cap);
  CS_GUARD_END("cs_ba_optimize_sharded")
}

}  // extern "C"
