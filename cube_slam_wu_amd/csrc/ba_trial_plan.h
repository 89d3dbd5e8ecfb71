// ba_trial_plan.h -- which flow one LM trial of the bundle adjustment takes, stated once.  Plain C++, no HIP include: ba_lm.cpp reads the
// facts off the handle in one place (trial_facts), everything below is a pure function of them, and tools/hostonly/ba_trial_plan_check.cpp
// enumerates every combination against the expressions this header replaced and against the implications the comments below claim.
//
// Two pairs of switches look like one fact each and are not.  Both are kept exactly as they behaved before this header existed:
//   * fuse_lin_ok asks whether CS_BA_DEBUG_NAN is PRESENT in the environment (nan_env_present), can_spec whether its VALUE is non-zero
//     (nan_scans_on: atoi, read once per process).  CS_BA_DEBUG_NAN=0 therefore keeps the classic linearisation kernels and still speculates.
//     The first is the older, cautious form (any mention of the scans keeps the kernels whose blocks the scans can read); the second was
//     written against the scan function itself, which does nothing at 0.
//   * ext_active (the driver) is "the graph has external edges, OR terms were set, OR a callback is registered"; pro_in_reduce and the
//     external off-diagonals (the solve) ask "external edges AND terms set".  The driver must refuse or refresh whenever anything external
//     is around; the solve only cares whether a kernel is about to write S between the prologue and the reduce.
#pragma once

namespace cs {

// What the handle and the call look like.  Plain values; nothing here is derived.
struct TrialFacts {
  bool callback_given = false;    // the caller's all-reduce callback, as the function that reads these facts received it
  bool comm_present = false;      // an RCCL communicator on the handle (cs_ba_comm_init)
  int shard_n = 1, band_ld = 0, n_red = 0;
  bool sparse = false, use_bcr = false, sep_mode = false, elim = false, fused = false;
  bool has_proj = false;          // n_proj > 0
  bool seg_classes_full = false;  // every segment of the fused schedule belongs to the largest class: n_seg == max(seg_class[..])
  bool ext_edges = false;         // ext_n > 0
  bool ext_terms_set = false;
  bool ext_fn_set = false;
  bool stage_timing = false;
  bool h_trial_present = false;   // the pinned, device-visible words a trial's last kernel writes
  bool fuse_lin_env = true;       // CS_BA_FUSE_LIN unset or non-zero (read per call)
  bool nan_env_present = false;   // getenv("CS_BA_DEBUG_NAN") != nullptr
  bool nan_scans_on = false;      // its value is non-zero (cached per process)
};

enum class CollKind { none, callback, rccl };

struct TrialPlan {
  CollKind coll = CollKind::none;
  bool sharded_sep = false, stream_flow = false, direct_scalars = false, can_spec = false, fuse_lin_ok = false, ext_active = false;
};

// Collectives of a sharded run: through the caller's callback (host-synchronous: CPU / gloo tests, ranks as threads -- it only counts on a
// handle that IS sharded), or issued by the library on the handle's stream (RCCL) when no callback came with the call.
inline CollKind coll_kind(const TrialFacts& f) {
  if (f.callback_given && f.shard_n > 1) return CollKind::callback;
  if (!f.callback_given && f.comm_present) return CollKind::rccl;
  return CollKind::none;
}

inline TrialPlan trial_plan(const TrialFacts& f) {
  TrialPlan p;
  p.coll = coll_kind(f);
  // Separator mode of the sharded solve is decided by the structure phase; a handle that was un-sharded since keeps the flag, hence both.
  p.sharded_sep = f.sep_mode && f.shard_n > 1;
  // One trial entirely on the stream (banded solver, no callback): damped solve, LM scale term, update, chi2 of the new state and --
  // sharded -- ONE RCCL all-reduce of [chi2, scale, failure flag] are queued back to back; the host waits once per trial.  Dense and sparse
  // solves synchronise inside, and a callback is host-synchronous: those take the synchronising flow.
  p.stream_flow = p.coll != CollKind::callback && f.band_ld > 0 && f.n_red > 0;
  // External (host-evaluated) edges: their terms depend on the state, so the caller's callback re-evaluates them before every linearisation
  // and after every trial's update.
  p.ext_active = f.ext_edges || f.ext_terms_set || f.ext_fn_set;
  // From the second iteration on the landmark side of the projection edges is linearised inside the trial's Schur kernels
  // (ba_lin_schur_kernel: one pass over the edges, H_pl never read back).  Same bits either way (CS_BA_FUSE_LIN=0: the classic pair of
  // kernels throughout).  Needs the fused schedule with every segment in one class, one rank, nothing host-evaluated, and no NaN scan that
  // would read H_pl.
  p.fuse_lin_ok = f.fuse_lin_env && p.stream_flow && f.fused && f.shard_n == 1 && !p.ext_active && f.has_proj && f.seg_classes_full && !f.nan_env_present;
  // The NEXT iteration's linearisation is queued right behind a trial, before the host has the trial's verdict: nearly every trial is
  // accepted, and the ~70 us the host needs to read the scalars, decide and queue again then pass while the device linearises.  A rejected
  // trial pops the estimates and linearises the restored state once more -- the same kernels on the same state: the same bits as the system
  // the speculation overwrote.  Off whenever something else must see the stream between trials: external edges, sharded runs, the NaN scans,
  // the stage split's phase marks.
  p.can_spec = p.stream_flow && f.shard_n == 1 && !p.ext_active && !f.stage_timing && !f.nan_scans_on;
  // A trial's scalars straight from its last kernel into pinned memory, polled by the host (no RCCL: no collective behind that kernel).
  p.direct_scalars = p.stream_flow && p.coll != CollKind::rccl && f.h_trial_present;
  return p;
}

// Speculate behind THIS trial: only when its scalars arrive without a stream synchronisation, and another iteration may follow.
inline bool spec_now(const TrialPlan& p, int it, int iterations) { return p.can_spec && p.direct_scalars && it + 1 < iterations; }

// The head of one damped solve outside separator mode.  deferred: called from the stream flow -- everything is queued, nothing waited for.
struct SolveHead {
  bool lean_head = false;          // banded path: one prologue kernel (lambda, status words, [S | rhs] cleared) instead of a copy and three fills
  bool pro_in_reduce = false;      // ... launched by the reduce on its side stream, beside the landmark segments: nothing reads the phase
                                   // marks, one rank, and no host-evaluated edge writes S in between
  bool status_in_scalars = false;  // block cyclic reduction in a deferred trial: no kernel of it waits for another (no time-out word), and
                                   // the two failure words reach the host folded into the trial's scalars -- two 4-byte copies stay away
  bool sum_ranks = false;          // the ranks' partial [S | rhs] are summed in one message
};
inline SolveHead solve_head(const TrialFacts& f, bool deferred) {
  SolveHead h;
  h.lean_head = f.band_ld > 0 && !f.sparse;
  h.pro_in_reduce = h.lean_head && deferred && !f.stage_timing && f.shard_n == 1 && !(f.ext_edges && f.ext_terms_set);
  h.status_in_scalars = deferred && f.band_ld > 0 && f.use_bcr;
  h.sum_ranks = coll_kind(f) != CollKind::none && !(f.sep_mode && f.shard_n > 1);
  return h;
}

}  // namespace cs
