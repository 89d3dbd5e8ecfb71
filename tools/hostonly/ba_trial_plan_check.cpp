// ba_trial_plan_check.cpp -- the switches of the bundle adjustment's trial flow (cube_slam_wu_amd/csrc/ba_trial_plan.h) on their own, without a
// GPU: every combination of the boolean facts, with shard_n in {1, 2, 3}, band_ld in {0, 33} and n_red in {0, 132} (1.6 million cases, each
// with the solve's head deferred and not), against
//   (a) the expressions as cs_ba_optimize and solve_device spelled them before the header existed, restated HERE with the names they had there
//       (never taken from the header), and
//   (b) the implications that the header's comments claim.
// One implication is known not to hold between the DRIVER's plan and the head of the solve it queues ("a callback on a
// one-rank communicator"): the program pins the exact set of combinations where it fails, so that the set can neither grow nor move unseen.
// tests/test_ba_trial_plan_cpu.py builds it with the host compiler and the sanitizers and runs it.
#include <algorithm>
#include <cstdio>

#include "../../cube_slam_wu_amd/csrc/ba_trial_plan.h"

using namespace cs;

static long g_fail = 0, g_cases = 0;
static void describe(const TrialFacts& f, bool deferred) {
  std::printf("fn %d comm %d shard_n %d band_ld %d n_red %d sparse %d bcr %d sep %d elim %d fused %d proj %d segfull %d ext_n %d ext_set %d ext_fn %d split %d h_trial %d fuse_env %d nan_env %d nan_on %d deferred %d",
              f.callback_given, f.comm_present, f.shard_n, f.band_ld, f.n_red, f.sparse, f.use_bcr, f.sep_mode, f.elim, f.fused, f.has_proj, f.seg_classes_full, f.ext_edges, f.ext_terms_set,
              f.ext_fn_set, f.stage_timing, f.h_trial_present, f.fuse_lin_env, f.nan_env_present, f.nan_scans_on, deferred);
}
#define CHECK(cond) do { if (!(cond)) { if (g_fail++ < 20) { std::printf("FAIL line %d: %s | ", __LINE__, #cond); describe(f, deferred); std::printf("\n"); } } } while (0)
#define IMPLIES(a, b) CHECK(!(a) || (b))

// (a) the driver: cs_ba_optimize_sharded_impl's locals, in its order and in its words.  `fn` is the callback pointer's truth value, `comm` the
// communicator's, h_trial the pinned words'; getenv_nan is `getenv("CS_BA_DEBUG_NAN") == nullptr` negated, debug_nan_enabled the cached atoi.
struct Driver { bool cb, rccl, stream_flow, ext_active, fuse_lin_ok, can_spec, direct_scalars, sharded_sep; };
static Driver parent_driver(const TrialFacts& f) {
  const bool fn = f.callback_given, comm = f.comm_present, h_trial = f.h_trial_present;
  const int shard_n = f.shard_n, band_ld = f.band_ld, n_red = f.n_red;
  Driver d;
  d.cb = fn && shard_n > 1;
  d.rccl = !fn && comm;
  d.stream_flow = !d.cb && band_ld > 0 && n_red > 0;
  d.ext_active = f.ext_edges || f.ext_terms_set || f.ext_fn_set;
  d.fuse_lin_ok = f.fuse_lin_env && d.stream_flow && f.fused && shard_n == 1 && !d.ext_active && f.has_proj && f.seg_classes_full && !f.nan_env_present;
  d.can_spec = d.stream_flow && shard_n == 1 && !d.ext_active && !f.stage_timing && !f.nan_scans_on;
  d.direct_scalars = d.stream_flow && !d.rccl && h_trial;
  d.sharded_sep = f.sep_mode && shard_n > 1;
  return d;
}
// (a) the solve: solve_device's locals; defer is `defer != nullptr`, fn what the function received
struct Solve { bool lean_head, pro_in_reduce, status_in_scalars, sum_ranks; };
static Solve parent_solve(const TrialFacts& f, bool defer) {
  const bool fn = f.callback_given, comm = f.comm_present;
  Solve s;
  s.lean_head = f.band_ld > 0 && !f.sparse;
  s.pro_in_reduce = s.lean_head && defer && !f.stage_timing && f.shard_n == 1 && !(f.ext_edges && f.ext_terms_set);
  s.status_in_scalars = defer && f.band_ld > 0 && f.use_bcr;
  // (the rank sum sits behind `if (sep_mode && shard_n > 1) return solve_device_sep(...)`)
  s.sum_ranks = !(f.sep_mode && f.shard_n > 1) && ((fn && f.shard_n > 1) || (!fn && comm));
  return s;
}

static void check_case(const TrialFacts& f, bool deferred) {
  g_cases++;
  const TrialPlan p = trial_plan(f);
  const SolveHead h = solve_head(f, deferred);
  const Driver d = parent_driver(f);
  const Solve s = parent_solve(f, deferred);
  // ---- (a)
  CHECK((p.coll == CollKind::callback) == d.cb);
  CHECK((p.coll == CollKind::rccl) == d.rccl);
  CHECK((p.coll == CollKind::none) == (!d.cb && !d.rccl));
  CHECK(p.sharded_sep == d.sharded_sep);
  CHECK(p.stream_flow == d.stream_flow);
  CHECK(p.ext_active == d.ext_active);
  CHECK(p.fuse_lin_ok == d.fuse_lin_ok);
  CHECK(p.can_spec == d.can_spec);
  CHECK(p.direct_scalars == d.direct_scalars);
  for (int iterations = 0; iterations < 4; iterations++)
    for (int it = 0; it < std::max(1, iterations); it++) CHECK(spec_now(p, it, iterations) == (d.can_spec && d.direct_scalars && it + 1 < iterations));
  CHECK(h.lean_head == s.lean_head);
  CHECK(h.pro_in_reduce == s.pro_in_reduce);
  CHECK(h.status_in_scalars == s.status_in_scalars);
  CHECK(h.sum_ranks == s.sum_ranks);
  // ---- (b)
  const bool spec = spec_now(p, 0, 2);
  IMPLIES(spec, p.stream_flow && f.shard_n == 1 && !f.ext_edges && !p.ext_active && !f.stage_timing && !f.nan_scans_on && p.direct_scalars);
  IMPLIES(p.direct_scalars, p.coll != CollKind::rccl);
  IMPLIES(p.fuse_lin_ok, p.stream_flow && f.shard_n == 1 && f.fused && !f.ext_edges);
  IMPLIES(h.pro_in_reduce, deferred && h.lean_head && !f.stage_timing);
  IMPLIES(h.status_in_scalars, deferred && f.use_bcr);
  CHECK(h.sum_ranks == (p.coll != CollKind::none && !p.sharded_sep));
  IMPLIES(p.stream_flow, p.coll != CollKind::callback);
  IMPLIES(f.ext_edges && f.ext_terms_set, p.ext_active);      // (of the two questions about external edges the solve's is the narrower one)
  // ---- the driver's plan against the head of the solve IT queues.  The stream flow hands the solve no callback, whatever the call received
  // (the synchronising flow passes the call's on), so the deferred solve reads its facts with callback_given = false.
  if (deferred && p.stream_flow) {
    TrialFacts q = f;
    q.callback_given = false;
    const bool solve_sums = solve_head(q, true).sum_ranks, driver_has_coll = p.coll != CollKind::none && !p.sharded_sep;
    // a callback given to an UNsharded handle that holds a (one-rank) communicator: the driver takes "no collectives" (polled scalars, no
    // all-reduce of them), the queued solve still sums [S | rhs] over the communicator's one rank.  Harmless in value (a sum over one
    // rank); recorded, not fixed.
    const bool known = f.callback_given && f.comm_present && f.shard_n == 1;
    CHECK((solve_sums != driver_has_coll) == known);
    IMPLIES(known, solve_sums && !driver_has_coll);
  }
}

int main() {
  const int shard_ns[3] = {1, 2, 3}, band_lds[2] = {0, 33}, n_reds[2] = {0, 132};
  for (unsigned m = 0; m < (1u << 17); m++) {
    TrialFacts f;
    unsigned b = m;
    auto next = [&b]() { const bool v = b & 1u; b >>= 1; return v; };
    f.callback_given = next(); f.comm_present = next(); f.sparse = next(); f.use_bcr = next(); f.sep_mode = next(); f.elim = next(); f.fused = next();
    f.has_proj = next(); f.seg_classes_full = next(); f.ext_edges = next(); f.ext_terms_set = next(); f.ext_fn_set = next(); f.stage_timing = next();
    f.h_trial_present = next(); f.fuse_lin_env = next(); f.nan_env_present = next(); f.nan_scans_on = next();
    for (int sn : shard_ns) for (int ld : band_lds) for (int nr : n_reds) {
      f.shard_n = sn; f.band_ld = ld; f.n_red = nr;
      check_case(f, false);
      check_case(f, true);
    }
  }
  std::printf("%ld cases, %ld failures\n", g_cases, g_fail);
  if (g_fail) return 1;
  std::printf("ba_trial_plan_check: ok\n");
  return 0;
}
