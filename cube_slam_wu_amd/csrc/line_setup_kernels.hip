// line_setup_kernels.hip -- the line setup of the cuboid proposal sweep for gfx950 (MI355X).
//
// Per (box, height sample): the ROI line filter (box_proposal_detail.cpp:271-283), merge_break_lines
// (object_3d_util.cpp:431-543) and the angle / midpoint tables (:309-315), one wavefront per job.
//
// merge_break_lines is sequential -- merge the lexicographically first pair (a, b), a < b, that passes three tests
// (angle difference, end-point gap, angle of the merged segment), overwrite row a, move the last row into b,
// restart -- and its result depends on that order, so the order is reproduced exactly.  Rescanning all pairs every
// round (what the reference does) costs O(m^2) pair tests per merge.  Round 5: the wave keeps the whole PAIR-TEST MATRIX as
// bits -- PM[a] = the set of partners b > a of row a -- built once (every lane owns the rows lane, lane + 64, ... and tests them
// against row b, broadcast from LDS, for b = 1 .. m-1; the two cheap tests first, the third only for their few survivors), and a
// round is: the first row with a partner (one ballot per 64 rows), its first partner (a find-first-set), the merge, and a repair
// of the matrix -- only pairs that involve the two rewritten rows can change: every row tests itself against the merged row (the
// merged row's own partner set is those tests' ballot), the row that moved into b inherits the bits of the old last row from the
// rows before it and tests the rows behind it.  No lane ever scans for a first partner again.  (Rounds 1-4 kept F[a] = the first
// partner only: every lane walked its row's partners until the first hit -- the wave as long as its unluckiest lane -- and a
// rewritten first partner meant a cooperative re-scan: 23 k wave instructions per job, now ~10 k.)
//
// Angles.  Only DECISIONS need a row's angle during the merges, so rows carry it as a float (atan2_float, 2.5e-6 rad) and the
// two angle tests are taken on floats with the exact evaluation (cs_atan2 of the row's end points -- the value the reference
// holds, whether the row is an input segment or a merge product) inside a margin; the exact angles of the rows that survive are
// computed once at the end, in parallel, where they leave the kernel.
//
// Two instances share the jobs and differ in WHERE the matrix lives; the procedure's steps -- ROI
// predicate, loader, merged row, a round's tests of one owned row, emission -- are the functions below, stated once for both.
#include <hip/hip_runtime.h>

#include "detect_types.h"
#include "cs_atan2_float.h"

namespace cs {

enum { LS_CAP = 512, LS_MID = 256, LS_SMALL = 128 };      // rows of the three instances

struct LineSetupParams {
  double dist_thre, angle_thre_rad, len_thre;  // 20 px, 5 deg, 30 px (:288-290)
  double dist_sq_bound;                        // sqrt(x) < dist_thre <=> x < dist_sq_bound   (cs_geom.h sqrt_lt_bound)
  double len_sq_bound;                         // sqrt(x) > len_thre  <=> x > len_sq_bound    (sqrt_le_bound)
};

struct LsRow { float af; double x1, y1, x2, y2; };   // af: the float angle, NaN = unusable (zero-length / non-finite): decided exactly

// a job's rows in LDS
template <int CAP>
struct LsRows {
  double X1[CAP], Y1[CAP], X2[CAP], Y2[CAP];
  float AF[CAP];
  __device__ __forceinline__ LsRow row(int i) const { return LsRow{AF[i], X1[i], Y1[i], X2[i], Y2[i]}; }
  __device__ __forceinline__ void store(int i, const LsRow& r) { X1[i] = r.x1; Y1[i] = r.y1; X2[i] = r.x2; Y2[i] = r.y2; AF[i] = r.af; }
};

__device__ __forceinline__ float ls_angf(double x1, double y1, double x2, double y2) {
  bool usable;
  const float a = atan2_float((float)(y2 - y1), (float)(x2 - x1), &usable);
  return usable ? a : __builtin_nanf("");
}
// first test of a pair, exactly as the reference evaluates it (rare: only inside the float test's margin)
__device__ __attribute__((noinline)) bool ls_rare_angle_diff(double ax1, double ay1, double ax2, double ay2, double bx1, double by1, double bx2, double by2, double thre) {
  const double diff = dabs(cs_atan2(ay2 - ay1, ax2 - ax1) - cs_atan2(by2 - by1, bx2 - bx1));
  return dmin(diff, CS_PI - diff) < thre;
}
// third test of a pair, exactly as the reference evaluates it (rare)
__device__ __attribute__((noinline)) bool ls_rare_angle_close(double ax1, double ay1, double ax2, double ay2, double dy, double dx, double thre) {
  const double t = dabs(cs_atan2(ay2 - ay1, ax2 - ax1) - cs_atan2(dy, dx));
  return dmin(t, CS_PI - t) < thre;
}
// The three tests of object_3d_util.cpp:464-497 for the ordered pair (A = the row with the lower index, B).  Only decisions leave
// these functions: float angles (each within 2.5e-6 rad of the row's exact angle, so a float difference is within 5.4e-6 of the exact
// one: margin 1.5e-5, the exact evaluation inside it), end-point gaps compared squared (sqrt_lt_bound).  Tests 1 + 2 are symmetric
// in A and B; test 3 is not (it compares the merged segment's angle with A's and breaks end-point ties towards B).
// Tests 1 + 2 come in two control-flow shapes.  FLAT = false: test 1 first, with its exact evaluation, and test 2 only behind it
// (data-dependent branches; the LDS instances, whose lanes run four or eight rows apiece).  FLAT = true: both cheap tests for every pair and the
// exact evaluation behind a wave-uniform ballot, for the pairs test 2 lets through (the register instance, written without data-dependent
// branches).  The same decision: test 2 does not depend on test 1.
#define LS_MARGIN 1.5e-5f
template <bool FLAT>
__device__ __forceinline__ bool ls_t12(const LsRow& A, const LsRow& B, const LineSetupParams& lp, float thf) {
  float df = fabsf(A.af - B.af);
  df = fminf(df, 3.14159274f - df);
  bool p1 = df < thf - LS_MARGIN;
  const bool unsure = !p1 && !(df > thf + LS_MARGIN);             // (a NaN lands here)
  if (!FLAT) {
    if (unsure) p1 = ls_rare_angle_diff(A.x1, A.y1, A.x2, A.y2, B.x1, B.y1, B.x2, B.y2, lp.angle_thre_rad);
    if (!p1) return false;
  }
  const double d_ab = v2_dist2(v2(A.x2, A.y2), v2(B.x1, B.y1));
  const double d_ba = v2_dist2(v2(B.x2, B.y2), v2(A.x1, A.y1));
  const bool p2 = (d_ab < lp.dist_sq_bound) || (d_ba < lp.dist_sq_bound);
  if (FLAT && __ballot(unsure && p2)) { if (unsure && p2) p1 = ls_rare_angle_diff(A.x1, A.y1, A.x2, A.y2, B.x1, B.y1, B.x2, B.y2, lp.angle_thre_rad); }
  return p1 && p2;
}
// test 3 of the pair {P, Q}; p_is_a: P is the row with the lower index (A).  The merged segment starts at A's start if A.x1 < B.x1,
// else at B's (a tie goes to B), ends at A's end if A.x2 > B.x2, else at B's, and its angle is compared with A's (rows hold finite
// coordinates: a NaN end point is never inside the ROI).
__device__ __forceinline__ bool ls_t3(const LsRow& P, const LsRow& Q, bool p_is_a, const LineSetupParams& lp, float thf) {
  const bool sp = p_is_a ? (P.x1 < Q.x1) : !(Q.x1 < P.x1), ep = p_is_a ? (P.x2 > Q.x2) : !(Q.x2 > P.x2);
  const double sx = sp ? P.x1 : Q.x1, sy = sp ? P.y1 : Q.y1, ex = ep ? P.x2 : Q.x2, ey = ep ? P.y2 : Q.y2;
  const double dy = ey - sy, dx = ex - sx;
  bool usable;
  const float at = atan2_float((float)dy, (float)dx, &usable);
  const float tf = fabsf((p_is_a ? P.af : Q.af) - at);
  const float mf = fminf(tf, 3.14159274f - tf);
  if (usable && mf < thf - LS_MARGIN) return true;
  if (usable && mf > thf + LS_MARGIN) return false;
  return p_is_a ? ls_rare_angle_close(P.x1, P.y1, P.x2, P.y2, dy, dx, lp.angle_thre_rad) : ls_rare_angle_close(Q.x1, Q.y1, Q.x2, Q.y2, dy, dx, lp.angle_thre_rad);
}

// ---- the procedure's steps
// the ROI filter: both end points of segment i of the frame inside the job's expanded bounds
__device__ __forceinline__ bool ls_inside(const double* __restrict__ FL, int i, const BoxGeom& g) {
  return inside_box(v2(FL[4 * i], FL[4 * i + 1]), g.el, g.et, g.er, g.eb) && inside_box(v2(FL[4 * i + 2], FL[4 * i + 3]), g.el, g.et, g.er, g.eb);
}
// 1. the frame's M segments that lie inside the ROI, in input order, into the rows; only rows below CAP are stored.  Returns how many
//    there are, whether stored or not.
template <int CAP>
__device__ __forceinline__ int ls_load(LsRows<CAP>& R, const double* __restrict__ FL, int M, const BoxGeom& g, int lane) {
  int total = 0;
  for (int base = 0; base < M; base += 64) {
    const int i = base + lane;
    const bool in = i < M && ls_inside(FL, i, g);
    const unsigned long long bal = __ballot(in);
    const int off = total + __popcll(bal & ((1ull << lane) - 1ull));
    if (in && off < CAP) {
      const double x1 = FL[4 * i], y1 = FL[4 * i + 1], x2 = FL[4 * i + 2], y2 = FL[4 * i + 3];
      R.store(off, LsRow{ls_angf(x1, y1, x2, y2), x1, y1, x2, y2});
    }
    total += __popcll(bal);
  }
  return total;
}
// the merged row (:499-523): the wider start / end of the two
__device__ __forceinline__ LsRow ls_merged(const LsRow& Ra, const LsRow& Rb) {
  const bool sa = Ra.x1 < Rb.x1, ea = Ra.x2 > Rb.x2;
  LsRow Mg;
  Mg.x1 = sa ? Ra.x1 : Rb.x1; Mg.y1 = sa ? Ra.y1 : Rb.y1; Mg.x2 = ea ? Ra.x2 : Rb.x2; Mg.y2 = ea ? Ra.y2 : Rb.y2;
  Mg.af = ls_angf(Mg.x1, Mg.y1, Mg.x2, Mg.y2);
  return Mg;
}
// 3. one round's tests of the owned row `own` = row a (valid: a row of the job after the merge) against Mg, the merged row now at
//    `as`, and -- test_bs, wave-uniform: some row behind bs exists among this call's rows -- against RL, the row that moved to bs.
//    Tests 1 + 2 first; test 3 for the survivors through one call site: every lane takes its pending test against the merged row first,
//    then the one against the moved row (a second trip only if some lane has both).
struct LsPair { bool as, bs; };
template <bool FLAT>
__device__ __forceinline__ LsPair ls_round_tests(const LsRow& own, int a, bool valid, int as, int bs, bool test_bs, const LsRow& Mg, const LsRow& RL,
                                                 const LineSetupParams& lp, float thf) {
  bool c_as = valid && a != as && ls_t12<FLAT>(own, Mg, lp, thf);
  bool c_bs = false;
  if (test_bs) c_bs = valid && a > bs && ls_t12<FLAT>(RL, own, lp, thf);
  LsPair p{false, false};
  while (__ballot(c_as | c_bs)) {
    const bool vs_merged = c_as, pending = c_as | c_bs;
    const LsRow Q = vs_merged ? Mg : RL;
    const bool r = pending && ls_t3(own, Q, vs_merged && a < as, lp, thf);
    if (vs_merged) { p.as = r; c_as = false; } else if (pending) { p.bs = r; c_bs = false; }
  }
  return p;
}
// 4. keep the rows longer than the threshold (in order), emit their angle (exact: cs_atan2 of the row's end points) / midpoint tables
//    from `out` on; returns how many
template <int CAP>
__device__ __forceinline__ int ls_emit(const LsRows<CAP>& R, int total, const LineSetupParams& lp, int out, double* mid_x, double* mid_y, double* line_angle, int lane) {
  int kept = 0;
  for (int base = 0; base < total; base += 64) {
    const int i = base + lane;
    bool keep = false;
    if (i < total) {
      const double len2 = v2_dist2(v2(R.X2[i], R.Y2[i]), v2(R.X1[i], R.Y1[i]));
      keep = (lp.len_thre > 0) ? (len2 > lp.len_sq_bound) : true;
    }
    const unsigned long long bal = __ballot(keep);
    const int off = kept + __popcll(bal & ((1ull << lane) - 1ull));
    if (keep) {
      line_angle[out + off] = cs_atan2(R.Y2[i] - R.Y1[i], R.X2[i] - R.X1[i]);
      mid_x[out + off] = (R.X1[i] + R.X2[i]) / 2;
      mid_y[out + off] = (R.Y1[i] + R.Y2[i]) / 2;
    }
    kept += __popcll(bal);
  }
  return kept;
}

// ---- the instances.  A job is ONE wavefront in all of them (tid == lane): what counts for the crowded ROIs is the latency of the longest
// job (the batch's chain waits for it), and four wavefronts per job, a ballot apiece and a barrier per round, were measured and dropped
// ("Measured and dropped").  A typical ROI holds a few dozen segments: LS_SMALL rows, the matrix in registers, 4.6 KB of LDS -- the kernel is
// bound by instruction issue, and a CU holds every wave slot's worth of such jobs.  The few crowded ROIs (6 % at C2) keep the matrix in
// LDS: lane l owns the rows l + 64 s, and the ballot of slot s is word s of a partner set.  LS_MID rows hold 17 KB, LS_CAP rows 50 KB.

// One listed job: it comes from line_classify_kernel's lists, which hold no skipped box and no ROI of another size class.
template <int CAP>
__device__ __forceinline__ void line_setup_job(int j, JobDesc* jobs, const double* __restrict__ frame_lines, const int* __restrict__ frame_line_ptr,
                                               double* mid_x, double* mid_y, double* line_angle, const LineSetupParams& lp) {
  constexpr int SL = CAP / 64;                  // rows per lane: lane + 64 s
  constexpr int W = CAP / 64;                   // 64-bit words per partner set; row a's own bit sits in word a >> 6
  __shared__ LsRows<CAP> R;
  __shared__ unsigned long long PM[CAP * W];    // PM[r * W + w]: the partners b in [64 w, 64 w + 64) of row r (bits b > r only)
  const JobDesc jd = jobs[j];
  const double* FL = frame_lines + 4 * (size_t)frame_line_ptr[jd.frame];
  const int M = frame_line_ptr[jd.frame + 1] - frame_line_ptr[jd.frame];
  const int lane = threadIdx.x;
  const float thf = (float)lp.angle_thre_rad;
  const int NONE = 0x7fffffff;
  int total = min(CAP, ls_load(R, FL, M, jd.g, lane));
  for (int e = lane; e < CAP * W; e += 64) PM[e] = 0ull;
  __syncthreads();
  // ---- 2. the pair-test matrix.  Own rows in registers; tests 1 + 2 against every later row b (broadcast), then test 3 for the survivors
  LsRow own[SL];
  int cnt[SL];
#pragma unroll
  for (int s = 0; s < SL; s++) {
    const int a = lane + 64 * s;
    own[s] = (a < total) ? R.row(a) : LsRow{0.f, 0., 0., 0., 0.};
    cnt[s] = 0;
  }
  for (int b = 1; b < total; b++) {
    const LsRow Rb = R.row(b);
#pragma unroll
    for (int s = 0; s < SL; s++) {
      if (64 * s >= b) break;
      const int a = lane + 64 * s;
      if (a < b && ls_t12<false>(own[s], Rb, lp, thf)) PM[a * W + (b >> 6)] |= 1ull << (b & 63);
    }
  }
#pragma unroll
  for (int s = 0; s < SL; s++) {
    if (64 * s >= total) break;
    const int a = lane + 64 * s;
    if (a < total) {
      for (int w = a >> 6; 64 * w < total; w++) {
        unsigned long long v = PM[a * W + w], keep = v;
        while (v) {
          const int b = 64 * w + __ffsll((long long)v) - 1;
          v &= v - 1;
          if (!ls_t3(own[s], R.row(b), true, lp, thf)) keep &= ~(1ull << (b & 63));
        }
        PM[a * W + w] = keep;
        cnt[s] += __popcll(keep);
      }
    }
  }
  __syncthreads();
  // ---- 3. merge rounds
  for (int rounds = 0; rounds < CAP; rounds++) {
    // the first row with a partner
    int as = NONE;
#pragma unroll
    for (int s = 0; s < SL; s++) {
      if (64 * s >= total) break;
      const unsigned long long bal = __ballot(cnt[s] > 0 && lane + 64 * s < total);
      if (bal && as == NONE) as = 64 * s + __ffsll((long long)bal) - 1;
    }
    if (as == NONE) break;
    int bs = -1;
    for (int w = as >> 6; 64 * w < total; w++) {
      const unsigned long long v = PM[as * W + w];
      if (v) { bs = 64 * w + __ffsll((long long)v) - 1; break; }
    }
    const int last = total - 1;
    const LsRow RL = R.row(last), Mg = ls_merged(R.row(as), R.row(bs));
    const bool moved = (bs != last);            // row bs takes what used to be the last row (fast_RemoveRow, matrix_utils.cpp:183)
    __syncthreads();                            // (everybody holds the three rows: they may be rewritten)
    if (lane == 0) { R.store(as, Mg); if (moved) R.store(bs, RL); }
    total = last;
#pragma unroll
    for (int s = 0; s < SL; s++) {              // (slot s: word s of a partner set)
      if (64 * s >= total) {                    // (no rows here any more: the two rebuilt rows hold nothing in these words)
        if (lane == 0) { PM[as * W + s] = 0ull; if (moved) PM[bs * W + s] = 0ull; }
        continue;
      }
      const int a = lane + 64 * s;
      if (a == as) own[s] = Mg;
      else if (moved && a == bs) own[s] = RL;
      const bool valid = a < total;
      const LsPair p = ls_round_tests<false>(own[s], a, valid, as, bs, moved, Mg, RL, lp, thf);
      // the two rebuilt rows' partner sets are these tests' ballots
      const unsigned long long bal_as = __ballot(p.as && a > as), bal_bs = __ballot(p.bs);
      if (lane == 0) { PM[as * W + s] = bal_as; if (moved) PM[bs * W + s] = bal_bs; }
      // every other row: its bit for the old last row goes; its bit for `as` is the fresh test; its bit for `bs` is what its bit for the old last row was
      if (valid && a != as && !(moved && a == bs)) {
        unsigned long long* pm = PM + a * W;
        int d = 0;
        bool old_last = false;
        { const unsigned long long v = pm[last >> 6]; old_last = (v >> (last & 63)) & 1ull; if (old_last) { pm[last >> 6] = v & ~(1ull << (last & 63)); d--; } }
        if (a < as) { const unsigned long long v = pm[as >> 6]; const bool old = (v >> (as & 63)) & 1ull; if (old != p.as) { pm[as >> 6] = v ^ (1ull << (as & 63)); d += p.as ? 1 : -1; } }
        if (moved && a < bs) { const unsigned long long v = pm[bs >> 6]; const bool old = (v >> (bs & 63)) & 1ull; if (old != old_last) { pm[bs >> 6] = v ^ (1ull << (bs & 63)); d += old_last ? 1 : -1; } }
        cnt[s] += d;
      }
    }
    __syncthreads();
    // the owners of the two rebuilt rows count their new partner sets
#pragma unroll
    for (int s = 0; s < SL; s++) {
      const int a = lane + 64 * s;
      if (a == as || (moved && a == bs)) {
        int c = 0;
        for (int w = a >> 6; w < W; w++) c += __popcll(PM[a * W + w]);
        cnt[s] = c;
      }
    }
  }
  const int kept = ls_emit(R, total, lp, jd.line_off, mid_x, mid_y, line_angle, lane);
  if (lane == 0) jobs[j].m = kept;
}
// Which jobs are crowded is asked first: a workgroup of the LDS instances per job of the batch had 94 % of them count their ROI's segments
// and leave again, each holding the instance's 50 KB of LDS while it counted (what that costs: DESIGN.md section 2, "Round 6: what moved").
// line_classify_kernel (a wavefront per job, no LDS) appends the crowded jobs to two lists -- ROIs of up to LS_MID rows, and the rest --
// and the LDS instances' workgroups, a fixed, modest grid, take their jobs from them.
// list[0] = how many, list[1 ..] = the jobs (in the order the atomics fell: the jobs are independent).
__global__ __launch_bounds__(256) void line_classify_kernel(const JobDesc* __restrict__ jobs, int n_jobs, const double* __restrict__ frame_lines, const int* __restrict__ frame_line_ptr,
                                                            int* __restrict__ crowded, int* __restrict__ crowded_big) {
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (j >= n_jobs) return;
  const JobDesc& jd = jobs[j];
  if (jd.Y == 0 || jd.T == 0) return;
  const BoxGeom g = jd.g;
  const double* FL = frame_lines + 4 * (size_t)frame_line_ptr[jd.frame];
  const int M = frame_line_ptr[jd.frame + 1] - frame_line_ptr[jd.frame];
  int n_in = 0;
  for (int base = 0; base < M; base += 64) {
    const int i = base + lane;
    n_in += __popcll(__ballot(i < M && ls_inside(FL, i, g)));
  }
  if (n_in > LS_SMALL && lane == 0) {
    int* list = n_in > LS_MID ? crowded_big : crowded;
    list[1 + atomicAdd(list, 1)] = j;
  }
}
template <int CAP>
__global__ __launch_bounds__(64) void line_setup_listed_kernel(JobDesc* jobs, const double* __restrict__ frame_lines, const int* __restrict__ frame_line_ptr,
                                                              double* mid_x, double* mid_y, double* line_angle, LineSetupParams lp, const int* __restrict__ crowded) {
  const int n = crowded[0];
  for (int k = blockIdx.x; k < n; k += gridDim.x) {
    line_setup_job<CAP>(crowded[1 + k], jobs, frame_lines, frame_line_ptr, mid_x, mid_y, line_angle, lp);
    __syncthreads();      // (the next job rewrites the rows and the matrix)
  }
}

// The typical job -- at most LS_SMALL segments inside the ROI -- with the pair-test matrix in REGISTERS: lane l owns the rows l and l + 64;
// row l's partner set is two words (partners below / from 64 on), row l + 64's one.  Written without data-dependent branches: both
// cheap tests are evaluated for every pair, the exact evaluations sit behind wave-uniform ballots, bit updates select their word with a
// uniform branch.  It looks at every job and leaves the crowded ones, which it recognises while loading, to the listed instances.
__device__ __forceinline__ void ls_setbit(unsigned long long& lo, unsigned long long& hi, int pos, bool val) {   // pos: wave-uniform
  const unsigned long long bit = 1ull << (pos & 63);
  if (pos < 64) lo = val ? (lo | bit) : (lo & ~bit); else hi = val ? (hi | bit) : (hi & ~bit);
}
__device__ __forceinline__ bool ls_getbit(unsigned long long lo, unsigned long long hi, int pos) {
  return (((pos < 64) ? lo : hi) >> (pos & 63)) & 1ull;
}
// a round's repair of the partner set (lo, hi) of row a, one of the rows that were not rewritten: its bit for the old last row goes; its bit
// for `as` is the fresh test; its bit for `bs` is what its bit for the old last row was
__device__ __forceinline__ void ls_repair(unsigned long long& lo, unsigned long long& hi, int a, int total, int as, int bs, int last, bool moved, bool p_as) {
  if (a < total && a != as && !(moved && a == bs)) {
    const bool old_last = ls_getbit(lo, hi, last);
    ls_setbit(lo, hi, last, false);
    if (a < as) ls_setbit(lo, hi, as, p_as);
    if (moved && a < bs) ls_setbit(lo, hi, bs, old_last);
  }
}
__global__ __launch_bounds__(64) void line_setup_small_kernel(JobDesc* jobs, int n_jobs, const double* __restrict__ frame_lines, const int* __restrict__ frame_line_ptr,
                                                              double* mid_x, double* mid_y, double* line_angle, LineSetupParams lp, const int* __restrict__ order) {
  constexpr int CAP = LS_SMALL;
  __shared__ LsRows<CAP> R;
  int j = order ? order[blockIdx.x] : blockIdx.x;   // longest jobs first (the kernel ends with its slowest workgroup)
  if (j >= n_jobs) return;
  const JobDesc jd = jobs[j];
  if (jd.Y == 0 || jd.T == 0) return;   // a box the sweep skips (no yaw / top-edge samples): m stays 0
  const double* FL = frame_lines + 4 * (size_t)frame_line_ptr[jd.frame];
  const int M = frame_line_ptr[jd.frame + 1] - frame_line_ptr[jd.frame];
  const int lane = threadIdx.x;
  const float thf = (float)lp.angle_thre_rad;
  const int NONE = 0x7fffffff;
  int total = ls_load(R, FL, M, jd.g, lane);
  if (total > CAP) return;              // a listed instance's job
  __syncthreads();
  // ---- 2. the pair-test matrix: tests 1 + 2 of the own rows against every later row b (broadcast), then test 3 for the survivors
  LsRow own0 = (lane < total) ? R.row(lane) : LsRow{0.f, 0., 0., 0., 0.};
  LsRow own1 = (lane + 64 < total) ? R.row(lane + 64) : LsRow{0.f, 0., 0., 0., 0.};
  unsigned long long m00 = 0ull, m01 = 0ull, m11 = 0ull;    // row lane: partners < 64 / >= 64; row lane + 64: partners >= 64
  for (int b = 1; b < total; b++) {
    const LsRow Rb = R.row(b);
    const bool t0 = ls_t12<true>(own0, Rb, lp, thf) && lane < b;
    const unsigned long long bit = 1ull << (b & 63);
    if (b < 64) m00 |= t0 ? bit : 0ull;
    else {
      m01 |= t0 ? bit : 0ull;
      if (b > 64) { const bool t1 = ls_t12<true>(own1, Rb, lp, thf) && lane + 64 < b; m11 |= t1 ? bit : 0ull; }
    }
  }
  // every lane walks the survivors of its rows (lowest partner first; three words)
#pragma unroll
  for (int q = 0; q < 3; q++) {
    unsigned long long v = q == 0 ? m00 : (q == 1 ? m01 : m11), keep = v;
    const int wbase = q == 0 ? 0 : 64;
    while (__ballot(v != 0ull)) {
      const bool have = v != 0ull;
      const int b = have ? wbase + __ffsll((long long)v) - 1 : 0;
      const unsigned long long lowbit = v & (0ull - v);
      v ^= lowbit;
      const bool ok = have && ls_t3(q == 2 ? own1 : own0, R.row(b), true, lp, thf);
      if (have && !ok) keep ^= lowbit;
    }
    if (q == 0) m00 = keep; else if (q == 1) m01 = keep; else m11 = keep;
  }
  // ---- 3. merge rounds
  for (int rounds = 0; rounds < CAP; rounds++) {
    const int first0 = m00 ? __ffsll((long long)m00) - 1 : (m01 ? 64 + __ffsll((long long)m01) - 1 : NONE);
    const int first1 = m11 ? 64 + __ffsll((long long)m11) - 1 : NONE;
    int as, bs;
    const unsigned long long bal0 = __ballot(first0 != NONE);
    if (bal0) {
      as = __ffsll((long long)bal0) - 1;
      bs = __builtin_amdgcn_readlane(first0, as);
    } else {
      const unsigned long long bal1 = __ballot(first1 != NONE);
      if (!bal1) break;
      const int l = __ffsll((long long)bal1) - 1;
      as = 64 + l;
      bs = __builtin_amdgcn_readlane(first1, l);
    }
    const int last = total - 1;
    const LsRow RL = R.row(last), Mg = ls_merged(R.row(as), R.row(bs));
    const bool moved = (bs != last);            // row bs takes what used to be the last row (fast_RemoveRow, matrix_utils.cpp:183)
    __syncthreads();
    if (lane == 0) { R.store(as, Mg); if (moved) R.store(bs, RL); }
    __syncthreads();
    total = last;
    // the removed row's partner set goes; the two rewritten rows are read back by their owners
    if (lane == (last & 63)) { if (last < 64) { m00 = 0ull; m01 = 0ull; } else m11 = 0ull; }
    if (lane < total) own0 = R.row(lane);
    const bool two = total > 64;
    if (two && lane + 64 < total) own1 = R.row(lane + 64);
    // this round's tests: every row against the merged row, the rows behind bs against the row that moved there (none of the rows
    // lane is behind bs = 63)
    const LsPair p0 = ls_round_tests<true>(own0, lane, lane < total, as, bs, moved && bs < 63, Mg, RL, lp, thf);
    const unsigned long long bal_as0 = __ballot(p0.as && lane > as), bal_bs0 = __ballot(p0.bs);
    LsPair p1{false, false};
    unsigned long long bal_as1 = 0ull, bal_bs1 = 0ull;
    if (two) {
      p1 = ls_round_tests<true>(own1, lane + 64, lane + 64 < total, as, bs, moved, Mg, RL, lp, thf);
      bal_as1 = __ballot(p1.as && lane + 64 > as); bal_bs1 = __ballot(p1.bs);
    }
    ls_repair(m00, m01, lane, total, as, bs, last, moved, p0.as);
    if (two) { unsigned long long none = 0ull; ls_repair(none, m11, lane + 64, total, as, bs, last, moved, p1.as); }
    // the two rebuilt rows' partner sets are the tests' ballots
    if (as < 64) { if (lane == as) { m00 = bal_as0; m01 = bal_as1; } } else if (lane == as - 64) m11 = bal_as1;
    if (moved) { if (bs < 64) { if (lane == bs) { m00 = bal_bs0; m01 = bal_bs1; } } else if (lane == bs - 64) m11 = bal_bs1; }
  }
  __syncthreads();
  const int kept = ls_emit(R, total, lp, jd.line_off, mid_x, mid_y, line_angle, lane);
  if (lane == 0) jobs[j].m = kept;
}

// The launcher: the crowded ROIs from line_classify_kernel's lists, the others in `order` (null: in job order).  crowded: 2 (n_jobs + 1)
// ints of scratch -- the list of the ROIs of up to LS_MID rows, behind it the list of the larger ones.  The crowded ROIs -- long,
// low-occupancy workgroups -- run on st_crowded beside the others, the mid-size instance behind the large one (on a stream of its own it
// cost 7 % of the sweep's rate); `fork` and `join` are recorded here and st waits for `join`.  st_crowded == st: everything in stream order.
void launch_line_setup_listed(JobDesc* jobs, int n_jobs, const double* frame_lines, const int* frame_line_ptr, double* mid_x, double* mid_y, double* line_angle,
                              double dist_thre, double angle_thre_deg, double len_thre, hipStream_t st, const int* order, hipStream_t st_crowded, hipEvent_t fork, hipEvent_t join, int* crowded) {
  if (skip_kernel("line_setup")) return;
  if (n_jobs <= 0) return;
  LineSetupParams lp{dist_thre, angle_thre_deg / 180.0 * CS_PI, len_thre, sqrt_lt_bound(dist_thre), sqrt_le_bound(len_thre)};
  int* big = crowded + n_jobs + 1;
  (void)hipMemsetAsync(crowded, 0, sizeof(int), st);
  (void)hipMemsetAsync(big, 0, sizeof(int), st);
  hipLaunchKernelGGL(line_classify_kernel, dim3((n_jobs + 3) / 4), dim3(256), 0, st, jobs, n_jobs, frame_lines, frame_line_ptr, crowded, big);
  (void)hipEventRecord(fork, st);
  const int grid = n_jobs < 1024 ? n_jobs : 1024;      // (more crowded ROIs than workgroups: a workgroup takes several)
  if (st_crowded != st) (void)hipStreamWaitEvent(st_crowded, fork, 0);      // (one stream for both: stream order)
  hipLaunchKernelGGL(line_setup_listed_kernel<LS_CAP>, dim3(grid), dim3(64), 0, st_crowded, jobs, frame_lines, frame_line_ptr, mid_x, mid_y, line_angle, lp, big);
  hipLaunchKernelGGL(line_setup_listed_kernel<LS_MID>, dim3(grid), dim3(64), 0, st_crowded, jobs, frame_lines, frame_line_ptr, mid_x, mid_y, line_angle, lp, crowded);
  (void)hipEventRecord(join, st_crowded);
  hipLaunchKernelGGL(line_setup_small_kernel, dim3(n_jobs), dim3(64), 0, st, jobs, n_jobs, frame_lines, frame_line_ptr, mid_x, mid_y, line_angle, lp, order);
  if (st_crowded != st) (void)hipStreamWaitEvent(st, join, 0);
}
int line_setup_capacity() { return LS_CAP; }

}  // namespace cs
