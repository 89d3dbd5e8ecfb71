// band_kernels.hip -- the banded Cholesky of the reduced (pose) system of the bundle adjustment, for gfx950 (MI355X), and the interior /
// separator kernels of the sharded solve ("sharded reduced solve" below).  Raw pointers in, band_solver.h is the seam; nothing here
// knows the BA's data layout.
//
// The pose graph of a trajectory is banded once its vertices are ordered by reverse Cuthill-McKee: cameras are
// coupled to the few neighbours they share landmarks with and to the cuboids they observe.  S is stored as a lower
// band (LD = bandwidth + 1 doubles per column): n * bw^2 flops instead of n^3 / 3 (0.35 Gflop instead of 385 Gflop at
// C4, n = 10494, bw = 182).  So little arithmetic that the factorisation is a chain of dependent 32-column steps and
// its cost is their latency; it therefore runs as ONE persistent (co-resident) kernel, left-looking over column blocks:
//   band_step               a worker workgroup's step: gather the block row's history (64-row x bw strip of L: the block's 32
//                           rows + its own 16 panel rows) through LDS, multiply its rows against the block rows, scale by
//                           the inverse of the diagonal block's factor, meet the team at a grid barrier.  The right-hand
//                           side rides along as one more row below the band, so L y = b costs no extra step.
//   band_diag_phase         one extra workgroup per front factorises the diagonal blocks (POTF2 + inverse in the registers
//                           of one wave) one step ahead of the workers and publishes the inverses.
//   band_chol_coop_kernel   two fronts (forward from the top, reverse from the bottom) + the middle block.
//   band_chol_nested_kernel four fronts: a separator block splits the band in two halves, each eliminated at both ends;
//                           the separator's rows ride along, its Schur complement is accumulated beside the fronts.
//   band_backsolve_kernel   L^T x = y per front with the inverted diagonal blocks (two small mat-vecs per step, every load
//                           that does not depend on x prefetched one step ahead); band_sep_* handle the separator.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>

#include "band_potf2.h"
#include "band_solver.h"
#include "cs_wave.h"

namespace cs {

// Hand-offs between workgroups (other CUs, mostly other XCDs -- whose L2s are not coherent with each other): every shared double is written
// with a write-through (sc1) store and read with an sc1 load that bypasses the reader's L1 -- 8-byte agent-scope relaxed atomics on both
// sides, the second of the valid forms of MI355X_MICROARCH.md -- so a producer only drains its stores (s_waitcnt vmcnt(0)) before it
// raises a counter or a flag, and a consumer only polls: no buffer_wbl2 (a write-back of the XCD's whole L2, >= 1.7 us) per release and
// no buffer_inv per acquire, which is what most of a step's chain used to consist of.  BAND_WT 0 restores plain accesses + agent fences.
#ifndef BAND_WT
#define BAND_WT 1
#endif
#ifndef BAND_WT_LOADS_
#define BAND_WT_LOADS_ 0     // 1: sc1 loads instead of acquire fence + plain loads (measured slower: the strip gather re-reads every entry many times and sc1 loads never hit)
#endif
__device__ __forceinline__ void band_release() {
#if !BAND_WT
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
#endif
}
__device__ __forceinline__ void band_acquire() {
#if !(BAND_WT && BAND_WT_LOADS_)
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#endif
}


// Bounded wait on a monotone counter.  The persistent kernels below need their whole team resident; the host checks that
// against the occupancy query before choosing the banded path (ba_band_fits_device), but a GPU shared with another process's
// persistent kernel can still starve a team.  Such a launch must fail, not hang: after ~1 s of polling the waiter raises the
// abort word of the launch's info block (all barrier counters and flags live in that one 96-byte, 256-byte-aligned block:
// info[BAND_ABORT_SLOT], band_solver.h), marks the factorisation as failed (info[0] = BAND_TIMEOUT_INFO) and every later wait of the
// launch returns at once.
enum { BAND_SPIN_LIMIT = 1 << 21 };
__device__ __forceinline__ void band_wait_ge(unsigned* ctr, unsigned target) {
  unsigned spins = 0;
  while (__hip_atomic_load(ctr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target) {
    __builtin_amdgcn_s_sleep(1);
    if ((++spins & 1023u) == 0) {
      unsigned* base = reinterpret_cast<unsigned*>(reinterpret_cast<unsigned long long>(ctr) & ~127ull);
      if (__hip_atomic_load(base + BAND_ABORT_SLOT, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) break;
      if (spins >= (unsigned)BAND_SPIN_LIMIT) {
        __hip_atomic_store(base + BAND_ABORT_SLOT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(base, (unsigned)BAND_TIMEOUT_INFO, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
    }
  }
}

// All workgroups of the (co-resident) grid arrive; thread 0 spins on the monotone counter.  Producer side: every
// wave drains its stores, lane 0 writes the XCD's L2 back (agent-scope release; the explicit wait restates the one the
// compiler may drop after buffer_wbl2) and arrives; consumer side: relaxed poll, one agent-scope acquire for the CU.
__device__ __forceinline__ void band_grid_sync(unsigned* bar, unsigned target) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    band_release();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    band_wait_ge(bar, target);
    band_acquire();
  }
  __syncthreads();
}

// Out-of-line, one instance per kernel: a device function with a single calling kernel keeps no callee-saved registers
// (the compiler specialises its convention); shared between two kernels it would save and restore ~45 of them per call.
__device__ __attribute__((noinline)) bool band_potf2_inv_k0(const double (*U)[BS + 1], int nb, double (*Dl)[BS + 1], double (*X)[BS + 1], double* colbuf) { return band_potf2_inv4b_impl(U, nb, Dl, X, colbuf); }
__device__ __attribute__((noinline)) bool band_potf2_inv_k1(const double (*U)[BS + 1], int nb, double (*Dl)[BS + 1], double (*X)[BS + 1], double* colbuf) { return band_potf2_inv4b_impl(U, nb, Dl, X, colbuf); }

typedef const __attribute__((address_space(1))) double* band_gptr;   // global address space: a noinline function would otherwise emit flat loads
__device__ __forceinline__ double band_gload(const double* p) {
#if BAND_WT && BAND_WT_LOADS_
  return __longlong_as_double((long long)__hip_atomic_load((const __attribute__((address_space(1))) unsigned long long*)(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
#else
  return *(band_gptr)(p);
#endif
}
__device__ __forceinline__ void band_gstore(const double* p, double v) {
#if BAND_WT
  __hip_atomic_store((__attribute__((address_space(1))) unsigned long long*)(const_cast<double*>(p)), (unsigned long long)__double_as_longlong(v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
  *const_cast<double*>(p) = v;
#endif
}
// plain store: ONLY in kernels whose workgroups hand nothing to each other within a launch (the substitution kernels: a front is
// walked by one workgroup, the kernel boundary publishes the result)
__device__ __forceinline__ void band_pstore(const double* p, double v) { *const_cast<double*>(p) = v; }

// panel rows per workgroup, per kernel.  16 in both: 8 rows in the nested kernel (twice the workgroups, half the product and
// panel work) was measured slower, 1.95 -> 2.15 ms at C4 -- what the halves save, the doubled teams lose in the barrier (2.5 ->
// 4.6 us), the gather (more workgroups behind the same L2) and the wait for the diagonal workgroup
enum { BAND_RW = 16, BAND_RW_NESTED = 16, BAND_NR = BS + BAND_RW + 8, BAND_NRP = 64, BAND_DC = 192, BAND_NV = BAND_DC * BAND_NRP / 256 };
__host__ __device__ constexpr int band_rw(int kid) { return kid ? BAND_RW_NESTED : BAND_RW; }

// An elimination front addresses the band through its own index space (v = 0 is where it starts): the forward front
// walks the matrix top-left to bottom-right (v = original index), the reverse front bottom-right to top-left
// (v = n - 1 - original index).  In both spaces the factor is lower triangular and banded; only the strides differ:
//   &L(i, j) = base + i * si + j * sj   (i >= j, i - j <= bw),      &rhs(v) = rb + v * sr
//   forward: base = Sb, si = 1, sj = bw              reverse: base = Sb + (n - 1) LD, si = -bw, sj = -1
// (Every global pointer of the persistent kernels is const-qualified: the ONLY ways to write through one are band_gstore -- the
// write-through store the hand-offs rely on -- and band_pstore, a plain store for kernels whose workgroups exchange nothing within a
// launch.  A plain `p[i] = v` in a step routine does not compile, so a future edit cannot slip a store past the hand-off protocol.)
struct BandView {
  const double* base; long long si, sj;
  const double* rb; long long sr;
};
struct BandSeg {            // one run of history columns [jlo, jhi) of a view; flip: the step's rows are re-indexed i -> n - 1 - i
  BandView v; int jlo, jhi, flip;
};
struct BandSegX : BandSeg { // ... of a front that carries separator rows (BandAug): their history of view column j >= lc_jmin
  int lc_t0, lc_jmin;       // is column lc_t0 + j of aug.lc
};
// Rows of a separator block that ride below a front (nested elimination, see band_chol_nested_kernel): row q of the
// separator against column j of the front's view.  A(q, j) is an entry of the band (zero outside it); the factor's
// entries fill in, so they live in their own array.  wc == 0: no such rows.
struct BandAug {
  const double* a_base; long long a_sq, a_sj;   // &A(q, j) = a_base + q a_sq + j a_sj, inside the band iff m0 + q + ms j <= bw
  int m0, ms;
  const double* lc; int wc, qflip, t0;          // &L(q, j) = lc + (t0 + j) wc + (qflip ? wc - 1 - q : q)   (t0: the view being eliminated)
};
struct BandLds { double* R; double (*U)[BS + 1]; double (*Dl)[BS + 1]; double (*X)[BS + 1]; double* colbuf; int* rowidx; };

// Strip gather + product of one step: U(rr, c) = A(rr, k0 + c) - sum_j L(rr, j) L(k0 + c, j) for the 32 block rows and
// this workgroup's rows, the history columns j coming from one or two segments (the second one only in the middle
// phase of the two-sided elimination: the other front's columns).  A thread gathers ONE row (rr = tid & 63) at every
// fourth column, so the addresses are a pointer walk, and all BAND_NV loads are unconditional (masked lanes read the
// zero word) and in flight together.
__device__ __forceinline__ int band_seg_jmin(const BandSeg&) { return 0; }
__device__ __forceinline__ int band_seg_jmin(const BandSegX& s) { return s.lc_jmin; }
__device__ __forceinline__ int band_seg_t0(const BandSeg&) { return 0; }
__device__ __forceinline__ int band_seg_t0(const BandSegX& s) { return s.lc_t0; }
template <bool AUG, class SEG, int RW>
__device__ __forceinline__ void band_gather_gemm_impl(const SEG& s0, const SEG& s1, int nseg, const BandAug& aug, const double* zero, int n, int bw, int k0, int nb, const int* rowidx,
                                                           double* R, double (*U)[BS + 1], long long* tp, long long* t_prev) {
  constexpr int NR = BS + RW + 8, NRP = BAND_NRP, NOWN = RW + 8, NRT = NOWN / 8, NV = BAND_NV, DC = BAND_DC;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int c1 = tid & 31, rg1 = tid >> 5;      // one-column mapping of the finishing pass
#define BAND_TICK(k) do { if (tp) { long long t_now = wall_clock64(); tp[k] += t_now - *t_prev; *t_prev = t_now; } } while (0)
  // the block's own columns (A of U = A - sum), in the step's own view s0.v: loads in flight while the strip is gathered
  double aval[NRT];
#pragma unroll
  for (int m = 0; m < NRT; m++) {
    const int i = rowidx[BS + rg1 + 8 * m], dlt = i - (k0 + c1), qa = -16 - i;   // i <= -16: separator row qa
    const bool ok = c1 < nb && (i == -2 || (i >= 0 && dlt >= 0 && dlt <= bw) || (AUG && i <= -16 && aug.m0 + qa + aug.ms * (k0 + c1) <= bw));
    const double* ptr = (i == -2) ? s0.v.rb + (long long)(k0 + c1) * s0.v.sr
                      : (AUG && i <= -16) ? aug.a_base + (long long)qa * aug.a_sq + (long long)(k0 + c1) * aug.a_sj
                                          : s0.v.base + (long long)i * s0.v.si + (long long)(k0 + c1) * s0.v.sj;
    aval[m] = band_gload(ok ? ptr : zero);
  }
  static_assert(NOWN <= 32 && NRP >= BS + 32, "two 16-row MFMA tiles of own rows");
  ba_v4d macc[2][2];
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int u = 0; u < 2; u++) macc[t][u] = ba_v4d{0.0, 0.0, 0.0, 0.0};
  const int row0 = lane < NR ? rowidx[lane] : -1;            // the row this thread gathers (in the step's view)
  for (int sg = 0; sg < nseg; sg++) {
    const SEG S = sg ? s1 : s0;
    const int my_i = (S.flip && row0 >= 0) ? n - 1 - row0 : row0;
    const bool sep = AUG && my_i <= -16;                           // a separator row: history in aug.lc
    const int qc = aug.qflip ? aug.wc - 1 - (-16 - my_i) : (-16 - my_i);
    const int jmin = my_i >= 0 ? max(S.jlo, my_i - bw) : (sep ? max(S.jlo, band_seg_jmin(S)) : S.jlo);   // in-band columns of that row: j >= i - bw
    double vals[NV];
    auto fetch = [&](int j0) {
      const int jend = (my_i == -1) ? 0 : min(S.jhi, j0 + DC);
      int j = j0 + wv;
      const double* p = (my_i == -2) ? S.v.rb + (long long)j * S.v.sr
                      : sep ? aug.lc + (long long)(band_seg_t0(S) + j) * aug.wc + qc
                            : S.v.base + (long long)(my_i >= 0 ? my_i : 0) * S.v.si + (long long)j * S.v.sj;
      const long long step = (my_i == -2) ? 4 * S.v.sr : (sep ? 4LL * aug.wc : 4 * S.v.sj);
#pragma unroll
      for (int u = 0; u < NV; u++) {
        const bool ok = j >= jmin && j < jend;
        vals[u] = band_gload(ok ? p : zero);
        p += step; j += 4;
      }
    };
    if (S.jlo < S.jhi) fetch(S.jlo);
    BAND_TICK(6);
    for (int j0 = S.jlo; j0 < S.jhi; j0 += DC) {
      const int jn = min(DC, S.jhi - j0);
#pragma unroll
      for (int u = 0; u < NV; u++) R[(wv + 4 * u) * NRP + lane] = vals[u];
      __syncthreads();
      BAND_TICK(7);
      if (j0 + DC < S.jhi) fetch(j0 + DC);
      BAND_TICK(6);
      // this wave's quarter of the depth on the matrix cores: acc(own rows, block columns) += sum_d R(d, rows) R(d, cols) as
      // v_mfma_f64_16x16x4_f64 tiles (own rows padded to 32: 2 x 2 tiles), four depth indices per issue; of every 16 depth indices
      // wave w takes 4 w .. 4 w + 3.  Rows of R past the chunk's jn were stored as zeros by the gather, so the last step may
      // overrun jn.  Operand lane map: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15].
      {
        const int li = lane & 15, lk = lane >> 4;
        for (int d0 = 4 * wv; d0 < jn; d0 += 16) {
          const double* rj = R + (d0 + lk) * NRP;
          const double a0 = rj[BS + li], a1 = rj[BS + 16 + li], b0 = rj[li], b1 = rj[16 + li];
          macc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, macc[0][0], 0, 0, 0);
          macc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, macc[0][1], 0, 0, 0);
          macc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, macc[1][0], 0, 0, 0);
          macc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, macc[1][1], 0, 0, 0);
        }
      }
      __syncthreads();
      BAND_TICK(8);
    }
  }
  // partial sums of the 4 waves -> LDS (over the strip buffer), then U = A - sum.  D[row = (lane >> 4) + 4 g][col = lane & 15].
#pragma unroll
  for (int t = 0; t < 2; t++)
#pragma unroll
    for (int u = 0; u < 2; u++)
#pragma unroll
      for (int g = 0; g < 4; g++) R[(wv * NRP + BS + 16 * t + (lane >> 4) + 4 * g) * BS + 16 * u + (lane & 15)] = macc[t][u][g];
  __syncthreads();
#pragma unroll
  for (int m = 0; m < NRT; m++) {
    const int rr = BS + rg1 + 8 * m;
    const double sum = (R[(0 * NRP + rr) * BS + c1] + R[(1 * NRP + rr) * BS + c1]) + (R[(2 * NRP + rr) * BS + c1] + R[(3 * NRP + rr) * BS + c1]);
    U[rr][c1] = aval[m] - sum;
  }
  __syncthreads();
  BAND_TICK(1);
#undef BAND_TICK
}
// out-of-line instances: fronts without / with separator rows
__device__ __attribute__((noinline)) void band_gather_gemm_plain_k0(BandSeg s0, BandSeg s1, int nseg, const double* zero, int n, int bw, int k0, int nb, const int* rowidx,
                                                                    double* R, double (*U)[BS + 1], long long* tp, long long* t_prev) {
  const BandAug noaug{zero, 0, 0, 0, 0, nullptr, 0, 0, 0};
  band_gather_gemm_impl<false, BandSeg, band_rw(0)>(s0, s1, nseg, noaug, zero, n, bw, k0, nb, rowidx, R, U, tp, t_prev);
}
__device__ __attribute__((noinline)) void band_gather_gemm_plain_k1(BandSeg s0, BandSeg s1, int nseg, const double* zero, int n, int bw, int k0, int nb, const int* rowidx,
                                                                    double* R, double (*U)[BS + 1], long long* tp, long long* t_prev) {
  const BandAug noaug{zero, 0, 0, 0, 0, nullptr, 0, 0, 0};
  band_gather_gemm_impl<false, BandSeg, band_rw(1)>(s0, s1, nseg, noaug, zero, n, bw, k0, nb, rowidx, R, U, tp, t_prev);
}
__device__ __attribute__((noinline)) void band_gather_gemm_sep(BandSegX s0, BandSegX s1, int nseg, BandAug aug, const double* zero, int n, int bw, int k0, int nb, const int* rowidx,
                                                               double* R, double (*U)[BS + 1], long long* tp, long long* t_prev) {
  band_gather_gemm_impl<true, BandSegX, band_rw(1)>(s0, s1, nseg, aug, zero, n, bw, k0, nb, rowidx, R, U, tp, t_prev);
}

// arrive without waiting (a workgroup that leaves the kernel): the release half of band_grid_sync
__device__ __forceinline__ void band_grid_arrive(unsigned* bar) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    band_release();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// One elimination step of `view`: block column k0 (nb wide), rows up to i_end, history segments s0 (the view's own
// columns) and s1.  Workgroup roles: cw < 0: panel rows own0 = k0 + nb + RW w ... of the view (has_rhs: plus the
// right-hand side); cw >= 0: separator rows RW cw ... of aug.  Every workgroup factorises the diagonal block itself.
template <int KID>
__device__ __forceinline__ void band_gather_gemm(const BandSeg& s0, const BandSeg& s1, int nseg, const BandAug&, const double* zero, int n, int bw, int k0, int nb, const int* rowidx,
                                                 double* R, double (*U)[BS + 1], long long* tp, long long* t_prev) {
  if (KID == 0) band_gather_gemm_plain_k0(s0, s1, nseg, zero, n, bw, k0, nb, rowidx, R, U, tp, t_prev);
  else band_gather_gemm_plain_k1(s0, s1, nseg, zero, n, bw, k0, nb, rowidx, R, U, tp, t_prev);
}
template <int KID>
__device__ __forceinline__ void band_gather_gemm(const BandSegX& s0, const BandSegX& s1, int nseg, const BandAug& aug, const double* zero, int n, int bw, int k0, int nb, const int* rowidx,
                                                 double* R, double (*U)[BS + 1], long long* tp, long long* t_prev) {
  band_gather_gemm_sep(s0, s1, nseg, aug, zero, n, bw, k0, nb, rowidx, R, U, tp, t_prev);
}
template <bool AUG, int KID, class SEG>
__device__ __forceinline__ void band_step(const BandLds& M, const BandView& view, const double* Linv, int k0, int nb, int i_end, const SEG& s0, const SEG& s1, int nseg,
                                          const BandAug& aug, int w, int cw, bool has_rhs, int n, int bw, const double* zero, unsigned* dflag, unsigned dtarget, long long* tp, long long* t_prev) {
  constexpr int RW = band_rw(KID), NR = BS + RW + 8;
  const int tid = threadIdx.x;
  const int own0 = k0 + nb + w * RW;
  if (tid < NR) {                                   // row (in the view's index space) of gathered row rr; -1 = none, -2 = right-hand side, <= -16: separator row
    int i = -1;
    if (tid < BS) i = tid < nb ? k0 + tid : -1;
    else if (tid - BS < RW) {
      if (cw >= 0) { const int q = cw * RW + (tid - BS); i = q < aug.wc ? -16 - q : -1; }
      else { const int q = own0 + (tid - BS); i = q < i_end ? q : -1; }
    }
    else if (tid - BS == RW && has_rhs) i = -2;
    M.rowidx[tid] = i;
  }
  __syncthreads();
  band_gather_gemm<KID>(s0, s1, nseg, aug, zero, n, bw, k0, nb, M.rowidx, M.R, M.U, tp, t_prev);
  // the inverse of the block's factor comes from the front's diagonal workgroup (band_diag_phase), normally before it is asked for
  if (tid == 0) {
    band_wait_ge(dflag, dtarget);
    band_acquire();
  }
  __syncthreads();
  {
    const double* Li = Linv + (size_t)(k0 / BS) * BS * BS;
    double xv[4];
#pragma unroll
    for (int u = 0; u < 4; u++) xv[u] = band_gload(Li + tid + 256 * u);
#pragma unroll
    for (int u = 0; u < 4; u++) { const int e = tid + 256 * u; M.X[e >> 5][e & 31] = xv[u]; }
  }
  __syncthreads();
  if (tp) { long long t_now = wall_clock64(); tp[2] += t_now - *t_prev; *t_prev = t_now; }
  // own rows (and the right-hand side): row <- row * L^-T
  for (int e = tid; e < (RW + 1) * BS; e += 256) {
    const int q = e >> 5, cc = e & 31, rr = BS + q, i = M.rowidx[rr];
    if (cc < nb && i != -1) {
      // X is stored with its upper triangle zeroed: the full-length dot product in four independent chains
      double sa[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int t = 0; t < BS; t += 4)
#pragma unroll
        for (int u = 0; u < 4; u++) sa[u] = fma(M.U[rr][t + u], M.X[cc][t + u], sa[u]);
      const double sacc = (sa[0] + sa[1]) + (sa[2] + sa[3]);
      if (i >= 0) { if (i - (k0 + cc) <= bw) band_gstore(&view.base[(long long)i * view.si + (long long)(k0 + cc) * view.sj], sacc); }
      else if (i == -2) band_gstore(&view.rb[(long long)(k0 + cc) * view.sr], sacc);
      else if (AUG) { const int qa = -16 - i; band_gstore(&aug.lc[(long long)(aug.t0 + k0 + cc) * aug.wc + (aug.qflip ? aug.wc - 1 - qa : qa)], sacc); }
    }
  }
  if (tp) { long long t_now = wall_clock64(); tp[4] += t_now - *t_prev; *t_prev = t_now; }
}
// ---- the diagonal workgroup of a front.  One extra workgroup per front factorises the diagonal blocks, so the 32-step
// chain of POTF2 leaves the other workgroups' step: while they still gather and multiply their strips of step k, it
// already holds sum_j L(k rows, j) L(k rows, j)^T over all history but the newest 32 columns (accumulated during step
// k - 1), adds those after the team's barrier, factorises, and publishes L_kk^-1 (and L_kk) with a monotone flag.

// acc(4 rg + m, 4 cg + t) += this wave's quarter of sum over columns j in [jlo, jhi) of S.v of L(k0 + row, j) L(k0 + col, j);
// rg = lane >> 3, cg = lane & 7; the four waves' partial sums meet when U is formed
template <int DC, class SEG>
__device__ __forceinline__ void band_diag_accum(const SEG& S, int jlo, int jhi, int n, int bw, int k0, int nb, const double* zero, double* R, double (&acc)[4][4]) {
  constexpr int LDR = BS + 1;
  const int tid = threadIdx.x, gr = tid & 31, ph = tid >> 5, lane = tid & 63, wv = tid >> 6, rg = lane >> 3, cg = lane & 7;
  const int i = k0 + gr, my_i = S.flip ? n - 1 - i : i;
  const int jmin = max(jlo, my_i - bw);
  const double* rowp = S.v.base + (long long)my_i * S.v.si;
  for (int j0 = jlo; j0 < jhi; j0 += DC) {
    const int jend = gr < nb ? min(jhi, j0 + DC) : 0;
    double vals[DC / 8];
#pragma unroll
    for (int u = 0; u < DC / 8; u++) {
      const int j = j0 + ph + 8 * u;
      vals[u] = band_gload((j >= jmin && j < jend) ? rowp + (long long)j * S.v.sj : zero);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < DC / 8; u++) R[(ph + 8 * u) * LDR + gr] = vals[u];
    __syncthreads();
    const int jn = min(DC, jhi - j0);
#pragma unroll 4
    for (int jj = wv; jj < jn; jj += 4) {
      const double* rj = R + jj * LDR;
      double rowv[4], colv[4];
#pragma unroll
      for (int m = 0; m < 4; m++) { rowv[m] = rj[4 * rg + m]; colv[m] = rj[4 * cg + m]; }
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int t = 0; t < 4; t++) acc[m][t] = fma(rowv[m], colv[t], acc[m][t]);
    }
  }
}
// The diagonal blocks k_begin, k_begin + 32, ... < k_end of `view` (one phase of a front).  History of block k0: the
// view's own columns [max(0, k0 - bw), k0) and, with two_seg, the columns [max(0, (n - min(k_end, k0 + nb + bw)) - bw), jhi1)
// of the other front's view v1 (rows re-indexed i -> n - 1 - i).  start: counter/target that opens the phase (may be null);
// bar: the team's step barrier, which reads G ep0 when the phase starts; flag: published block count, f0 at the start.
template <int KID>
__device__ __forceinline__ void band_diag_phase(const BandLds& M, const BandView& view, const double* Linv, int k_begin, int k_end, bool two_seg, const BandView& v1, int jhi1,
                                                unsigned* start, unsigned start_target, unsigned* bar, unsigned G, unsigned ep0, unsigned* flag, unsigned f0,
                                                int n, int bw, const double* zero, int* info, long long* dprof = nullptr) {
  const int tid = threadIdx.x, r = tid >> 3, cq = tid & 7, lane = tid & 63, wv = tid >> 6, rg = lane >> 3, cg = lane & 7;
  long long dt_prev = dprof ? wall_clock64() : 0;      // optional phase clock of this workgroup (CS_BAND_PROF): wait, newest block + U, POTF2, publish, look-ahead
#define BAND_DTICK(k) do { if (dprof && tid == 0) { const long long t_now = wall_clock64(); dprof[k] += t_now - dt_prev; dt_prev = t_now; } } while (0)
  auto wait_for = [&](unsigned* ctr, unsigned target) {
    if (tid == 0) {
      band_wait_ge(ctr, target);
      band_acquire();
    }
    __syncthreads();
  };
  auto seg1 = [&](int k0, int nb) { return BandSeg{v1, max(0, (n - min(k_end, k0 + nb + bw)) - bw), jhi1, 1}; };
  double acc[4][4];
#pragma unroll
  for (int m = 0; m < 4; m++)
#pragma unroll
    for (int t = 0; t < 4; t++) acc[m][t] = 0.0;
  unsigned s = 0;
  for (int k0 = k_begin; k0 < k_end; k0 += BS, s++) {
    const int nb = min(BS, k_end - k0);
    const BandSeg s0{view, max(0, k0 - bw), k0, 0};
    double av[4];                                // the block's own entries (lower triangle)
    auto load_block = [&]() {
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int c = 4 * cq + t;
        const bool ok = r < nb && c <= r && r - c <= bw;
        av[t] = band_gload(ok ? view.base + (long long)(k0 + r) * view.si + (long long)(k0 + c) * view.sj : zero);
      }
    };
    if (s > 0) load_block();                     // in flight across the wait (nobody writes the block before this workgroup does)
    if (s == 0) {
      if (start) wait_for(start, start_target);  // (the gate may be what completes the matrix itself: the separator block)
      load_block();
      band_diag_accum<BAND_DC>(s0, s0.jlo, k0, n, bw, k0, nb, zero, M.R, acc);
      if (two_seg) { const BandSeg s1 = seg1(k0, nb); band_diag_accum<BAND_DC>(s1, s1.jlo, s1.jhi, n, bw, k0, nb, zero, M.R, acc); }
    } else {
      BAND_DTICK(4);
      wait_for(bar, (ep0 + s) * G);
      BAND_DTICK(0);
      band_diag_accum<BS>(s0, max(s0.jlo, k0 - BS), k0, n, bw, k0, nb, zero, M.R, acc);   // the newest block: 4 loads per thread
    }
    // U = A - sum of the four waves' partial sums (lower triangle)
    {
      __syncthreads();
      double* part = M.R;                       // [wave][32][33]
#pragma unroll
      for (int m = 0; m < 4; m++)
#pragma unroll
        for (int t = 0; t < 4; t++) part[(wv * BS + 4 * rg + m) * (BS + 1) + 4 * cg + t] = acc[m][t];
      __syncthreads();
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const int o = r * (BS + 1) + 4 * cq + t, ws = BS * (BS + 1);
        M.U[r][4 * cq + t] = av[t] - ((part[o] + part[ws + o]) + (part[2 * ws + o] + part[3 * ws + o]));
      }
    }
    __syncthreads();
    BAND_DTICK(1);
    {
      const bool bad = KID == 0 ? band_potf2_inv_k0(M.U, nb, M.Dl, M.X, M.colbuf) : band_potf2_inv_k1(M.U, nb, M.Dl, M.X, M.colbuf);
      if (bad && tid == 0) atomicCAS(info, 0, k0 + 1);
    }
    __syncthreads();
    BAND_DTICK(2);
    {
      const double* Li = Linv + (size_t)(k0 / BS) * BS * BS;
      for (int e = tid; e < BS * BS; e += 256) {
        const int rr = e >> 5, cc = e & 31;
        band_gstore(&Li[e], M.X[rr][cc]);
        if (rr < nb && cc <= rr && rr - cc <= bw) band_gstore(&view.base[(long long)(k0 + rr) * view.si + (long long)(k0 + cc) * view.sj], M.Dl[rr][cc]);
      }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      band_release();
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __hip_atomic_store(flag, f0 + s + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    BAND_DTICK(3);
    // the next block's history except its newest 32 columns (those wait for the team's barrier)
#pragma unroll
    for (int m = 0; m < 4; m++)
#pragma unroll
      for (int t = 0; t < 4; t++) acc[m][t] = 0.0;
    const int k1 = k0 + BS;
    if (k1 < k_end) {
      const int nb1 = min(BS, k_end - k1);
      const BandSeg n0{view, max(0, k1 - bw), k1, 0};
      band_diag_accum<BAND_DC>(n0, n0.jlo, max(n0.jlo, k1 - BS), n, bw, k1, nb1, zero, M.R, acc);
      if (two_seg) { const BandSeg n1 = seg1(k1, nb1); band_diag_accum<BAND_DC>(n1, n1.jlo, n1.jhi, n, bw, k1, nb1, zero, M.R, acc); }
    }
  }
}

#undef BAND_DTICK
// (see band_potf2_inv_k0: a caller-side object whose address escapes before the first out-of-line call keeps those calls from
// being marked as tail-call candidates, which would switch the callees back to the save-everything convention)
__device__ __attribute__((noinline)) void band_clock_init(long long* t) { asm volatile("" : : "v"(t) : "memory"); *t = 0; }

// Two-sided ("burn at both ends") elimination.  Phase 1: team 0 eliminates the first K1 column blocks with the forward
// front while team 1 eliminates the last K2 column blocks with the reverse front -- the two regions are further apart
// than the bandwidth, so they never touch the same entries; each front also produces the rows of L that reach into the
// middle block M = [32 K1, n - 32 K2).  Phase 2: team 0 eliminates M, whose history now has two segments (the tails of
// both fronts).  The chain of dependent steps is halved.  K2 = 0 degenerates to the one-sided left-looking algorithm.
// bars: [team 0, team 1, both].
__global__ __launch_bounds__(256) void band_chol_coop_kernel(const double* Sb, const double* __restrict__ Linv_f, const double* __restrict__ Linv_r, const double* rhs, const double* zero, int n,
                                                             int LD, int K1, int K2, int* info, unsigned* bars, int G, long long* prof) {
  __shared__ double R[BAND_DC * BAND_NRP];   // strip chunk, transposed: R[jj * 64 + rr]; afterwards the 4 waves' partial sums
  __shared__ double U[BAND_NR][BS + 1];
  __shared__ double Dl[BS][BS + 1];
  __shared__ double X[BS][BS + 1];
  __shared__ double colbuf[2 * 256];
  __shared__ int rowidx[BAND_NR];
  const BandLds M{R, U, Dl, X, colbuf, rowidx};
  const int team = blockIdx.x / (G + 1), w = blockIdx.x % (G + 1);   // w == G: the front's diagonal workgroup
  const int tid = threadIdx.x;
  const int bw = LD - 1;
  const bool has_rhs = (w == G - 1);
  unsigned* dflag = bars + (BAND_INFO_PUBLISHED - BAND_INFO_BARS) + team;
  long long t_escape; band_clock_init(&t_escape);
  const BandView fwd{Sb, 1, (long long)bw, rhs, 1};
  const BandView rev{Sb + (size_t)(n - 1) * LD, -(long long)bw, -1, rhs + (n - 1), -1};
  const int m_begin = BS * K1, m_end = n - BS * K2;      // the middle block (original indices)
  long long tp[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t_prev = prof ? wall_clock64() : 0;   // optional phase clock (CS_BAND_PROF)
  const long long c_begin = prof ? clock64() : 0, w_begin = t_prev;
  const bool clocked = prof && team == 0;
  long long* tpp = clocked ? tp : nullptr;
#define BAND_TICK(k) do { if (clocked) { long long t_now = wall_clock64(); tp[k] += t_now - t_prev; t_prev = t_now; } } while (0)
  const BandSeg none{fwd, 0, 0, 0};
  const BandAug noaug{zero, 0, 0, 0, 0, nullptr, 0, 0, 0};
  // ---- phase 1: the two fronts, each with its own barrier (after every step, the last one included: the deferred
  // write of the diagonal block must not overtake a team-mate still reading A's block)
  unsigned ep = 0;   // barriers completed on this team's counter
  if (w == G) {
    const BandView view = team ? rev : fwd;
    band_diag_phase<0>(M, view, team ? Linv_r : Linv_f, 0, BS * (team ? K2 : K1), false, rev, 0, nullptr, 0, bars + team, (unsigned)G, 0, dflag, 0, n, bw, zero, info);
    // the middle block opens when both fronts have met (one-sided order: when the forward front's last barrier is through)
    if (team == 0) band_diag_phase<0>(M, fwd, Linv_f, m_begin, m_end, K2 > 0, rev, BS * K2, K2 > 0 ? bars + 2 : bars + 0, K2 > 0 ? 2u * (unsigned)G : (unsigned)K1 * (unsigned)G, bars + 0, (unsigned)G, (unsigned)K1, dflag, (unsigned)K1, n, bw, zero, info);
    return;
  }
  {
    const BandView view = team ? rev : fwd;
    const double* Linv = team ? Linv_r : Linv_f;
    const int Kt = team ? K2 : K1;
    for (int kb = 0; kb < Kt; kb++) {
      const int k0 = kb * BS;
      const BandSeg s0{view, max(0, k0 - bw), k0, 0};
      band_step<false, 0>(M, view, Linv, k0, BS, min(n, k0 + BS + bw), s0, none, 1, noaug, w, -1, has_rhs, n, bw, zero, dflag, ep + 1, tpp, &t_prev);
      ep++;
      band_grid_sync(bars + team, ep * (unsigned)G);
      BAND_TICK(5);
    }
    if (K2 > 0) {   // the fronts meet: the reverse team publishes and leaves, the forward team waits for it
      if (team) { band_grid_arrive(bars + 2); return; }
      band_grid_sync(bars + 2, 2u * (unsigned)G);
    }
  }
  // ---- phase 2: the middle block, forward front, history = tail of the forward front (+ M's own earlier columns) and
  // tail of the reverse front
  for (int k0 = m_begin; k0 < m_end; k0 += BS) {
    const int nb = min(BS, m_end - k0);
    const int i_end = min(m_end, k0 + nb + bw);
    const BandSeg s0{fwd, max(0, k0 - bw), k0, 0};
    const BandSeg s1{rev, max(0, (n - i_end) - bw), BS * K2, 1};     // rows i -> i' = n - 1 - i; columns of the reverse front within the band
    band_step<false, 0>(M, fwd, Linv_f, k0, nb, i_end, s0, s1, K2 > 0 ? 2 : 1, noaug, w, -1, has_rhs, n, bw, zero, dflag, ep + 1, tpp, &t_prev);
    ep++;
    band_grid_sync(bars + 0, ep * (unsigned)G);
    BAND_TICK(5);
  }
  if (prof && tid == 0 && (w == 0 || w == G - 1)) for (int k = 0; k < 9; k++) prof[(w == 0 ? 0 : 9) + k] = tp[k];
  if (prof && tid == 0 && w == 0) { prof[18] = clock64() - c_begin; prof[19] = wall_clock64() - w_begin; }
#undef BAND_TICK
}

// Nested elimination: four fronts.  A separator block C (wc >= bw columns in the middle of the matrix) splits the band
// into a left and a right half that touch only through C.  Each half is eliminated "at both ends" as above -- the left
// one in the matrix's own index space, the right one in the mirrored one (v = n - 1 - index), so that in both C lies
// below the half -- by two teams: team 0 the front that starts at the far end, team 1 the front that starts next to C
// and then the half's middle block.  The rows of C ride along with team 1 as extra panel rows (GC more workgroups): they
// fill in across everything team 1 eliminates, so their factor entries go to a dense array lc[t][q] (t: elimination
// column of the half, q: row of C).  A third team per half (GC workgroups, 16 rows of C each) accumulates C's Schur
// complement sum_t L(i, t) L(j, t) one step behind team 1, off the chain.  When both halves are done, C -- a dense
// wc x wc block in its own storage -- is factorised by the same step routine.  Chain of dependent steps: about
// n / (4 * 32) instead of n / (2 * 32).
struct BandHalf {
  BandView fv, rv;        // the half's index space [0, nh) (C at rows nh ...) and its reverse front's (u = nh - 1 - v)
  int nh, K1, K2, qflip;  // column blocks of the two fronts; qflip: C's rows appear in reverse order below this half
  const double* Linv_f; const double* Linv_r; const double* lc;
};
struct BandNested {
  BandHalf h[2];
  int n, bw, wc, c0, LD, G, GC, GS;     // C = [c0, c0 + wc); G workgroups per front, GC for C's rows (and C's own factorisation), GS Schur accumulators
  const double* Sb; const double* rhs; const double* SC; const double* rhsC; const double* LinvC; const double* part;
  const double* zero; int* info; unsigned* bars;   // bars: [half 0: team 0, team 1, join][half 1: ...][teams 1 + 2 of both halves][-][C team]
  long long* prof;                                 // optional phase stamps of half 0's team 1 (CS_BAND_PROF)
};
__device__ __forceinline__ const double* band_half_y(const BandHalf& H, int t) {   // right-hand side entry of elimination column t of team 1
  const int Trev = BS * H.K2;
  return t < Trev ? H.rv.rb + (long long)t * H.rv.sr : H.fv.rb + (long long)(BS * H.K1 + t - Trev) * H.fv.sr;
}
__global__ __launch_bounds__(256) void band_chol_nested_kernel(BandNested P) {
  __shared__ double R[BAND_DC * BAND_NRP];
  __shared__ double U[BAND_NR][BS + 1];
  __shared__ double Dl[BS][BS + 1];
  __shared__ double X[BS][BS + 1];
  __shared__ double colbuf[2 * 256];
  __shared__ int rowidx[BAND_NR];
  const BandLds M{R, U, Dl, X, colbuf, rowidx};
  const int tid = threadIdx.x;
  const int G = P.G, G1 = P.G + P.GC, per = (G + 1) + (G1 + 1) + P.GS;   // team 0 + its diagonal workgroup, team 1 + its, team 2
  const int hid = blockIdx.x / per, r = blockIdx.x % per;
  const int team = r < G + 1 ? 0 : (r < G + 1 + G1 + 1 ? 1 : 2), wi = team == 2 ? r - (G + 1) - (G1 + 1) : (team ? r - (G + 1) : r);
  const bool diag = (team == 0 && wi == G) || (team == 1 && wi == G1);   // the front's diagonal workgroup
  const int cw = (team == 1 && !diag && wi >= G) ? wi - G : -1;           // separator-row workgroup
  unsigned* dflag = P.bars + (BAND_INFO_PUBLISHED - BAND_INFO_NESTED_BARS) + 2 * hid + (team == 1);
  long long t_escape; band_clock_init(&t_escape);
  const int w = cw < 0 ? wi : 0;
  const bool has_rhs = (cw < 0 && w == G - 1);
  const BandHalf H = P.h[hid];
  unsigned* bars = P.bars + 3 * hid;
  const int nh = H.nh, bw = P.bw, wc = P.wc;
  const int Trev = BS * H.K2, m_begin = BS * H.K1, m_end = nh - BS * H.K2;
  const double* zero = P.zero;
  const BandSeg none{H.fv, 0, 0, 0};
  const BandSegX nonex{{H.fv, 0, 0, 0}, 0, 0};
  const BandAug noaug{zero, 0, 0, 0, 0, nullptr, 0, 0, 0};
  // (the clock words are passed by address to the out-of-line step functions: with a caller-side object escaping, their calls
  // are not tail-call candidates and the functions keep the no-callee-saved-registers convention, see band_potf2_inv_k0)
  long long tp[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, t_prev = 0;
  long long* tpp = (P.prof && hid == 0 && team == 1 && (wi == 0 || wi == G1 - 1)) ? tp : nullptr;   // phase clock of a panel-row and a separator-row workgroup
  if (tpp) t_prev = wall_clock64();
  unsigned ep = 0;
  const bool stamp = P.prof && hid == 0 && team == 1 && wi == 0 && tid == 0;
#define BAND_STAMP(k) do { if (stamp) P.prof[k] = wall_clock64(); } while (0)
  BAND_STAMP(0);
  const int nslab = P.GS, GCC = P.GC;   // Schur slabs of 16 rows; workgroups of C's own factorisation
  if (diag) {
    if (team == 0) { band_diag_phase<1>(M, H.fv, H.Linv_f, 0, m_begin, false, H.rv, 0, nullptr, 0, bars + 0, (unsigned)G, 0, dflag, 0, nh, bw, zero, P.info); return; }
    band_diag_phase<1>(M, H.rv, H.Linv_r, 0, Trev, false, H.fv, 0, nullptr, 0, bars + 1, (unsigned)G1, 0, dflag, 0, nh, bw, zero, P.info, (P.prof && hid == 0) ? P.prof + 34 : nullptr);
    band_diag_phase<1>(M, H.fv, H.Linv_f, m_begin, m_end, true, H.rv, Trev, bars + 2, (unsigned)(G + G1), bars + 1, (unsigned)G1, (unsigned)H.K2, dflag, (unsigned)H.K2, nh, bw, zero, P.info);
    if (hid != 0) return;
    const BandView vcd{P.SC, 1, (long long)wc, P.rhsC, 1};
    const unsigned km = (unsigned)((m_end - m_begin + BS - 1) / BS);
    band_diag_phase<1>(M, vcd, P.LinvC, 0, wc, false, vcd, 0, P.bars + 8, (unsigned)GCC, P.bars + 8, (unsigned)GCC, 1, dflag, (unsigned)H.K2 + km, wc, wc - 1, zero, P.info);
    return;
  }
  if (team == 0) {
    for (int kb = 0; kb < H.K1; kb++) {
      const int k0 = kb * BS;
      const BandSeg s0{H.fv, max(0, k0 - bw), k0, 0};
      band_step<false, 1>(M, H.fv, H.Linv_f, k0, BS, min(nh, k0 + BS + bw), s0, none, 1, noaug, w, -1, has_rhs, nh, bw, zero, dflag, ep + 1, tpp, &t_prev);
      ep++;
      band_grid_sync(bars + 0, ep * (unsigned)G);
    }
    band_grid_arrive(bars + 2);
    return;
  }
  if (team == 2) {
    // Schur accumulator of C: 16 rows of sum_t L(i, t) L(j, t) and sum_t L(i, t) y(t) over everything team 1 eliminates,
    // one 32-column block behind it (waits on team 1's barrier counter without taking part in it)
    const int ldb = wc + 1, Th = nh - BS * H.K1, nstep = (Th + BS - 1) / BS;
    double* buf = R;                         // 32 x (wc + 1): rows of lc + the right-hand side entry
    const int tt8 = tid >> 3, l8 = tid & 7, lane = tid & 63, wv4 = tid >> 6, li = lane & 15, lk = lane >> 4;
    // the slab's 16 x wc block on the matrix cores: wave w takes the 16-column tiles w, w + 4, ... (wc <= 256: at most four), every
    // step is 8 x 16x16x4 issues per tile -- the multiply-add form read 17 LDS words per row of the step and per thread, and had
    // become the slowest team of the kernel once the fronts' hand-offs got cheaper
    ba_v4d acc[4];
#pragma unroll
    for (int q = 0; q < 4; q++) acc[q] = ba_v4d{0.0, 0.0, 0.0, 0.0};
    double accy = 0.0;                       // threads 0..15: the slab's share of sum_t L(i, t) y(t)
    for (int sidx = 0; sidx < nstep; sidx++) {
      if (tid == 0) {
        band_wait_ge(bars + 1, (unsigned)(sidx + 1) * (unsigned)G1);
        band_acquire();
      }
      __syncthreads();
      const int t = sidx * BS + tt8;
      const double* row = H.lc + (long long)t * wc + l8;
      double vals[32];
#pragma unroll
      for (int u = 0; u < 32; u++) vals[u] = band_gload((t < Th && 8 * u + l8 < wc) ? row + 8 * u : zero);
      const double yv = band_gload((t < Th && l8 == 0) ? band_half_y(H, t) : zero);
#pragma unroll
      for (int u = 0; u < 32; u++) if (8 * u < wc) buf[tt8 * ldb + l8 + 8 * u] = vals[u];
      if (l8 == 0) buf[tt8 * ldb + wc] = yv;
      __syncthreads();
#pragma unroll
      for (int t0 = 0; t0 < BS; t0 += 4) {
        const double* bt = buf + (t0 + lk) * ldb;
        const double a = bt[wi * 16 + li];
#pragma unroll
        for (int q = 0; q < 4; q++) {
          const int ct = wv4 + 4 * q;
          if (16 * ct < wc) acc[q] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, bt[16 * ct + li], acc[q], 0, 0, 0);
        }
      }
      if (tid < 16) {
#pragma unroll 8
        for (int tt = 0; tt < BS; tt++) accy = fma(buf[tt * ldb + wi * 16 + tid], buf[tt * ldb + wc], accy);
      }
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const int ct = wv4 + 4 * q;
      if (16 * ct >= wc) continue;
#pragma unroll
      for (int g = 0; g < 4; g++) band_gstore(&P.part[((size_t)hid * wc + wi * 16 + lk + 4 * g) * ldb + 16 * ct + li], acc[q][g]);
    }
    if (tid < 16) band_gstore(&P.part[((size_t)hid * wc + wi * 16 + tid) * ldb + wc], accy);
    band_grid_arrive(P.bars + 6);
    return;
  }
  // ---- team 1: the front next to C (reverse view of the half), C's rows below it
  {
    // A(q, u): entry (nh + q, nh - 1 - u) of the half's space, inside the band iff q + 1 + u <= bw
    const BandAug aug{H.fv.base + (long long)nh * H.fv.si + (long long)(nh - 1) * H.fv.sj, H.fv.si, -H.fv.sj, 1, 1, H.lc, wc, H.qflip, 0};
    for (int kb = 0; kb < H.K2; kb++) {
      const int k0 = kb * BS;
      const BandSegX s0{{H.rv, max(0, k0 - bw), k0, 0}, 0, 0};
      band_step<true, 1>(M, H.rv, H.Linv_r, k0, BS, min(nh, k0 + BS + bw), s0, nonex, 1, aug, w, cw, has_rhs, nh, bw, zero, dflag, ep + 1, tpp, &t_prev);
      ep++;
      band_grid_sync(bars + 1, ep * (unsigned)G1);
      if (tpp) { long long t_now = wall_clock64(); tp[5] += t_now - t_prev; t_prev = t_now; }
    }
  }
  if (tpp && tid == 0) for (int k = 0; k < 9; k++) P.prof[16 + (wi == 0 ? 0 : 9) + k] = tp[k];
  BAND_STAMP(1);
  band_grid_sync(bars + 2, (unsigned)(G + G1));
  BAND_STAMP(2);
  // ---- the half's middle block (its own space): history = tail of team 0's front + the block's earlier columns, and
  // the tail of the reverse front; C's rows: entry (nh + q, j), inside the band iff nh + q - j <= bw
  {
    const BandAug aug{H.fv.base + (long long)nh * H.fv.si, H.fv.si, H.fv.sj, nh, -1, H.lc, wc, H.qflip, Trev - m_begin};
    for (int k0 = m_begin; k0 < m_end; k0 += BS) {
      const int nb = min(BS, m_end - k0);
      const int i_end = min(m_end, k0 + nb + bw);
      const BandSegX s0{{H.fv, max(0, k0 - bw), k0, 0}, Trev - m_begin, m_begin};
      const BandSegX s1{{H.rv, max(0, (nh - i_end) - bw), Trev, 1}, 0, 0};
      band_step<true, 1>(M, H.fv, H.Linv_f, k0, nb, i_end, s0, s1, 2, aug, w, cw, has_rhs, nh, bw, zero, dflag, ep + 1, tpp, &t_prev);
      ep++;
      band_grid_sync(bars + 1, ep * (unsigned)G1);
    }
  }
  // ---- both halves (and their Schur accumulators, team 2) done
  BAND_STAMP(3);
  band_grid_sync(P.bars + 6, 2u * (unsigned)(G1 + nslab));
  BAND_STAMP(4);
  if (hid != 0 || wi >= GCC) return;
  // ---- the C team: Schur complement of its row slab (lower triangle; the first GS workgroups, 16 rows each), then the dense factorisation
  if (wi < nslab) {
    const int ldb = wc + 1, rr = tid >> 4, cg = tid & 15, i = wi * 16 + rr;
    for (int j = cg; j <= wc; j += 16) {
      const double s = band_gload(&P.part[(size_t)i * ldb + j]) + band_gload(&P.part[((size_t)wc + i) * ldb + j]);
      if (j < wc) {
        if (j <= i) band_gstore(&P.SC[(size_t)j * wc + i], ((i - j <= bw) ? band_gload(&P.Sb[(size_t)(P.c0 + j) * P.LD + (i - j)]) : 0.0) - s);
      } else {
        band_gstore(&P.rhsC[i], band_gload(&P.rhs[P.c0 + i]) - s);
      }
    }
  }
  unsigned epc = 1;
  band_grid_sync(P.bars + 8, epc * (unsigned)GCC);
  BAND_STAMP(7);
  const BandView vc{P.SC, 1, (long long)wc, P.rhsC, 1};
  for (int k0 = 0; k0 < wc; k0 += BS) {
    const BandSeg s0{vc, 0, k0, 0};
    band_step<false, 1>(M, vc, P.LinvC, k0, BS, wc, s0, none, 1, noaug, wi, -1, wi == GCC - 1, wc, wc - 1, zero, dflag, ep + epc, tpp, &t_prev);
    epc++;
    band_grid_sync(P.bars + 8, epc * (unsigned)GCC);
  }
  BAND_STAMP(8);
#undef BAND_STAMP
}

// L^T x = y in place in rhs, in the elimination order reversed: first the middle block (forward view), then the two
// fronts' regions independently -- workgroup 0 walks the forward front's blocks back to the top, workgroup 1 (it
// repeats the middle block for itself) the reverse front's blocks back to the bottom.  Per block: t = (rows below)^T x
// with x from an LDS window, x_k = L_kk^-T (y_k - t) with the inverted diagonal block.  Everything a step reads from
// memory (its panel of L, L_kk^-1, y_k) is independent of x and is fetched one step ahead, all loads unconditional.
// With the nested elimination the same runs per half (4 workgroups), after C's unknowns have been solved and their
// contribution taken out of the halves' right-hand sides (band_sep_solve_kernel, band_sep_correct_kernel).
enum { BAND_WIN = 8192, BAND_PF = 24 };      // x window (a step touches <= 32 + 4096 consecutive rows); prefetched rows per thread
struct BandSolveLds { double* xw; double* z; double (*Li)[BS + 1]; double (*part)[BS]; };
// blocks kb_hi .. kb_lo (descending) of `view`; rows of the view at or beyond row_limit do not exist
__device__ __forceinline__ void band_backsolve_run(const BandSolveLds& M, const BandView& view, const double* Linv, int kb_hi, int kb_lo, int row_limit, int bw, const double* zero) {
  constexpr int WIN = BAND_WIN, PF = BAND_PF;
  const int tid = threadIdx.x, c = tid & 31, g = tid >> 5;
  double lv[PF], li[4], yv = 0.0;
  auto prefetch = [&](int kb) {
    const int k0 = kb * BS, nb = min(BS, row_limit - k0), i_end = min(row_limit, k0 + nb + bw);
    const double* col = view.base + (long long)(k0 + c) * view.sj;     // &L(i, k0 + c) = col + i * si
#pragma unroll
    for (int s = 0; s < PF; s++) {
      const int i = k0 + nb + g + 8 * s;
      const bool ok = c < nb && i < i_end && i - (k0 + c) <= bw;
      lv[s] = *(ok ? col + (long long)i * view.si : zero);
    }
#pragma unroll
    for (int u = 0; u < 4; u++) li[u] = Linv[(size_t)kb * BS * BS + tid + 256 * u];
    yv = (tid < nb) ? view.rb[(long long)(k0 + tid) * view.sr] : 0.0;
  };
  if (kb_hi < kb_lo) return;
  prefetch(kb_hi);
  __syncthreads();
  for (int kb = kb_hi; kb >= kb_lo; kb--) {
    const int k0 = kb * BS, nb = min(BS, row_limit - k0);
    const int i_end = min(row_limit, k0 + nb + bw);
    double acc = 0;   // t[c] = sum over the rows below the block of L(i, k0 + c) x[i]; 8 row groups
#pragma unroll
    for (int s = 0; s < PF; s++) acc = fma(lv[s], M.xw[(k0 + nb + g + 8 * s) & (WIN - 1)], acc);
    if (c < nb)
      for (int i = k0 + nb + g + 8 * PF; i < i_end; i += 8)
        if (i - (k0 + c) <= bw) acc = fma(view.base[(long long)i * view.si + (long long)(k0 + c) * view.sj], M.xw[i & (WIN - 1)], acc);
    M.part[g][c] = acc;
#pragma unroll
    for (int u = 0; u < 4; u++) { int e = tid + 256 * u; M.Li[e >> 5][e & 31] = li[u]; }
    __syncthreads();
    if (tid < BS) {
      double tt = 0;
#pragma unroll
      for (int q = 0; q < 8; q++) tt += M.part[q][tid];
      M.z[tid] = (tid < nb) ? yv - tt : 0.0;
    }
    __syncthreads();
    if (kb > kb_lo) prefetch(kb - 1);
    if (tid < nb) {
      double a2 = 0;
#pragma unroll 8
      for (int r = 0; r < BS; r++) a2 = fma(M.Li[r][tid], M.z[r], a2);   // (L^-1)^T z
      band_pstore(&view.rb[(long long)(k0 + tid) * view.sr], a2);
      M.xw[(k0 + tid) & (WIN - 1)] = a2;
    }
    __syncthreads();
  }
}
struct BandSolve { BandHalf h[2]; int bw; const double* zero; };   // one half (the whole matrix) or two
__global__ __launch_bounds__(256) void band_backsolve_kernel(BandSolve P) {
  __shared__ double xw[BAND_WIN];
  __shared__ double z[BS];
  __shared__ double Li[BS][BS + 1];
  __shared__ double part[8][BS];
  const BandSolveLds M{xw, z, Li, part};
  const int tid = threadIdx.x;
  const BandHalf H = P.h[blockIdx.x >> 1];
  const int bw = P.bw, nh = H.nh, m_end = nh - BS * H.K2;
  for (int e = tid; e < BAND_WIN; e += 256) xw[e] = 0.0;
  // the middle block (the half's own view; rows end at m_end)
  band_backsolve_run(M, H.fv, H.Linv_f, (m_end - 1) / BS, H.K1, m_end, bw, P.zero);
  if ((blockIdx.x & 1) == 0) {
    band_backsolve_run(M, H.fv, H.Linv_f, H.K1 - 1, 0, nh, bw, P.zero);
  } else {
    // the same unknowns seen from the reverse front: x of the middle block into the window at its reverse indices
    __syncthreads();
    for (int e = tid; e < BAND_WIN; e += 256) xw[e] = 0.0;
    __syncthreads();
    for (int v = BS * H.K2 + tid; v < min(nh, BS * H.K2 + bw + BS); v += 256) xw[v & (BAND_WIN - 1)] = H.rv.rb[(long long)v * H.rv.sr];
    __syncthreads();
    band_backsolve_run(M, H.rv, H.Linv_r, H.K2 - 1, 0, nh, bw, P.zero);
  }
}
// C's unknowns: L_C^T x_C = y_C on the dense block (one workgroup)
__global__ __launch_bounds__(256) void band_sep_solve_kernel(BandNested P) {
  __shared__ double xw[BAND_WIN];
  __shared__ double z[BS];
  __shared__ double Li[BS][BS + 1];
  __shared__ double part[8][BS];
  const BandSolveLds M{xw, z, Li, part};
  for (int e = threadIdx.x; e < BAND_WIN; e += 256) xw[e] = 0.0;
  const BandView vc{P.SC, 1, (long long)P.wc, P.rhsC, 1};
  band_backsolve_run(M, vc, P.LinvC, P.wc / BS - 1, 0, P.wc, P.wc - 1, P.zero);
}
// y(t) -= sum_q L(q, t) x_C(q) for every elimination column t that carries C's rows (32 per workgroup, 8 lanes each);
// workgroup 0 also stores x_C at C's place in the solution vector
__global__ __launch_bounds__(256) void band_sep_correct_kernel(BandNested P) {
  __shared__ double xc[256];
  const int tid = threadIdx.x, wc = P.wc;
  for (int e = tid; e < wc; e += 256) xc[e] = P.rhsC[e];
  __syncthreads();
  if (blockIdx.x == 0) for (int e = tid; e < wc; e += 256) band_pstore(&P.rhs[P.c0 + e], xc[e]);
  const int T0 = P.h[0].nh - BS * P.h[0].K1, T1 = P.h[1].nh - BS * P.h[1].K1;
  const int t = blockIdx.x * 32 + (tid >> 3), l8 = tid & 7;
  double s = 0.0;
  if (t < T0 + T1) {
    const BandHalf& H = P.h[t < T0 ? 0 : 1];
    const double* row = H.lc + (long long)(t < T0 ? t : t - T0) * wc;
    for (int q = l8; q < wc; q += 8) s = fma(row[q], xc[q], s);
  }
  s += __shfl_xor(s, 1); s += __shfl_xor(s, 2); s += __shfl_xor(s, 4);
  if (t < T0 + T1 && l8 == 0) {
    const double* y = band_half_y(P.h[t < T0 ? 0 : 1], t < T0 ? t : t - T0);
    band_pstore(y, *y - s);
  }
}

int ba_band_team(int LD, int* rw_out) {   // workgroups of the factorisation team and their rows per step
  const int bw = LD - 1;
  int G = (bw + BAND_RW - 1) / BAND_RW;
  if (G < 1) G = 1;
  *rw_out = BAND_RW;
  return G;
}

static void ba_band_split(int n, int LD, int* K1, int* K2, bool force_one_sided = false) {   // column blocks of the two fronts; the middle block keeps >= bw columns
  const int bw = LD - 1;
  const int Kt = n > bw ? (n - bw) / BS : 0;
  static const bool one_sided = getenv("CS_BAND_ONE_SIDED") != nullptr;   // diagnostics: plain left-looking order
  *K2 = (Kt >= 8 && !one_sided && !force_one_sided) ? Kt / 2 : 0;
  *K1 = Kt - *K2;
}
// The nested (four-front) order pays when both halves still have two real fronts; it needs the separator's row
// workgroups co-resident with the four teams, which bounds the bandwidth it is used for.
static bool ba_band_nested(int n, int LD, int* wc_out, int* c0_out, bool force_one_sided = false) {
  if (force_one_sided) return false;
  static const bool off = getenv("CS_BAND_TWO_FRONTS") != nullptr || getenv("CS_BAND_ONE_SIDED") != nullptr;   // diagnostics: the two-front order
  const int bw = LD - 1;
  const int wc = ((bw + BS - 1) / BS) * BS;
  const int nh = (n - wc) / 2;
  if (off || bw > 256 || bw < 1 || nh < bw + 16 * BS) return false;
  *wc_out = wc; *c0_out = nh;
  return true;
}
static size_t band_blocks(int n) { return (size_t)((n + BS - 1) / BS) * BS * BS; }
// doubles of workspace behind `work` (inverted diagonal blocks; nested order: + the separator's factor rows, partial
// Schur complements and dense block)
size_t ba_band_workspace_doubles(int n, int LD) {
  if (n <= 0) return 1;
  size_t two = 2 * band_blocks(n);
  int wc = 0, c0 = 0;
  if (!ba_band_nested(n, LD, &wc, &c0)) return two;
  const int nh0 = c0, nh1 = n - c0 - wc;
  size_t nest = 2 * band_blocks(nh0) + 2 * band_blocks(nh1) + band_blocks(wc) + (size_t)(nh0 + nh1) * wc + (size_t)2 * wc * (wc + 1) + (size_t)wc * wc + wc;
  return nest > two ? nest : two;
}

// Does the persistent factorisation of an n x n band with LD = bandwidth + 1 fit the current device?  Its workgroups wait for
// each other, so the whole grid must be resident at once: the grid may not exceed (workgroups the occupancy query admits per
// CU, capped at 1: the kernels are written for one workgroup per CU) x (CUs of the device or partition).  The caller takes the
// dense rocSOLVER path otherwise.
bool ba_band_fits_device(int n, int LD, bool one_sided) {   // one_sided: the order ba_launch_band_cholesky(..., one_sided = true) runs (the sharded solve's interiors)
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return false;
  int rw = 0, K1 = 0, K2 = 0, wc = 0, c0 = 0, occ = 0, grid = 0;
  const int G = ba_band_team(LD, &rw), bw = LD - 1;
  if (ba_band_nested(n, LD, &wc, &c0, one_sided)) {
    const int Gn = (bw + BAND_RW_NESTED - 1) / BAND_RW_NESTED, GC = wc / BAND_RW_NESTED, GS = wc / 16;
    grid = 2 * (Gn + 1 + Gn + GC + 1 + GS);
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, band_chol_nested_kernel, 256, 0) != hipSuccess) return false;
  } else {
    ba_band_split(n, LD, &K1, &K2, one_sided);
    grid = K2 > 0 ? 2 * (G + 1) : G + 1;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, band_chol_coop_kernel, 256, 0) != hipSuccess) return false;
  }
  return occ >= 1 && grid <= prop.multiProcessorCount;
}

// ---- CS_BAND_PROF diagnostics: the persistent kernels' phase clocks, read back behind the launch (which synchronises the stream) and
// printed for the first three launches of each order.  Without the variable the clock buffers stay nullptr and the kernels skip them.
static bool band_prof_wanted() { static const bool want = getenv("CS_BAND_PROF") != nullptr; return want; }
static long long* band_nested_prof_begin(hipStream_t st) {   // 40 words; the diagonal workgroup's six accumulate, so they are cleared per launch
  static long long* stamps = nullptr;
  if (band_prof_wanted() && !stamps) (void)hipMalloc(&stamps, 40 * sizeof(long long));
  if (stamps) (void)hipMemsetAsync(stamps + 34, 0, 6 * sizeof(long long), st);
  return stamps;
}
static void band_nested_prof_report(const BandNested& P, hipStream_t st) {
  if (!P.prof) return;
  long long h[40];
  (void)hipMemcpyAsync(h, P.prof, sizeof(h), hipMemcpyDeviceToHost, st);
  (void)hipStreamSynchronize(st);
  static int shown = 0;
  if (shown++ >= 3) return;
  fprintf(stderr, "[band nested] n=%d bw=%d C=%d+%d halves %d/%d fronts %d+%d / %d+%d us: reverse front %.0f  join wait %.0f  middle %.0f  halves wait %.0f  C build %.0f  C factor %.0f\n",
          P.n, P.bw, P.c0, P.wc, P.h[0].nh, P.h[1].nh, P.h[0].K1, P.h[0].K2, P.h[1].K1, P.h[1].K2, (h[1] - h[0]) * 0.01, (h[2] - h[1]) * 0.01, (h[3] - h[2]) * 0.01, (h[4] - h[3]) * 0.01,
          (h[7] - h[4]) * 0.01, (h[8] - h[7]) * 0.01);
  for (int q = 0; q < 2; q++)
    fprintf(stderr, "[band nested] reverse front, %s workgroup us: fetch-issue %.0f  store+wait %.0f  gemm %.0f  reduce+U %.0f  wait for L^-1 %.0f  panel %.0f  barrier %.0f\n", q ? "separator-row" : "panel-row",
            h[16 + 9 * q + 6] * 0.01, h[16 + 9 * q + 7] * 0.01, h[16 + 9 * q + 8] * 0.01, h[16 + 9 * q + 1] * 0.01, h[16 + 9 * q + 2] * 0.01, h[16 + 9 * q + 4] * 0.01, h[16 + 9 * q + 5] * 0.01);
  fprintf(stderr, "[band nested] reverse front, diagonal workgroup us: wait for the team's barrier %.0f  newest block + U %.0f  POTF2 + inverse %.0f  publish %.0f  look-ahead accumulation %.0f\n",
          h[34] * 0.01, h[35] * 0.01, h[36] * 0.01, h[37] * 0.01, h[38] * 0.01);
}
static long long* band_coop_prof_begin() {   // 20 words: phase clock of the forward team's first / last workgroup
  static long long* prof = nullptr;
  if (band_prof_wanted() && !prof) (void)hipMalloc(&prof, 20 * sizeof(long long));
  return prof;
}
static void band_coop_prof_report(const long long* prof, int n, int LD, int G, int K1, int K2, hipStream_t st) {
  if (!prof) return;
  long long h[20];
  (void)hipMemcpyAsync(h, prof, sizeof(h), hipMemcpyDeviceToHost, st);
  (void)hipStreamSynchronize(st);
  static int shown = 0;
  if (shown++ >= 3) return;
  fprintf(stderr, "[band] shader clock %.0f MHz over %.0f us; fronts %d + %d blocks, middle %d columns\n", h[18] / (h[19] * 0.01), h[19] * 0.01, K1, K2, n - BS * (K1 + K2));
  for (int q = 0; q < 2; q++)
    fprintf(stderr, "[band] n=%d LD=%d G=%d wg%s us: fetch-issue %.0f  store+wait %.0f  gemm %.0f  reduce+U %.0f  potf2+inverse %.0f  panel %.0f  barrier %.0f\n", n, LD, G, q ? "last" : "0",
            h[9 * q + 6] * 0.01, h[9 * q + 7] * 0.01, h[9 * q + 8] * 0.01, h[9 * q + 1] * 0.01, h[9 * q + 2] * 0.01, h[9 * q + 4] * 0.01, h[9 * q + 5] * 0.01);
}

// (arguments: band_solver.h)
void ba_launch_band_cholesky(double* Sb, double* work, int n, int LD, double* rhs, int* info, bool solve, hipStream_t st, bool one_sided) {
  int rw = 0, K1 = 0, K2 = 0, wc = 0, c0 = 0;
  const int G = ba_band_team(LD, &rw);
  const int bw = LD - 1;
  const double* zero = reinterpret_cast<const double*>(info + BAND_INFO_ZERO);
  const BandView fwd{Sb, 1, (long long)bw, rhs, 1};
  const BandView rev{Sb + (size_t)(n - 1) * LD, -(long long)bw, -1, rhs + (n - 1), -1};
  if (ba_band_nested(n, LD, &wc, &c0, one_sided)) {
    BandNested P;
    const int c1 = c0 + wc, nh[2] = {c0, n - c1};
    double* wp = work;
    for (int h = 0; h < 2; h++) {
      BandHalf& H = P.h[h];
      H.nh = nh[h];
      ba_band_split(nh[h], LD, &H.K1, &H.K2);
      H.qflip = h;
      H.Linv_f = wp; wp += band_blocks(nh[h]);
      H.Linv_r = wp; wp += band_blocks(nh[h]);
    }
    // left half: the matrix's own index space, reverse front from c0 - 1 down; right half: the mirrored space, its
    // reverse front therefore walks forward from c1
    P.h[0].fv = fwd;
    P.h[0].rv = BandView{Sb + (size_t)(c0 - 1) * LD, -(long long)bw, -1, rhs + (c0 - 1), -1};
    P.h[1].fv = rev;
    P.h[1].rv = BandView{Sb + (size_t)c1 * LD, 1, (long long)bw, rhs + c1, 1};
    P.LinvC = wp; wp += band_blocks(wc);
    for (int h = 0; h < 2; h++) { P.h[h].lc = wp; wp += (size_t)nh[h] * wc; }
    P.part = wp; wp += (size_t)2 * wc * (wc + 1);
    P.SC = wp; wp += (size_t)wc * wc;
    P.rhsC = wp; wp += wc;
    P.n = n; P.bw = bw; P.wc = wc; P.c0 = c0; P.LD = LD; P.G = (bw + BAND_RW_NESTED - 1) / BAND_RW_NESTED; P.GC = wc / BAND_RW_NESTED; P.GS = wc / 16;
    const int G1 = P.G + P.GC;
    P.Sb = Sb; P.rhs = rhs; P.zero = zero; P.info = info; P.bars = reinterpret_cast<unsigned*>(info + BAND_INFO_NESTED_BARS);
    P.prof = band_nested_prof_begin(st);
    hipLaunchKernelGGL(band_chol_nested_kernel, dim3(2 * (P.G + 1 + G1 + 1 + P.GS)), dim3(256), 0, st, P);
    band_nested_prof_report(P, st);
    if (solve) {
      const int TT = (nh[0] - BS * P.h[0].K1) + (nh[1] - BS * P.h[1].K1);
      hipLaunchKernelGGL(band_sep_solve_kernel, dim3(1), dim3(256), 0, st, P);
      hipLaunchKernelGGL(band_sep_correct_kernel, dim3((TT + 31) / 32), dim3(256), 0, st, P);
      BandSolve Q; Q.h[0] = P.h[0]; Q.h[1] = P.h[1]; Q.bw = bw; Q.zero = zero;
      hipLaunchKernelGGL(band_backsolve_kernel, dim3(4), dim3(256), 0, st, Q);
    }
    return;
  }
  ba_band_split(n, LD, &K1, &K2, one_sided);
  unsigned* bars = reinterpret_cast<unsigned*>(info + BAND_INFO_BARS);
  double* Linv_f = work;
  double* Linv_r = work + band_blocks(n);
  long long* prof = band_coop_prof_begin();
  hipLaunchKernelGGL(band_chol_coop_kernel, dim3(K2 > 0 ? 2 * (G + 1) : G + 1), dim3(256), 0, st, Sb, Linv_f, Linv_r, rhs, zero, n, LD, K1, K2, info, bars, G, prof);
  band_coop_prof_report(prof, n, LD, G, K1, K2, st);
  if (solve) {
    BandSolve Q;
    Q.h[0] = BandHalf{fwd, rev, n, K1, K2, 0, Linv_f, Linv_r, nullptr}; Q.h[1] = Q.h[0]; Q.bw = bw; Q.zero = zero;
    hipLaunchKernelGGL(band_backsolve_kernel, dim3(K2 > 0 ? 2 : 1), dim3(256), 0, st, Q);
  }
}


// ------------------------------------------------------------- sharded reduced solve: interiors and separators --
// Sharded BA (ba_host.cpp, "separator mode"): rank r owns the columns [cut_r, cut_r+1) of the band; its first w >= bw columns are the
// separator Z_r (none on rank 0), the rest its interior I_r.  Interiors of different ranks are further apart than the bandwidth, so
// they are decoupled; an interior is coupled to the separator in front of it (Z_r, "left") and to the one behind it (Z_r+1, the next
// rank's, "right").  Per damped solve a rank factorises ITS interior only (band_chol_coop_kernel, one-sided order, right-hand side
// riding along), and forms what the separators need of it:
//     Y = B L^-T   (rows: the unknowns of Z_r and Z_r+1, columns: the interior)      ba_sep_trsm_kernel
//     T = C - Y Y^T,   t = b_Z - Y y                                                  ba_sep_schur_kernel, ba_sep_rhs_kernel
// with C the rank's own partial blocks S(Z_r, Z_r), S(Z_r+1, Z_r+1).  The ranks exchange (T, t) -- three w x w blocks and two
// w-vectors each, the only matrix data that crosses the links --, every rank assembles and solves the small block-tridiagonal
// separator system, then x_I = L^-T (y - Y^T x_Z) (ba_sep_correct_kernel + band_backsolve_kernel).
struct SepView {
  const double* S; int LD;          // the band (lower, LD doubles per column), the interior's factor in place
  const double* Linv;               // inverted diagonal blocks of the interior's factor (32 x 32 each, row-major)
  int ci, ni;                       // interior = columns [ci, ci + ni)
  int zl, wl, zr, wr;               // left separator [zl, zl + wl), right separator [zr, zr + wr); widths may be 0
  double* Y;                        // (wl + wr) x ni, row-major
  const double* rhs;                // the global right-hand side / solution vector (y of the interior at rhs + ci)
};
// A(q, j): coupling of separator row q (0 .. wl - 1 left, wl .. wl + wr - 1 right) with interior column j
__device__ __forceinline__ double sep_coupling(const SepView& V, int q, int j) {
  const int bw = V.LD - 1;
  if (q < V.wl) {           // S(row ci + j, col zl + q): stored in the separator's column
    const int d = (V.ci + j) - (V.zl + q);
    return d <= bw ? V.S[(size_t)(V.zl + q) * V.LD + d] : 0.0;
  }
  const int d = (V.zr + (q - V.wl)) - (V.ci + j);     // S(row zr + q', col ci + j): stored in the interior's column, below the interior
  return d <= bw ? V.S[(size_t)(V.ci + j) * V.LD + d] : 0.0;
}
enum { SEP_RW = 8 };
// One workgroup per SEP_RW separator rows, walking the interior's column blocks in order (the rows are independent of each other:
// no grid barrier).  Thread (rq, c): row rq of the group, column c of the block.
__global__ __launch_bounds__(256) void ba_sep_trsm_kernel(SepView V) {
  __shared__ double Lc[BS][BS + 1];      // Lc[c'][d] = L(k0 + c', s0 + d)
  __shared__ double Yc[SEP_RW][BS + 1];  // Yc[rq][d] = Y(q, s0 + d); afterwards U
  __shared__ double Li[BS][BS + 1];
  const int tid = threadIdx.x, c = tid & 31, rq = tid >> 5;
  const int nq = V.wl + V.wr, q = blockIdx.x * SEP_RW + rq, bw = V.LD - 1;
  const bool qok = q < nq;
  const double* Sint = V.S + (size_t)V.ci * V.LD;      // &L(i, j) = Sint + j LD + (i - j)
  // rows of the right separator are zero up to the first interior column inside their band
  int first = 0;
  {
    const int q_lo = blockIdx.x * SEP_RW;              // the group's first row decides (left rows: column 0)
    if (q_lo >= V.wl) first = max(0, (V.zr + (q_lo - V.wl)) - bw - V.ci) / BS;
  }
  double* Yrow = V.Y + (size_t)(qok ? q : 0) * V.ni;
  for (int j = tid; j < first * BS; j += 256)
    for (int r = 0; r < SEP_RW; r++) if (blockIdx.x * SEP_RW + r < nq) V.Y[(size_t)(blockIdx.x * SEP_RW + r) * V.ni + j] = 0.0;
  const int nblk = (V.ni + BS - 1) / BS;
  for (int kb = first; kb < nblk; kb++) {
    const int k0 = kb * BS, nb = min(BS, V.ni - k0);
    double acc = 0.0;
    const int jlo = max(first * BS, max(0, k0 - bw) & ~(BS - 1));
    for (int s0 = jlo; s0 < k0; s0 += BS) {
      // L(k0 + c', s0 + d): thread loads c' = c, d = rq + 8 u (consecutive c' are consecutive addresses)
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int d = rq + 8 * u, i = k0 + c, j = s0 + d;
        Lc[c][d] = (c < nb && i - j <= bw) ? Sint[(size_t)j * V.LD + (i - j)] : 0.0;
      }
      Yc[rq][c] = qok ? Yrow[s0 + c] : 0.0;
      __syncthreads();
#pragma unroll 8
      for (int d = 0; d < BS; d++) acc = fma(Yc[rq][d], Lc[c][d], acc);
      __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 4; u++) { const int e = tid + 256 * u; Li[e >> 5][e & 31] = V.Linv[(size_t)kb * BS * BS + e]; }
    Yc[rq][c] = (qok && c < nb) ? sep_coupling(V, q, k0 + c) - acc : 0.0;     // U
    __syncthreads();
    double y = 0.0;
    for (int cc = 0; cc <= c; cc++) y = fma(Yc[rq][cc], Li[c][cc], y);        // U L_kk^-T
    if (qok && c < nb) Yrow[k0 + c] = y;
    __syncthreads();   // (also orders this block's stores before the next block's loads of them)
  }
}
// T = C - Y Y^T on the index pairs a >= b of the combined separator index (left rows first): one 16 x 16 tile per workgroup.
// msg = [LL | RL | RR | tL | tR] with blocks of wm x wm (row-major, wm = the widest separator of the job) and vectors of wm.
__global__ __launch_bounds__(256) void ba_sep_schur_kernel(SepView V, double* msg, int wm) {
  __shared__ double Ya[16][BS + 1], Yb[16][BS + 1];
  const int nq = V.wl + V.wr, nt = (nq + 15) / 16;
  // tile (ta, tb), ta >= tb, from the linear block index
  int ta = 0, rem = blockIdx.x;
  while (rem > ta) { rem -= ta + 1; ta++; }
  const int tb = rem;
  if (ta >= nt) return;
  const int tid = threadIdx.x, la = tid >> 4, lb = tid & 15;
  const int a = ta * 16 + la, b = tb * 16 + lb;
  double acc = 0.0;
  for (int j0 = 0; j0 < V.ni; j0 += BS) {
    for (int e = tid; e < 16 * BS; e += 256) {
      const int r = e >> 5, d = e & 31, j = j0 + d;
      Ya[r][d] = (ta * 16 + r < nq && j < V.ni) ? V.Y[(size_t)(ta * 16 + r) * V.ni + j] : 0.0;
      Yb[r][d] = (tb * 16 + r < nq && j < V.ni) ? V.Y[(size_t)(tb * 16 + r) * V.ni + j] : 0.0;
    }
    __syncthreads();
#pragma unroll 8
    for (int d = 0; d < BS; d++) acc = fma(Ya[la][d], Yb[lb][d], acc);
    __syncthreads();
  }
  if (a >= nq || b >= nq || a < b) return;
  const int bw = V.LD - 1;
  const bool ar = a >= V.wl, br = b >= V.wl;
  double cval = 0.0;
  if (ar == br) {         // both in one separator: the rank's own partial block of S
    const int z = ar ? V.zr : V.zl, ia = ar ? a - V.wl : a, ib = br ? b - V.wl : b;
    if (ia - ib <= bw) cval = V.S[(size_t)(z + ib) * V.LD + (ia - ib)];
  }
  double* dst = (!ar) ? msg + (size_t)a * wm + b                                   // LL
              : (!br) ? msg + (size_t)wm * wm + (size_t)(a - V.wl) * wm + b        // RL (row: right, column: left)
                      : msg + 2 * (size_t)wm * wm + (size_t)(a - V.wl) * wm + (b - V.wl);   // RR
  *dst = cval - acc;
}
// t = b_Z - Y y: one wavefront per separator row
__global__ __launch_bounds__(64) void ba_sep_rhs_kernel(SepView V, double* msg, int wm) {
  const int q = blockIdx.x, lane = threadIdx.x;
  if (q >= V.wl + V.wr) return;
  double s = 0.0;
  for (int j = lane; j < V.ni; j += 64) s = fma(V.Y[(size_t)q * V.ni + j], V.rhs[V.ci + j], s);
  s = wave_sum(s);
  if (lane == 0) {
    const bool right = q >= V.wl;
    const int g = right ? V.zr + (q - V.wl) : V.zl + q;
    msg[3 * (size_t)wm * wm + (right ? wm + (q - V.wl) : q)] = V.rhs[g] - s;
  }
}
// The separator system from the ranks' messages.  Separator k (k = 1 .. R - 1, rows sep_off[k] .. sep_off[k + 1] of the system) is
// the left separator of rank k and the right separator of rank k - 1: its diagonal block is LL of rank k + RR of rank k - 1, its
// right-hand side tL of rank k + tR of rank k - 1; the block (Z_k+1, Z_k) is RL of rank k, whose interior lies between the two.
// Lower band, LDs = 2 * wm doubles per column (a block-tridiagonal matrix with blocks <= wm wide has bandwidth < 2 wm): element
// (r, c), r >= c, at Ssep[c * LDs + (r - c)] -- the layout band_chol_*_kernel factorises.
__global__ __launch_bounds__(256) void ba_sep_assemble_kernel(const double* msgs, size_t msg_doubles, int wm, int R, const int* sep_off, int n, int LDs, double* Ssep, double* rsep) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)n * (LDs + 1)) return;
  const int c = (int)(e / (LDs + 1)), dd = (int)(e % (LDs + 1));
  if (dd == LDs) {   // right-hand side of row c: tL of rank k + tR of rank k - 1
    int k = 1;
    while (k + 1 < R && sep_off[k + 1] <= c) k++;
    const int l = c - sep_off[k];
    rsep[c] = msgs[(size_t)k * msg_doubles + 3 * (size_t)wm * wm + l] + msgs[(size_t)(k - 1) * msg_doubles + 3 * (size_t)wm * wm + wm + l];
    return;
  }
  const int r = c + dd;
  double v = 0.0;
  if (r < n) {
    int kr = 1, kc = 1;
    while (kr + 1 < R && sep_off[kr + 1] <= r) kr++;
    while (kc + 1 < R && sep_off[kc + 1] <= c) kc++;
    const int lr = r - sep_off[kr], lc = c - sep_off[kc];
    if (kr == kc) v = msgs[(size_t)kr * msg_doubles + (size_t)lr * wm + lc] + msgs[(size_t)(kr - 1) * msg_doubles + 2 * (size_t)wm * wm + (size_t)lr * wm + lc];
    else if (kr == kc + 1) v = msgs[(size_t)kc * msg_doubles + (size_t)wm * wm + (size_t)lr * wm + lc];
  }
  Ssep[(size_t)c * LDs + dd] = v;
}
// x of the separators to their places in the solution vector (sep_col[k]: first column of Z_k)
__global__ __launch_bounds__(256) void ba_sep_scatter_kernel(const double* xsep, int n, int R, const int* sep_off, const int* sep_col, double* x) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  int k = 1;
  while (k + 1 < R && sep_off[k + 1] <= r) k++;
  x[sep_col[k] + (r - sep_off[k])] = xsep[r];
}
// y_I -= Y^T x_Z
__global__ __launch_bounds__(256) void ba_sep_correct_kernel(SepView V, double* y) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= V.ni) return;
  double s = 0.0;
  for (int q = 0; q < V.wl; q++) s = fma(V.Y[(size_t)q * V.ni + j], V.rhs[V.zl + q], s);
  for (int q = 0; q < V.wr; q++) s = fma(V.Y[(size_t)(V.wl + q) * V.ni + j], V.rhs[V.zr + q], s);
  y[V.ci + j] -= s;
}

void ba_launch_sep_reduce(const double* S, int LD, const double* Linv, int ci, int ni, int zl, int wl, int zr, int wr, double* Y, const double* rhs, double* msg, int wm, hipStream_t st) {
  const SepView V{S, LD, Linv, ci, ni, zl, wl, zr, wr, Y, rhs};
  const int nq = wl + wr;
  if (nq <= 0) return;
  hipLaunchKernelGGL(ba_sep_trsm_kernel, dim3((nq + SEP_RW - 1) / SEP_RW), dim3(256), 0, st, V);
  const int nt = (nq + 15) / 16;
  hipLaunchKernelGGL(ba_sep_schur_kernel, dim3(nt * (nt + 1) / 2), dim3(256), 0, st, V, msg, wm);
  hipLaunchKernelGGL(ba_sep_rhs_kernel, dim3(nq), dim3(64), 0, st, V, msg, wm);
}
void ba_launch_sep_assemble(const double* msgs, size_t msg_doubles, int wm, int R, const int* sep_off, int n, int LDs, double* Ssep, double* rsep, hipStream_t st) {
  const long long total = (long long)n * (LDs + 1);
  if (total > 0) hipLaunchKernelGGL(ba_sep_assemble_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, msgs, msg_doubles, wm, R, sep_off, n, LDs, Ssep, rsep);
}
void ba_launch_sep_scatter(const double* xsep, int n, int R, const int* sep_off, const int* sep_col, double* x, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(ba_sep_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, st, xsep, n, R, sep_off, sep_col, x);
}
// x_I = L^-T (y - Y^T x_Z): the correction, then the interior's back-substitution (one-sided order: one workgroup)
void ba_launch_sep_backsolve(double* S, int LD, double* work, int ci, int ni, int zl, int wl, int zr, int wr, double* Y, double* rhs, int* info, hipStream_t st) {
  if (ni <= 0) return;
  const SepView V{S, LD, work, ci, ni, zl, wl, zr, wr, Y, rhs};
  if (wl + wr > 0) hipLaunchKernelGGL(ba_sep_correct_kernel, dim3((ni + 255) / 256), dim3(256), 0, st, V, rhs);
  int K1 = 0, K2 = 0;
  ba_band_split(ni, LD, &K1, &K2, true);
  const int bw = LD - 1;
  double* Sb = S + (size_t)ci * LD;
  const BandView fwd{Sb, 1, (long long)bw, rhs + ci, 1};
  const BandView rev{Sb + (size_t)(ni - 1) * LD, -(long long)bw, -1, rhs + ci + (ni - 1), -1};
  BandSolve Q;
  Q.h[0] = BandHalf{fwd, rev, ni, K1, K2, 0, work, work + band_blocks(ni), nullptr}; Q.h[1] = Q.h[0]; Q.bw = bw; Q.zero = reinterpret_cast<const double*>(info + BAND_INFO_ZERO);
  hipLaunchKernelGGL(band_backsolve_kernel, dim3(1), dim3(256), 0, st, Q);
}

}  // namespace cs
