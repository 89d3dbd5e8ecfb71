// band_solver.h -- what a host hands to band_kernels.hip (the persistent banded Cholesky; the sharded solve's interiors and separators)
// and bcr_kernels.hip (block cyclic reduction): raw device pointers to the reduced system in lower band storage (element (r, c), r >= c,
// at S[c * LD + (r - c)], LD = bandwidth + 1), a workspace the host sizes with the *_workspace_doubles functions, and the status words.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

namespace cs {

// The status words of a solve: BAND_INFO_WORDS ints in one 256-byte-aligned block, zeroed by the caller before every launch
// (ba_trial_prologue_kernel on the BA's trial path).  The host reads BAND_INFO_STATUS only: 0 = fine, k + 1 = the first non-positive
// pivot's column, BAND_TIMEOUT_INFO = a wait of the persistent kernel timed out (band_wait_ge).
enum {
  BAND_INFO_STATUS = 0,        // [0]       pivot / time-out word
  BAND_INFO_BARS = 1,          // [1..3]    barrier counters of the two-front order (forward team, reverse team, both)
  BAND_INFO_ZERO = 4,          // [4..5]    a zero double (the target of masked loads)
  BAND_INFO_NESTED_BARS = 6,   // [6..14]   barrier counters of the nested order
  BAND_INFO_PUBLISHED = 15,    // [15..18]  published-block counters of the fronts' diagonal workgroups
  BAND_ABORT_SLOT = 19,        // [19]      abort word: raised by the waiter that timed out, ends every later wait of the launch
  BAND_INFO_WORDS = 24,
  BAND_TIMEOUT_INFO = 0x7fffffff
};

// ---- band_kernels.hip
// work: ba_band_workspace_doubles(n, LD) doubles.  one_sided: the plain left-looking order (the factor then lies in the band in the
// matrix's own index space: what the sharded solve's interior elimination needs, ba_launch_sep_*)
void ba_launch_band_cholesky(double* Sb, double* work, int n, int LD, double* rhs, int* info, bool solve, hipStream_t st, bool one_sided = false);
size_t ba_band_workspace_doubles(int n, int LD);
int ba_band_team(int LD, int* rw_out);
bool ba_band_fits_device(int n, int LD, bool one_sided = false);
void ba_launch_sep_reduce(const double* S, int LD, const double* Linv, int ci, int ni, int zl, int wl, int zr, int wr, double* Y, const double* rhs, double* msg, int wm, hipStream_t st);
void ba_launch_sep_assemble(const double* msgs, size_t msg_doubles, int wm, int R, const int* sep_off, int n, int LDs, double* Ssep, double* rsep, hipStream_t st);
void ba_launch_sep_scatter(const double* xsep, int n, int R, const int* sep_off, const int* sep_col, double* x, hipStream_t st);
void ba_launch_sep_backsolve(double* S, int LD, double* work, int ci, int ni, int zl, int wl, int zr, int wr, double* Y, double* rhs, int* info, hipStream_t st);
// ---- bcr_kernels.hip
bool ba_bcr_ok(int n, int LD);
double ba_bcr_estimate_ms(int n);
size_t ba_bcr_workspace_doubles(int n, int Bv);
void ba_launch_bcr(const double* Sb, double* work, int n, int LD, int Bv, double* rhs, int* info, hipStream_t st);
bool ba_bcr_sep_ok(int wm, int R);
size_t ba_bcr_sep_workspace_doubles(int R);
void ba_launch_bcr_sep(const double* msgs, size_t msg_doubles, int wm, int R, const int* sep_off, const int* sep_col, int ns, double* work, double* x, int* info, hipStream_t st);

}  // namespace cs
