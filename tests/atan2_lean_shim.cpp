// atan2_lean_shim.cpp -- TEST INFRASTRUCTURE (tests/atan2_lean_cases.py builds and loads it): cs_atan2_lean next to cs_atan2 on
// the host.  Both consist of IEEE-exact operations only, so what holds here holds on the device.
#include <cstdint>
#include "../cube_slam_wu_amd/csrc/cs_atan2_lean.h"

namespace {
bool same_bits(double a, double b) {
  uint64_t ua, ub;
  __builtin_memcpy(&ua, &a, 8); __builtin_memcpy(&ub, &b, 8);
  return ua == ub;
}
// the arguments cs_atan2_lean has to decline by definition; every other pair is "ordinary"
bool special(double y, double x) {
  if (y != y || x != x) return true;
  const double ay = __builtin_fabs(y), ax = __builtin_fabs(x);
  const double big = ay > ax ? ay : ax, small = ay > ax ? ax : ay;
  if (big == 0 || big == __builtin_huge_val() || big < 0x1p-1022 || small == 0) return true;
  int e;
  (void)__builtin_frexp(big, &e);                      // big = f * 2^e, f in [0.5, 1): scaling big into [1, 2) multiplies by 2^(1 - e)
  return __builtin_ldexp(small, 1 - e) < 0x1p-200;
}
}  // namespace

extern "C" {

// out[i] = cs_atan2_lean's value where accepted[i] (else untouched), ref[i] = cs_atan2; returns the number of accepted pairs whose bits differ
long long lean_batch(const double* y, const double* x, long long n, double* out, unsigned char* accepted, double* ref, unsigned char* is_special) {
  long long bad = 0;
  for (long long k = 0; k < n; k++) {
    const double r = cs::cs_atan2(y[k], x[k]);
    double v = 0;
    const bool ok = cs::cs_atan2_lean(y[k], x[k], &v);
    if (ok) { out[k] = v; bad += !same_bits(v, r); }
    accepted[k] = ok; ref[k] = r;
    if (is_special) is_special[k] = special(y[k], x[k]);
  }
  return bad;
}

// the lean evaluation's unevaluated sum (the angle of (|y|, x), or its negative) and the relative bound of its rounding test; returns 0 for a special pair
int lean_value(double y, double x, double* hi, double* lo, double* rel_bound) {
  cs::dd_t v{0, 0};
  const bool ok = cs::cs_atan2_lean_eval(y, x, &v);
  *hi = v.hi; *lo = v.lo; *rel_bound = CS_ATAN2_LEAN_BOUND;
  return ok;
}

// n pseudo-random argument pairs of the given kind; returns the number of ACCEPTED pairs on which cs_atan2_lean and cs_atan2 differ,
// in *declined how many ordinary pairs were declined and in *specials how many pairs were special (all of which must be declined:
// one that is accepted counts as a difference).
//   kind 0: uniform in [-1500, 1500]^2   1: differences of integer pixel coordinates   2: half-pixel grid (segment mid points)
//   kind 3: exponents spread over 2^-60 .. 2^60
//   kind 4: quotients within +-0.51 / 256 of every table point i / 256 (even k: across the whole cell, to both of its edges and just beyond;
//           odd k: within 1e-6 / 256 of the cell edge (i + 0.5) / 256, where the single-precision quotient may pick either neighbour),
//           all four sign combinations, both argument orders
long long lean_compare(long long n, unsigned long long seed, int kind, long long* declined, long long* specials) {
  unsigned long long s = seed * 6364136223846793005ULL + 1442695040888963407ULL;
  auto rnd = [&]() { s = s * 6364136223846793005ULL + 1442695040888963407ULL; return (double)(s >> 11) * (1.0 / 9007199254740992.0); };
  long long bad = 0, dec = 0, spc = 0;
  for (long long k = 0; k < n; k++) {
    double y, x;
    if (kind == 0) { y = (rnd() * 2 - 1) * 1500; x = (rnd() * 2 - 1) * 1500; }
    else if (kind == 1) { y = (double)((long long)(rnd() * 2483) - 1241); x = (double)((long long)(rnd() * 2483) - 1241); }
    else if (kind == 2) { y = ((long long)(rnd() * 4966) - 2483) * 0.5; x = ((long long)(rnd() * 4966) - 2483) * 0.5 + (rnd() - 0.5) * 1e-9 * (double)(k & 1); }
    else if (kind == 3) {
      union { double d; uint64_t u; } a, b;
      a.d = rnd() + 1.0; b.d = rnd() + 1.0;
      a.u += (uint64_t)((long long)(rnd() * 120) - 60) << 52; b.u += (uint64_t)((long long)(rnd() * 120) - 60) << 52;
      y = (k & 1) ? -a.d : a.d; x = (k & 2) ? -b.d : b.d;
    } else {
      const int i = (int)((k >> 4) % 257);
      double q = (k & 1) ? ((double)i + 0.5 + (rnd() - 0.5) * 1e-6) / 256.0 : ((double)i + (rnd() - 0.5) * 1.02) / 256.0;
      q = q < 1e-9 ? 1e-9 : (q > 1.0 ? 1.0 : q);
      x = (rnd() + 0.5) * 1000; y = x * q;
      if (k & 2) { double t = x; x = y; y = t; }
      if (k & 4) x = -x;
      if (k & 8) y = -y;
    }
    const double r = cs::cs_atan2(y, x);
    double v = 0;
    const bool ok = cs::cs_atan2_lean(y, x, &v);
    const bool sp = special(y, x);
    spc += sp;
    if (ok) bad += (sp || !same_bits(v, r));
    else dec += !sp;
  }
  *declined = dec; *specials = spc;
  return bad;
}
}  // extern "C"
