// cs_atan2_lean.h -- cs_atan2's light evaluation without the plumbing its ordinary callers never need.
//
// cs_atan2_lean(y, x, &out) either returns true and cs_atan2(y, x)'s bits in *out, or returns false and leaves *out
// alone; the caller then asks cs_atan2.  It serves callers that evaluate many ordinary arguments per lane (the scorer's
// angle term, detect_kernels.hip): the IEEE special cases, the subnormal pre-scaling and the double-double evaluation
// stay in cs_atan2, behind the caller's cold call.
//
// What it computes.  For ordinary arguments -- no NaN, the larger magnitude finite and normal, the smaller one not
// zero and, after scaling, not below 2^-200 -- the larger magnitude's exponent is removed from both with one exact
// ldexp each (big in [1, 2); small cannot underflow once it passes the 2^-200 test, and a small that does underflow
// fails that test).  Table index, numerator and denominator pairs, the single division with its remainder and the
// cubic correction are dd_atan_fast's, value for value: a = atan(small / big) = A[i] + th + tl + corr.  Where
// cs_atan2 then reflects a twice, each time through a renormalised double-double, the angle of the octant,
//     K + s * a,   (K, s) = (0, +), (pi/2, -), (pi, -), (pi/2, +)   for (swap, x < 0) = (0,0), (1,0), (0,1), (1,1),
// is formed here, up to its sign, as ONE double-double sum
//     s * K + a = m * pi/2 + a,   m = 0, -1, -2, +1
// (the pi and pi/2 pairs of cs_atan2_tab.h differ by an exact factor of two).  The sign is dropped at the end, where y's
// sign goes on: no operand is negated on the way.  0 < a <= pi/4 + , so the sum's magnitude is never smaller than a: the
// absolute error of a (< 2^-69 a, see dd_atan_fast), that of K (2^-106 K) and the roundings of the low-order additions
// (a few 2^-106 of the sum) stay below 2^-69 of the sum.  tests/test_atan2_lean.py measures hi + lo against mpmath at 300
// bits over the four octant cases (2^-70.5) and requires the worst relative error to stay four times below the bound used
// in the rounding test, 2^-68.
//
// Why an accepted value is cs_atan2's.  The rounding test hi + (lo + bound) == hi + (lo - bound), with a valid bound,
// shows that every real number within bound of hi + lo rounds to the same double; the true angle is one of them, so
// the returned double is the correctly rounded true angle.  cs_atan2 returns the correctly rounded true angle unless
// the true angle lies within ~2^-83 (relative) of a rounding boundary, whichever of its two paths it takes.  Such an
// angle is within 2^-68 of a boundary as well, so it fails the test here and is declined.  Wherever the lean function
// accepts, both therefore return the same double.  About 4e-5 of ordinary arguments are declined (2 * 2^-68 / 2^-53
// of the values lie that close to a boundary, more for results just above a power of two).
//
// Only +, -, *, /, fma and exact power-of-two scaling are used, all IEEE-exact on x86-64 and gfx950: host and device
// accept the same arguments and return the same bits.  Build rule as for cs_atan2.h: -ffp-contract=off.
#pragma once
#include "cs_atan2.h"

namespace cs {

// relative bound of the rounding test; the measured error of hi + lo is more than four times smaller (header comment)
#define CS_ATAN2_LEAN_BOUND 0x1p-68

// The evaluation: false for a special argument pair, else true and *v = the angle of (|y|, x) in [0, pi] OR ITS NEGATIVE as an
// unevaluated sum (v->hi carries it to a few ulp, v->lo need not be below half an ulp of v->hi).
CS_HD bool cs_atan2_lean_eval(double y, double x, dd_t* v_out) {
  static const double ftab[CS_ATAN_FTAB_N][2] = CS_ATAN_FTAB_INIT;
  const bool swap = __builtin_fabs(y) > __builtin_fabs(x);   // false when either is NaN: a NaN x is caught by its exponent, a NaN y by the 2^-200 test
  const double hi_arg = swap ? y : x, lo_arg = swap ? x : y;
  const int eb = (int)((cs_bits(hi_arg) >> 52) & 0x7ff);
  const double big = __builtin_ldexp(__builtin_fabs(hi_arg), 1023 - eb), small = __builtin_ldexp(__builtin_fabs(lo_arg), 1023 - eb);
  // larger magnitude zero or subnormal (eb == 0), infinite or NaN (eb == 2047); smaller one zero, NaN or too small to scale
  bool ok = ((unsigned)(eb - 1) < 2046u) & (small >= 0x1p-200);      // (& and not &&: no branches, the lanes of a wavefront go together anyway)
  // ---- dd_atan_fast(small, big) without its last renormalisation.  Two of its two_sums are written as fast_two_sums: big >= c small
  // and A[i] >= atan(1 / 256) > |th| (or A[0] == 0) meet the precondition, and both forms return the one exact (sum, error) pair
  const float qf = (float)small / (float)big;
  int i = (int)(qf * 256.0f + 0.5f);
  i = i < 0 ? 0 : (i > 256 ? 256 : i);
  const double c = (double)i * (1.0 / 256.0);
  const dd_t pb = dd_two_prod(c, big);
  const dd_t ns = dd_two_sum(small, -pb.hi);
  const double Nl = ns.lo - pb.lo;
  const dd_t ps = dd_two_prod(c, small);
  const dd_t ds = dd_fast_two_sum(big, ps.hi);
  const double Dl = ds.lo + ps.lo;
  const double inv = 1.0 / ds.hi;
  const double th = ns.hi * inv;
  const double r = __builtin_fma(-th, ds.hi, ns.hi) + (Nl - th * Dl);
  const double tl = r * inv;
  ok = ok & (__builtin_fabs(th) <= 0x1.1p-9);    // the error bound assumes |t| <= 2^-9 (+ slack), as in dd_atan_fast
  const double u = th * th;
  const double corr = th * (u * (-1.0 / 3.0 + u * (1.0 / 5.0 + u * (-1.0 / 7.0))));
  const dd_t s = dd_fast_two_sum(ftab[i][0], th);
  const double lo = s.lo + (ftab[i][1] + (tl + corr));
  // ---- sigma * (K + sigma * a) = m * pi/2 + a as one double-double sum, m = 0, -1, -2, +1: the angle up to its sign, which the caller drops
  // (|m pi/2| >= pi/2 > a, or m == 0: fast_two_sum again)
  const bool xneg = cs_bits(x) < 0;
  const double m = swap ? (xneg ? 1.0 : -1.0) : (xneg ? -2.0 : 0.0);
  const dd_t v = dd_fast_two_sum(m * CS_DD_PI_2_HI, s.hi);
  *v_out = dd_t{v.hi, v.lo + (m * CS_DD_PI_2_LO + lo)};
  return ok;
}

CS_HD bool cs_atan2_lean(double y, double x, double* out) {
  dd_t v;
  const bool ok = cs_atan2_lean_eval(y, x, &v);
  // (the sum is not renormalised: v.lo + bound rounds at 2^-53 |v.lo| <= 2^-72 |v.hi|, which the margin on the bound covers;
  // v may be the negated angle, which the test does not mind)
  const double bound = v.hi * CS_ATAN2_LEAN_BOUND;
  const double up = v.hi + (v.lo + bound), dn = v.hi + (v.lo - bound);
  const bool accept = ok & (up == dn);
  if (accept) *out = __builtin_copysign(up, y);
  return accept;
}

}  // namespace cs
