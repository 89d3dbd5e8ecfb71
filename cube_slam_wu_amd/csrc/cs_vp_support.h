// cs_vp_support.h -- the decisions of VP_support_edge_infos (object_3d_util.cpp:548-619) for one vanishing point, without angles.
//
// The reference evaluates raw_i = atan2(P_i - vp) for every segment (mid point P_i, angle la_i), keeps the segments whose
// direction is within `thre` of their own angle (the inliers), unwraps the kept angles against the first one (smooth_jump_angles,
// :278-302: sh_i = raw_i, shifted by -+2 pi where raw_i - base exceeds +-pi) and returns the segment angles at the arg-max and the
// arg-min of sh (maxCoeff / minCoeff: strict, the first occurrence wins a tie).  Only those two indices leave the function, so this
// header states a procedure that reaches the same indices from cross products, and names the few cases it hands to the exact
// evaluation (cs_atan2 on the reference's own argument pairs).  One statement for the HIP kernels (detect_kernels.hip) and the host
// (tools/hostonly/vp_support_check.cpp runs it against the plain loop).
//
// 1. Three-way classification of a segment against a point (vp_classify).  With u = (cosf, sinf) of the segment's angle and
//    f = (float)(P - vp), the circular angle between them is below thre exactly when |u x f| < tan(thre) |u . f|.  In float, with
//    thre moved by 1e-4 rad and 2e-6 (|fx| + |fy|) of slack for the roundings (direction 3e-7 rad, each product / sum 6e-8
//    relative; tests/test_device_decisions.py models the first test):
//      out for sure   cr > fma(tanf(thre_f + 1e-4f), dt,  slack)     no true inlier passes this test;
//      in for sure    cr < fma(tanf(thre_f - 1e-4f), dt, -slack)     the same budget mirrored: no true outlier passes this one.  False for
//                     NaN and inf, false for the zero vector (0 < 0), never true when thre_f - 1e-4f <= 0 or thre_f >= 1.5 (where the
//                     first test keeps everything): such thresholds send every segment to the exact test, slow and correct;
//      undecided      everything else, a band 2e-4 rad wide: the exact evaluation decides (cs_atan2, normalize_to_pi, the fold).
//    (Both tests assume what the line setup guarantees: segment angles in [-pi/2, pi/2], so that the reference's
//    min(|la - nrm|, pi - |la - nrm|) is the circular distance.)
//
// 2. Order without angles (vp_order_step).  Let d_i = P_i - vp in double -- the pair the reference hands to atan2 -- and b = d of
//    the first inlier; x(a, c) = a.x c.y - a.y c.x and lim(a, c) = 1e-12 (|a.x| + |a.y|) (|c.x| + |c.y|).
//      x(b, d_i) >  lim   the inlier is LEFT of the base:  sh_i - base in (0, pi);
//      x(b, d_i) < -lim   it is RIGHT of the base:          sh_i - base in (-pi, 0).
//    Left values lie above the base and right values below it, so a right inlier never raises the maximum and a left one never
//    lowers the minimum (the maximum is never below the base, the minimum never above it, whatever installed them).  A left
//    inlier raises a maximum that still is the base; against a maximum that is itself left it differs by less than pi, and
//    x(d_hi, d_i) > lim means sh_i > sh_hi, < -lim means sh_i < sh_hi.  The minimum is the mirror image.  Updates are strict.
//    Two cases go to the exact comparison of the two unwrapped cs_atan2 values (Exact::greater / Exact::less):
//      any |x| <= lim (or NaN): collinear with the base or with the extreme, in the same or the opposite direction -- the +-pi
//        unwrap edge and exact ties are here;
//      any comparison against an extreme whose side is UNKNOWN, which is the side of an extreme that an exact comparison installed.
//
// Why the signs are the reference's decisions.  cs_atan2 is within 2^-83 relative of the true angle of exactly these argument pairs,
// and the +-2 pi shift adds one rounding (2^-52 of at most 3 pi).  |x| > lim means the true directions differ by more than 1e-12 rad
// (|sin| = |x| / (|a| |c|) and the product of the 1-norms is at least the product of the 2-norms), thousands of ulps of the rounded
// values, so the rounded values are ordered as the true ones and are not equal.  x itself is two products and a difference in
// double: its rounding error is below 4e-16 of the product of the 1-norms, so a value beyond lim has the true sign.  The
// reference's unwrap decision (raw_i - base against +-pi) can disagree with the side only when the two directions are opposite to
// within rounding, and then |x(b, d_i)| <= lim and the exact path runs: for a left inlier the true difference lies in
// (1e-12, pi - 1e-12), the rounded raw_i - base is that or that minus 2 pi, the first is not shifted and the second is shifted up.
#pragma once
#include "cs_geom.h"
#if !defined(__HIPCC__)
#include <math.h>
#endif

namespace cs {

enum { VP_OUT = 0, VP_IN = 1, VP_UNDECIDED = 2 };                 // vp_classify
enum { VP_SIDE_BASE = 0, VP_SIDE_OWN = 1, VP_SIDE_UNKNOWN = 2 };  // a running extreme: the first inlier itself; left (maximum) / right (minimum) of it; installed by an exact comparison

// the two tangents of the classification for a threshold
struct VpTan { float out, in; };
CS_HD VpTan vp_tan_bounds(float thre_f) {
  VpTan t;
  t.out = thre_f < 1.5f ? tanf(thre_f + 1.0e-4f) : __builtin_huge_valf();      // (a threshold near 90 degrees keeps everything)
  t.in = (thre_f < 1.5f && thre_f - 1.0e-4f > 0.0f) ? tanf(thre_f - 1.0e-4f) : -__builtin_huge_valf();
  return t;
}

// the two tests apart, on the float difference (fx, fy) and the unit direction (ux, uy): the staged kernel keeps a bit of each
struct VpSure { bool out, in; };
CS_HD VpSure vp_classify_sure(float fx, float fy, float ux, float uy, VpTan t) {
  const float cr = __builtin_fabsf(__builtin_fmaf(fx, uy, -(fy * ux))), dt = __builtin_fabsf(__builtin_fmaf(fx, ux, fy * uy));
  const float slack = 2.0e-6f * (__builtin_fabsf(fx) + __builtin_fabsf(fy));
  VpSure s;
  s.out = cr > __builtin_fmaf(t.out, dt, slack);      // (false for NaN / inf: those go on)
  s.in = cr < __builtin_fmaf(t.in, dt, -slack);       // (false for NaN / inf / the zero vector)
  return s;
}
CS_HD int vp_classify(float fx, float fy, float ux, float uy, VpTan t) {
  const VpSure s = vp_classify_sure(fx, fy, ux, uy, t);
  return s.out ? VP_OUT : s.in ? VP_IN : VP_UNDECIDED;
}

// the exact inlier test of an undecided segment: the reference's expressions (:573-577)
CS_HD bool vp_exact_inlier(double dy, double dx, double lai, double thre) {
  const double nrm = normalize_to_pi(cs_atan2(dy, dx));
  double d = dabs(lai - nrm);
  d = dmin(d, CS_PI - d);
  return d < thre;
}

// exact unwrapped angle of segment i against the first inlier ib (both evaluated anew: this runs a few times per million segments)
CS_HD double vp_exact_unwrapped(const double* mx, const double* my, int i, int ib, double vpx, double vpy) {
  const double raw = cs_atan2(my[i] - vpy, mx[i] - vpx);
  if (i == ib) return raw;
  const double base = cs_atan2(my[ib] - vpy, mx[ib] - vpx);
  if ((raw - base) < -CS_PI) return raw + 2 * CS_PI;
  if ((raw - base) > CS_PI) return raw - 2 * CS_PI;
  return raw;
}

struct VpRun {               // running state of one vanishing point's sweep over the segments
  bool have;
  unsigned char side_hi, side_lo;   // VP_SIDE_* of the two running extremes
  int ib, i_hi, i_lo;        // first inlier, running arg-max / arg-min of the unwrapped angle
  double bx, by;             // mid point - vanishing point of the first inlier ...
  double hx, hy, lx, ly;     // ... and of the two running extremes
};
CS_HD VpRun vp_run_empty() { return VpRun{false, VP_SIDE_BASE, VP_SIDE_BASE, 0, 0, 0, 0., 0., 0., 0., 0., 0.}; }

// One segment i (d = mid point - vanishing point, in double) against the running extremes; `inlier` = it is one (false: nothing moves).
// Exact: bool greater(int i, int i_ref, int ib) const -- sh_i > sh_ref on the exact unwrapped values -- and less(...) likewise.
// An inlier is left or right of the base (or neither), so it can move one extreme only: that extreme is selected first, and the
// one cross product against it decides.  Written as one straight line of selects with a single, rarely taken branch (the exact
// comparisons): the lanes of a wavefront each sweep their own point, and every data-dependent branch here would be taken by some lane.
// (The first inlier runs through the same arithmetic on a zeroed state and is installed by `first`.)
// Two things below are there for the reader and for caution, not because a case needs them:
//   * the VP_SIDE_BASE terms of `sure` and `moves` restate the rule "a left inlier raises a maximum that still is the base".  While an
//     extreme's side is BASE its vector is the base vector, so c and lim repeat xb and limb bit for bit and `beyond` alone says the same;
//   * VP_SIDE_UNKNOWN is conservative.  An exact comparison installs only extremes that are collinear with the base or with an extreme of
//     their own side, and no table is known on which treating such an extreme as VP_SIDE_OWN gives a wrong index (the stand-alone check
//     passes either way); the argument above is made for extremes strictly left or right of the base only, so the others are not trusted
//     with a cross product.  The cost is an exact comparison per later inlier of that side, in tables that have such an extreme.
template <class Exact>
CS_HD void vp_order_step(VpRun& R, int i, double dx, double dy, bool inlier, const Exact& ex) {
  const bool first = inlier && !R.have;          // base of smooth_jump_angles (:278-302), and initial arg-max / arg-min
  const double nd = dabs(dx) + dabs(dy);
  const double xb = R.bx * dy - R.by * dx, limb = 1.0e-12 * (nd * (dabs(R.bx) + dabs(R.by)));
  const bool left = xb > limb, right = xb < -limb;
  const double ex_ = left ? R.hx : R.lx, ey_ = left ? R.hy : R.ly;      // the extreme this inlier can move: the maximum for left, the minimum for right
  const int side_e = left ? R.side_hi : R.side_lo;
  const double c = ex_ * dy - ey_ * dx, lim = 1.0e-12 * (nd * (dabs(ex_) + dabs(ey_)));
  const bool above = c > lim, below = c < -lim;
  const bool beyond = (left && above) || (right && below), decided = above || below;
  const bool sure = (left || right) && (side_e == VP_SIDE_BASE || (side_e == VP_SIDE_OWN && decided));
  const bool moves = side_e == VP_SIDE_BASE || beyond;
  bool up = left && moves, down = right && moves;      // this inlier becomes the maximum / the minimum
  unsigned char side = first ? VP_SIDE_BASE : VP_SIDE_OWN;
  if (inlier && !first && !sure) {      // collinear with the base or the extreme (same or opposite direction, zero vector, NaN), or an extreme of unknown side
    side = VP_SIDE_UNKNOWN;
    up = !right && ex.greater(i, R.i_hi, R.ib);
    down = !left && ex.less(i, R.i_lo, R.ib);
  }
  up = first || (inlier && up); down = first || (inlier && down);
  R.have = R.have || inlier;
  R.ib = first ? i : R.ib; R.bx = first ? dx : R.bx; R.by = first ? dy : R.by;
  R.i_hi = up ? i : R.i_hi; R.hx = up ? dx : R.hx; R.hy = up ? dy : R.hy; R.side_hi = up ? side : R.side_hi;      // maxCoeff: first occurrence, strict
  R.i_lo = down ? i : R.i_lo; R.lx = down ? dx : R.lx; R.ly = down ? dy : R.ly; R.side_lo = down ? side : R.side_lo;      // minCoeff
}

}  // namespace cs
