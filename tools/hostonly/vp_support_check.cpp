// vp_support_check.cpp -- the vanishing-point support procedure of cube_slam_wu_amd/csrc/cs_vp_support.h on the CPU, against the reference's loop
// (object_3d_util.cpp:548-619) written plainly with cs_atan2.  Stand-alone: tests/test_vp_support_host_cpu.py builds it with
//   g++ -O1 -ffp-contract=off -fsanitize=address,undefined
// and runs it.  It demands equal (arg-max, arg-min) INDICES, not only equal angles, on
//   * 2 million seeded random tables of at most 70 segments (argument 1 = another count), vanishing points inside the segment cloud, around the
//     image and far away, half of the segments pointing at the vanishing point to within +-0.5 rad;
//   * the adversarial families below (each a few thousand tables): far vanishing points, collinear mid points on one side and on both sides of the
//     vanishing point, duplicated mid points, segment angles on both edges of the undecided band, vanishing points to the right of everything
//     (raw near +-pi), a vanishing point on a mid point, non-finite vanishing points, tables with no inlier and with exactly one.
// It counts how often each exact fallback ran.  On the random tables the undecided share must stay below 1e-3 of the classified segments (the band
// is 2e-4 rad wide out of pi): a cap on hidden fallbacks, not a performance figure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../cube_slam_wu_amd/csrc/cs_vp_support.h"

namespace {

struct Rng {      // splitmix64: the same stream on every standard library
  uint64_t s;
  uint64_t next() { uint64_t z = (s += 0x9e3779b97f4a7c15ull); z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull; z = (z ^ (z >> 27)) * 0x94d049bb133111ebull; return z ^ (z >> 31); }
  double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
  double uni(double a, double b) { return a + (b - a) * uni(); }
  int below(int n) { return (int)(next() % (uint64_t)n); }
};

struct Table {
  std::vector<double> mx, my, la;
  int m() const { return (int)mx.size(); }
  void push(double x, double y, double a) { mx.push_back(x); my.push_back(y); la.push_back(a); }
};

struct Counts { long long classified = 0, undecided = 0, inliers = 0, exact_greater = 0, exact_less = 0, tables = 0, with_inlier = 0; };

double fold(double a) { return a > CS_PI / 2 ? a - CS_PI : (a < -CS_PI / 2 ? a + CS_PI : a); }

// the reference's loop: indices of the arg-max and arg-min of the unwrapped inlier angles (-1, -1: no inlier)
void reference(const Table& t, double vpx, double vpy, double thre, int* i_hi, int* i_lo) {
  bool have = false;
  double base = 0, hi = 0, lo = 0;
  *i_hi = *i_lo = -1;
  for (int i = 0; i < t.m(); i++) {
    const double raw = cs::cs_atan2(t.my[i] - vpy, t.mx[i] - vpx);
    const double nrm = cs::normalize_to_pi(raw);
    double d = std::fabs(t.la[i] - nrm);
    d = std::fmin(d, CS_PI - d);
    if (!(d < thre)) continue;
    if (!have) { have = true; base = hi = lo = raw; *i_hi = *i_lo = i; continue; }
    double sh = raw;
    if ((raw - base) < -CS_PI) sh = raw + 2 * CS_PI;
    else if ((raw - base) > CS_PI) sh = raw - 2 * CS_PI;
    if (sh > hi) { hi = sh; *i_hi = i; }
    if (sh < lo) { lo = sh; *i_lo = i; }
  }
}

struct ExactCounted {
  const double* mx; const double* my; double vpx, vpy; Counts* c;
  bool greater(int i, int i_ref, int ib) const { c->exact_greater++; return cs::vp_exact_unwrapped(mx, my, i, ib, vpx, vpy) > cs::vp_exact_unwrapped(mx, my, i_ref, ib, vpx, vpy); }
  bool less(int i, int i_ref, int ib) const { c->exact_less++; return cs::vp_exact_unwrapped(mx, my, i, ib, vpx, vpy) < cs::vp_exact_unwrapped(mx, my, i_ref, ib, vpx, vpy); }
};

// the header's procedure, as the unstaged kernel form walks it
void procedure(const Table& t, double vpx, double vpy, double thre, Counts* c, int* i_hi, int* i_lo) {
  cs::VpRun R = cs::vp_run_empty();
  const cs::VpTan tn = cs::vp_tan_bounds((float)thre);
  const ExactCounted ex{t.mx.data(), t.my.data(), vpx, vpy, c};
  for (int i = 0; i < t.m(); i++) {
    const double dx = t.mx[i] - vpx, dy = t.my[i] - vpy;
    const int cls = cs::vp_classify((float)dx, (float)dy, cosf((float)t.la[i]), sinf((float)t.la[i]), tn);
    c->classified++;
    bool inlier = cls == cs::VP_IN;
    if (cls == cs::VP_UNDECIDED) { c->undecided++; inlier = cs::vp_exact_inlier(dy, dx, t.la[i], thre); }
    if (inlier) c->inliers++;
    cs::vp_order_step(R, i, dx, dy, inlier, ex);
  }
  *i_hi = R.have ? R.i_hi : -1;
  *i_lo = R.have ? R.i_lo : -1;
}

long long g_bad = 0;

void check(const char* family, const Table& t, double vpx, double vpy, double thre, Counts* c) {
  int rh, rl, ph, pl;
  reference(t, vpx, vpy, thre, &rh, &rl);
  procedure(t, vpx, vpy, thre, c, &ph, &pl);
  c->tables++;
  if (rh >= 0) c->with_inlier++;
  if (rh != ph || rl != pl) {
    if (g_bad < 20) std::printf("MISMATCH %s: m=%d vp=(%.17g, %.17g) thre=%.17g reference (%d, %d) procedure (%d, %d)\n", family, t.m(), vpx, vpy, thre, rh, rl, ph, pl);
    g_bad++;
  }
}

void report(const char* family, const Counts& c) {
  std::printf("%-22s tables %8lld with inlier %8lld segments %10lld inliers %9lld undecided %7lld exact greater %7lld less %7lld\n", family, c.tables, c.with_inlier, c.classified,
              c.inliers, c.undecided, c.exact_greater, c.exact_less);
}

const double THRE[2] = {15.0 / 180.0 * CS_PI, 10.0 / 180.0 * CS_PI};

// a segment cloud like an object's ROI; `aim` of the segments point at the vanishing point to within +-spread
Table cloud(Rng& g, int m, double vpx, double vpy, double aim, double spread) {
  Table t;
  for (int i = 0; i < m; i++) {
    const double x = g.uni(200, 500), y = g.uni(100, 300);
    double a = g.uni(-CS_PI / 2, CS_PI / 2);
    if (g.uni() < aim) a = fold(fold(std::atan2(y - vpy, x - vpx)) + g.uni(-spread, spread));
    t.push(x, y, a);
  }
  return t;
}

void random_vp(Rng& g, int kind, double* vpx, double* vpy) {
  if (kind == 0) { *vpx = g.uni(150, 550); *vpy = g.uni(50, 350); }                    // inside the cloud: wrap-arounds
  else if (kind == 1) { *vpx = g.uni(-2000, 3000); *vpy = g.uni(-1500, 2000); }
  else { const double r = std::pow(10.0, g.uni(4, 9)), a = g.uni(0, 2 * CS_PI); *vpx = r * std::cos(a); *vpy = r * std::sin(a); }
}

}  // namespace

int main(int argc, char** argv) {
  const long long n_random = argc > 1 ? std::atoll(argv[1]) : 2000000;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  Rng g{20240611};

  {  // seeded random tables
    Counts c;
    for (long long k = 0; k < n_random; k++) {
      double vpx, vpy;
      random_vp(g, (int)(k % 4), &vpx, &vpy);
      const int m = 1 + g.below(k % 16 == 0 ? 70 : 12);      // (short tables mostly: a table costs its segments; every sixteenth up to 70)
      check("random", cloud(g, m, vpx, vpy, 0.5, 0.5), vpx, vpy, THRE[k & 1], &c);
    }
    report("random", c);
    if (!(c.undecided < 1e-3 * c.classified)) { std::printf("FAIL: undecided share %.3g of the classified segments is not below 1e-3\n", (double)c.undecided / (double)c.classified); g_bad++; }
    if (c.with_inlier * 2 < c.tables) { std::printf("FAIL: fewer than half of the random tables have an inlier\n"); g_bad++; }
  }
  {  // far vanishing points, 1e1 .. 1e8 px from the segments: every direction within microradians
    Counts c;
    for (int k = 0; k < 8000; k++) {
      const double r = std::pow(10.0, 1 + (k % 8)), a = g.uni(0, 2 * CS_PI);
      const double vpx = 350 + r * std::cos(a), vpy = 200 + r * std::sin(a);
      check("far", cloud(g, 3 + g.below(67), vpx, vpy, 0.7, 0.2), vpx, vpy, THRE[k & 1], &c);
    }
    report("far", c);
  }
  {  // mid points collinear with the vanishing point, on one side (difference 0) and on both (difference pi), mixed into a cloud
    Counts c;
    for (int k = 0; k < 8000; k++) {
      double vpx, vpy;
      random_vp(g, k % 2, &vpx, &vpy);
      if (k % 3 == 0) { vpx = std::floor(vpx); vpy = std::floor(vpy); }      // (integers: exactly collinear points exist)
      Table t = cloud(g, g.below(20), vpx, vpy, 0.6, 0.2);
      const double a = g.uni(0, 2 * CS_PI), cx = std::cos(a), cy = std::sin(a);
      const int n_line = 2 + g.below(8);
      for (int q = 0; q < n_line; q++) {
        double s = (k % 3 == 0) ? (double)(1 + g.below(40)) : g.uni(1, 300);
        if ((k & 4) && g.uni() < 0.5) s = -s;
        const double x = (k % 3 == 0) ? vpx + s * 3 : vpx + s * cx, y = (k % 3 == 0) ? vpy + s * 4 : vpy + s * cy;
        t.push(x, y, fold(fold(std::atan2(y - vpy, x - vpx)) + g.uni(-0.1, 0.1)));
      }
      for (int q = 0; q < t.m(); q++) {      // shuffle, so that the base is not always a cloud segment
        const int r = g.below(t.m());
        std::swap(t.mx[q], t.mx[r]); std::swap(t.my[q], t.my[r]); std::swap(t.la[q], t.la[r]);
      }
      check("collinear", t, vpx, vpy, THRE[k & 1], &c);
    }
    report("collinear", c);
  }
  {  // duplicated mid points with different segment angles, both inliers: a tie in the unwrapped angle, visible in the output angle
    Counts c;
    for (int k = 0; k < 8000; k++) {
      double vpx, vpy;
      random_vp(g, k % 3, &vpx, &vpy);
      Table t = cloud(g, 2 + g.below(30), vpx, vpy, 0.7, 0.2);
      const int n_dup = 1 + g.below(4);
      for (int q = 0; q < n_dup; q++) {
        const int src = g.below(t.m()), at = g.below(t.m() + 1);
        const double x = t.mx[src], y = t.my[src], a = fold(fold(std::atan2(y - vpy, x - vpx)) + g.uni(-0.15, 0.15));
        t.mx.insert(t.mx.begin() + at, x); t.my.insert(t.my.begin() + at, y); t.la.insert(t.la.begin() + at, a);
      }
      check("duplicates", t, vpx, vpy, THRE[k & 1], &c);
    }
    report("duplicates", c);
  }
  {  // segment angles at thre +- {0, 1 ulp, 1e-12, 1e-6, 9e-5, 1.1e-4} from the direction: both edges of the undecided band
    Counts c;
    const double off[6] = {0.0, -1.0, 1e-12, 1e-6, 9e-5, 1.1e-4};
    for (int k = 0; k < 12000; k++) {
      double vpx, vpy;
      random_vp(g, k % 3, &vpx, &vpy);
      const double thre = THRE[k & 1];
      Table t = cloud(g, 2 + g.below(20), vpx, vpy, 0.3, 0.2);
      for (int i = 0; i < t.m(); i++) {
        if (g.uni() < 0.3) continue;
        const double nrm = fold(std::atan2(t.my[i] - vpy, t.mx[i] - vpx));
        const double side = g.uni() < 0.5 ? -1.0 : 1.0, sgn = g.uni() < 0.5 ? -1.0 : 1.0;
        const int o = g.below(6);
        double a = nrm + side * thre;
        if (off[o] < 0) a = std::nextafter(a, sgn * 10.0); else a += sgn * off[o];
        t.la[i] = fold(a);
      }
      check("band edges", t, vpx, vpy, thre, &c);
    }
    report("band edges", c);
  }
  {  // vanishing points to the right of all segments: raw sits near +-pi, and the unwrap shifts some inliers and not others
    Counts c;
    for (int k = 0; k < 8000; k++) {
      const double vpx = 500 + std::pow(10.0, g.uni(0, 6)), vpy = g.uni(100, 300);
      Table t = cloud(g, 2 + g.below(40), vpx, vpy, 0.8, 0.2);
      if (k % 4 == 0) for (int i = 0; i < t.m(); i += 3) t.my[i] = vpy;      // (raw = +pi exactly)
      check("right of all", t, vpx, vpy, THRE[k & 1], &c);
    }
    report("right of all", c);
  }
  {  // a vanishing point equal to a mid point (the zero vector)
    Counts c;
    for (int k = 0; k < 6000; k++) {
      Table t = cloud(g, 2 + g.below(30), 350, 200, 0.0, 0.0);
      const int z = g.below(t.m());
      const double vpx = t.mx[z], vpy = t.my[z];
      for (int i = 0; i < t.m(); i++)
        if (g.uni() < 0.7) t.la[i] = fold(fold(std::atan2(t.my[i] - vpy, t.mx[i] - vpx)) + g.uni(-0.2, 0.2));      // (the zero vector: atan2 = 0)
      if (k % 2) t.la[z] = g.uni(-0.1, 0.1);
      check("on a mid point", t, vpx, vpy, THRE[k & 1], &c);
    }
    report("on a mid point", c);
  }
  {  // vanishing point coordinates of +-inf and NaN (a homogeneous point with h2 = 0)
    Counts c;
    const double special[3] = {inf, -inf, nan};
    for (int k = 0; k < 3000; k++) {
      Table t = cloud(g, 1 + g.below(30), 350, 200, 0.0, 0.0);
      for (int i = 0; i < t.m(); i++)
        if (g.uni() < 0.5) t.la[i] = fold((g.uni() < 0.5 ? 0.0 : CS_PI / 2) + (g.uni() < 0.5 ? 0.0 : g.uni(-0.2, 0.2)));      // (atan2 of an infinite pair is a multiple of pi/4)
      const double sx = special[k % 3], sy = special[(k / 3) % 3];
      const int which = (k / 9) % 3;
      check("non-finite", t, which == 1 ? g.uni(0, 600) : sx, which == 0 ? g.uni(0, 400) : sy, THRE[k & 1], &c);
    }
    report("non-finite", c);
  }
  {  // tables with no inlier and with exactly one; the empty table
    Counts c;
    long long expected = 0;
    for (int k = 0; k < 6000; k++) {
      double vpx, vpy;
      random_vp(g, k % 3, &vpx, &vpy);
      const double thre = THRE[k & 1];
      Table t = cloud(g, g.below(40), vpx, vpy, 0.0, 0.0);
      for (int i = 0; i < t.m(); i++) t.la[i] = fold(fold(std::atan2(t.my[i] - vpy, t.mx[i] - vpx)) + (g.uni() < 0.5 ? -1 : 1) * g.uni(thre + 0.01, CS_PI / 2));
      if ((k % 2) && t.m()) { const int i = g.below(t.m()); t.la[i] = fold(fold(std::atan2(t.my[i] - vpy, t.mx[i] - vpx)) + g.uni(-0.9, 0.9) * thre); expected++; }
      check("none or one", t, vpx, vpy, thre, &c);
    }
    report("none or one", c);
    if (c.with_inlier != expected || c.inliers != expected) { std::printf("FAIL: the tables built with no inlier or exactly one have others\n"); g_bad++; }
  }
  if (g_bad) { std::printf("vp_support_check: %lld FAILURES\n", g_bad); return 1; }
  std::printf("vp_support_check: ok\n");
  return 0;
}
