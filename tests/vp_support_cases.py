"""Inputs for the vanishing-point support check (cs_check_vp_support: one segment table against up to 192 points), and a plain float64 statement
of VP_support_edge_infos (object_3d_util.cpp:548-619) in numpy for the points that keep clear of every threshold.

A case is a dict: name, mx, my, la (the table: mid points and segment angles in [-pi/2, pi/2]), vpx, vpy (the points), thre (radians).
Table sizes m = 0, 1, 2, 63, 64, 65, 130 (the staged form's chunk is 64 segments), with the first inlier also in the second and in the third chunk.
The adversarial families (tools/hostonly/vp_support_check.cpp runs the same ones on the CPU):
  far          vanishing points 1e1 .. 1e8 px from the segments (far points see every direction within microradians);
  collinear    mid points collinear with the vanishing point, on one side (difference 0) and on both sides (difference pi);
  duplicates   duplicated mid points with different segment angles, both inliers (a tie in the unwrapped angle shows in the output angle);
  band         segment angles at thre +- {0, 1 ulp, 1e-12, 1e-6, 9e-5, 1.1e-4} from the direction: both edges of the undecided band;
  right        vanishing points to the right of all segments: raw sits near +-pi, the unwrap shifts some inliers and not others;
  on_mid       a vanishing point equal to a mid point (the zero vector);
  nonfinite    vanishing point coordinates of +-inf and NaN;
  none / one   tables with no inlier and with exactly one."""
import numpy as np

PI = np.pi
THRE = (15.0 / 180.0 * PI, 10.0 / 180.0 * PI)
SIZES = (0, 1, 2, 63, 64, 65, 130)
N_POINTS = 192


def fold(a):
    a = np.asarray(a, np.float64)
    return np.where(a > PI / 2, a - PI, np.where(a < -PI / 2, a + PI, a))


def direction(mx, my, vpx, vpy):
    """normalize_to_pi of the angle of (mid point - vanishing point)"""
    return fold(np.arctan2(my - vpy, mx - vpx))


def cloud(rng, m, vpx, vpy, aim, spread):
    """m segments in an ROI-sized cloud; a share `aim` of them point at (vpx, vpy) to within +-spread"""
    mx, my = rng.uniform(200, 500, m), rng.uniform(100, 300, m)
    la = rng.uniform(-PI / 2, PI / 2, m)
    pick = rng.random(m) < aim
    la = np.where(pick, fold(direction(mx, my, vpx, vpy) + rng.uniform(-spread, spread, m)), la)
    return mx, my, la


def points_around(rng, n, cx, cy):
    """n points of every kind around a nominal vanishing point: itself, near it, inside the cloud, around the image"""
    k = np.arange(n) % 4
    jit = 10.0 ** rng.uniform(-3, 2, n)
    ang = rng.uniform(0, 2 * PI, n)
    vx = np.where(k == 0, cx, np.where(k == 1, cx + jit * np.cos(ang), np.where(k == 2, rng.uniform(150, 550, n), rng.uniform(-2000, 3000, n))))
    vy = np.where(k == 0, cy, np.where(k == 1, cy + jit * np.sin(ang), np.where(k == 2, rng.uniform(50, 350, n), rng.uniform(-1500, 2000, n))))
    return vx, vy


def _case(name, mx, my, la, vpx, vpy, thre):
    c = dict(name=name, thre=float(thre))
    for k, v in (("mx", mx), ("my", my), ("la", la), ("vpx", vpx), ("vpy", vpy)):
        c[k] = np.ascontiguousarray(v, np.float64)
    assert len(c["mx"]) == len(c["my"]) == len(c["la"]) and len(c["vpx"]) == len(c["vpy"]) <= N_POINTS
    assert np.all(np.abs(c["la"]) <= PI / 2)
    return c


def all_cases():
    rng = np.random.default_rng(20240611)
    cases = []
    # every table size, points of every kind
    for q, m in enumerate(SIZES):
        thre = THRE[q & 1]
        cx, cy = (rng.uniform(-500, 1200), rng.uniform(-400, 800))
        mx, my, la = cloud(rng, m, cx, cy, 0.6, 0.3)
        vx, vy = points_around(rng, N_POINTS if m != 1 else 191, cx, cy)      # (an odd count: the last pair of the paired forms is half empty)
        cases.append(_case("size_%d" % m, mx, my, la, vx, vy, thre))
    # the first inlier in the second and in the third chunk: every earlier segment is perpendicular to its direction from every point used
    for first in (64, 100, 128, 129):
        cx, cy = 350.0 + 3000.0, 200.0
        mx, my, la = cloud(rng, 130, cx, cy, 0.7, 0.2)
        la[:first] = fold(direction(mx[:first], my[:first], cx, cy) + PI / 2 + rng.uniform(-0.3, 0.3, first))
        la[first] = fold(direction(mx[first], my[first], cx, cy) + 0.05)
        ang = rng.uniform(0, 2 * PI, N_POINTS)
        vx, vy = cx + rng.uniform(0, 100, N_POINTS) * np.cos(ang), cy + rng.uniform(0, 100, N_POINTS) * np.sin(ang)
        cases.append(_case("first_inlier_at_%d" % first, mx, my, la, vx, vy, THRE[0]))
    # far vanishing points
    for m in (65, 130):
        r = 10.0 ** (1 + np.arange(N_POINTS) % 8)
        ang = rng.uniform(0, 2 * PI, N_POINTS)
        vx, vy = 350 + r * np.cos(ang), 200 + r * np.sin(ang)
        mx, my, la = cloud(rng, m, vx[7], vy[7], 0.8, 0.15)
        cases.append(_case("far_%d" % m, mx, my, la, vx, vy, THRE[1]))
    # collinear mid points: on a ray from the point (difference 0) and on both sides of it (difference pi); integer coordinates make it exact
    for both in (False, True):
        vpx0, vpy0 = 340.0, 210.0
        mx, my, la = cloud(rng, 70, vpx0, vpy0, 0.5, 0.2)
        s = rng.integers(1, 40, 30).astype(np.float64) * (np.where(rng.random(30) < 0.5, -1.0, 1.0) if both else 1.0)
        at = rng.choice(70, 30, replace=False)
        mx[at], my[at] = vpx0 + 3 * s, vpy0 + 4 * s
        la[at] = fold(direction(mx[at], my[at], vpx0, vpy0) + rng.uniform(-0.1, 0.1, 30))
        vx, vy = points_around(rng, N_POINTS, vpx0, vpy0)
        vx[::2], vy[::2] = vpx0, vpy0
        cases.append(_case("collinear_%s" % ("both_sides" if both else "one_side"), mx, my, la, vx, vy, THRE[0]))
    # duplicated mid points, different angles, both inliers
    vpx0, vpy0 = -300.0, 900.0
    mx, my, la = cloud(rng, 66, vpx0, vpy0, 0.7, 0.15)
    src, dst = rng.choice(66, 40, replace=False).reshape(2, 20)
    mx[dst], my[dst] = mx[src], my[src]
    la[dst] = fold(direction(mx[dst], my[dst], vpx0, vpy0) + rng.uniform(-0.12, 0.12, 20))
    la[src] = fold(direction(mx[src], my[src], vpx0, vpy0) + rng.uniform(-0.12, 0.12, 20))
    vx, vy = points_around(rng, N_POINTS, vpx0, vpy0)
    cases.append(_case("duplicates", mx, my, la, vx, vy, THRE[0]))
    # both edges of the undecided band, for the first point; the other points sit within 1e-3 px of it (their directions move by microradians)
    for q, (vpx0, vpy0) in enumerate(((420.0, 180.0), (-1500.0, 2600.0), (3.0e6, -2.0e6))):
        thre = THRE[q & 1]
        mx, my, la = cloud(rng, 65, vpx0, vpy0, 0.3, 0.2)
        off = np.array([0.0, np.nan, 1e-12, 1e-6, 9e-5, 1.1e-4])[rng.integers(0, 6, 65)]
        side, sgn = np.where(rng.random(65) < 0.5, -1.0, 1.0), np.where(rng.random(65) < 0.5, -1.0, 1.0)
        a = direction(mx, my, vpx0, vpy0) + side * thre
        a = np.where(np.isnan(off), np.nextafter(a, sgn * 10.0), a + sgn * np.nan_to_num(off))
        keep = rng.random(65) < 0.3
        la = np.where(keep, la, fold(a))
        vx, vy = vpx0 + rng.uniform(-1e-3, 1e-3, N_POINTS), vpy0 + rng.uniform(-1e-3, 1e-3, N_POINTS)
        vx[:8], vy[:8] = vpx0, vpy0
        cases.append(_case("band_%d" % q, mx, my, la, vx, vy, thre))
    # to the right of all segments
    vx, vy = 500 + 10.0 ** rng.uniform(0, 6, N_POINTS), rng.uniform(100, 300, N_POINTS)
    mx, my, la = cloud(rng, 67, vx[0], vy[0], 0.8, 0.2)
    my[::5] = vy[1]
    vy[1:40:2] = vy[1]      # (raw = +pi exactly for those segments from those points)
    la[::5] = fold(rng.uniform(-0.1, 0.1, len(la[::5])))
    cases.append(_case("right_of_all", mx, my, la, vx, vy, THRE[0]))
    # a vanishing point equal to a mid point
    mx, my, la = cloud(rng, 64, 350.0, 200.0, 0.0, 0.0)
    z = rng.integers(0, 64, N_POINTS)
    vx, vy = mx[z].copy(), my[z].copy()
    la = fold(direction(mx, my, vx[0], vy[0]) + rng.uniform(-0.2, 0.2, 64))
    la[z[:4]] = rng.uniform(-0.1, 0.1, 4)      # (atan2 of the zero vector is 0: the segment on the point is an inlier)
    cases.append(_case("on_a_mid_point", mx, my, la, vx, vy, THRE[0]))
    # non-finite vanishing points
    special = np.array([np.inf, -np.inf, np.nan])
    k = np.arange(N_POINTS)
    vx = np.where((k // 9) % 3 == 1, rng.uniform(0, 600, N_POINTS), special[k % 3])
    vy = np.where((k // 9) % 3 == 0, rng.uniform(0, 400, N_POINTS), special[(k // 3) % 3])
    mx, my, la = cloud(rng, 40, 350.0, 200.0, 0.0, 0.0)
    la[::2] = fold(np.where(rng.random(20) < 0.5, 0.0, PI / 2) + np.where(rng.random(20) < 0.5, 0.0, rng.uniform(-0.2, 0.2, 20)))
    cases.append(_case("nonfinite", mx, my, la, vx, vy, THRE[0]))
    # no inlier; exactly one
    for one in (False, True):
        vpx0, vpy0 = 900.0, -250.0
        mx, my, _ = cloud(rng, 65, vpx0, vpy0, 0.0, 0.0)
        la = fold(direction(mx, my, vpx0, vpy0) + np.where(rng.random(65) < 0.5, -1.0, 1.0) * rng.uniform(THRE[0] + 0.05, PI / 2, 65))
        if one:
            la[41] = fold(direction(mx[41], my[41], vpx0, vpy0) + 0.05)
        ang = rng.uniform(0, 2 * PI, N_POINTS)
        vx, vy = vpx0 + rng.uniform(0, 5, N_POINTS) * np.cos(ang), vpy0 + rng.uniform(0, 5, N_POINTS) * np.sin(ang)      # (5 px at 700 px: directions move by < 0.01 rad)
        cases.append(_case("one_inlier" if one else "no_inlier", mx, my, la, vx, vy, THRE[0]))
    return cases


def statement(case, swapped=False, clearance=1e-6):
    """The reference's loop in float64 numpy, per point: (angles (n, 2), clear (n,)).  clear[p]: every decision of point p -- the inlier tests, the
    unwrap tests against +-pi, the gap between the best and the second-best unwrapped angle at both ends -- keeps `clearance` rad from its
    threshold, so that numpy's arctan2 and cs_atan2 (which agree to an ulp) decide alike.  Only those points are compared."""
    mx, my, la, thre = case["mx"], case["my"], case["la"], case["thre"]
    n = len(case["vpx"])
    out, clear = np.full((n, 2), np.nan), np.zeros(n, bool)
    for p in range(n):
        with np.errstate(invalid="ignore"):
            raw = np.arctan2(my - case["vpy"][p], mx - case["vpx"][p])
            d = np.abs(la - fold(raw))
            d = np.minimum(d, PI - d)
            inl = d < thre
            margin = np.min(np.abs(d - thre)) if len(d) else np.inf
            idx = np.nonzero(inl)[0]
            if len(idx):
                r = raw[idx]
                diff = r - r[0]
                sh = np.where(diff < -PI, r + 2 * PI, np.where(diff > PI, r - 2 * PI, r))
                margin = min(margin, np.min(np.abs(np.abs(diff) - PI)))
                hi, lo = la[idx[np.argmax(sh)]], la[idx[np.argmin(sh)]]      # (argmax / argmin: the first occurrence)
                out[p] = (lo, hi) if swapped else (hi, lo)
                if len(idx) > 1:
                    s = np.sort(sh)
                    margin = min(margin, s[-1] - s[-2], s[1] - s[0])
            clear[p] = bool(margin >= clearance)
    return out, clear
