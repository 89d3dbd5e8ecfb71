"""The numpy statement of the two-view triangulation of new map points (cube_slam_wu_amd/csrc/cs_triangulate.h, whose top comment it
follows line by line), in float64 or in long double: the same Jacobi pair order and sweep count, the same order of tests, every sum left
to right.  Vectorised over the matches of a batch; nothing here is fused.  run() returns every decision quantity beside the outcome, and
the list of threshold comparisons it made with the difference each one decided on."""
import numpy as np

OK, PAIR_NOT_RUN, LOW_PARALLAX, W_ZERO, DEPTH1, DEPTH2, REPROJ1, REPROJ2, ZERO_DIST, SCALE = range(10)
STATUS_NAMES = ("OK", "PAIR_NOT_RUN", "LOW_PARALLAX", "W_ZERO", "DEPTH1", "DEPTH2", "REPROJ1", "REPROJ2", "ZERO_DIST", "SCALE")
ROUTE_NONE, TRIANGULATED, STEREO1, STEREO2 = range(4)
SWEEPS = 8
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
PARAM_KEYS = ("min_baseline_ratio", "max_cos_parallax", "chi2_mono", "chi2_stereo", "ratio_factor", "scale_range")


def params(**kw):
    p = dict(min_baseline_ratio=0.01, max_cos_parallax=0.9998, chi2_mono=5.991, chi2_stereo=7.8, ratio_factor=1.5 * 1.2, scale_range=1.2 * 1.2 * 1.2 * 1.2 * 1.2 * 1.2 * 1.2)
    p.update(kw)
    return p


def camera(Tcw, dt):
    """R (n, 3, 3), t (n, 3), O (n, 3) of poses (n, 7)."""
    T = np.asarray(Tcw, np.float64).astype(dt)
    n = np.sqrt(T[:, 3] * T[:, 3] + T[:, 4] * T[:, 4] + T[:, 5] * T[:, 5] + T[:, 6] * T[:, 6])
    x, y, z, w = T[:, 3] / n, T[:, 4] / n, T[:, 5] / n, T[:, 6] / n
    one, two = dt(1), dt(2)
    R = np.empty((len(T), 3, 3), dt)
    R[:, 0, 0] = one - two * (y * y + z * z); R[:, 0, 1] = two * (x * y - w * z); R[:, 0, 2] = two * (x * z + w * y)
    R[:, 1, 0] = two * (x * y + w * z); R[:, 1, 1] = one - two * (x * x + z * z); R[:, 1, 2] = two * (y * z - w * x)
    R[:, 2, 0] = two * (x * z - w * y); R[:, 2, 1] = two * (y * z + w * x); R[:, 2, 2] = one - two * (x * x + y * y)
    t = T[:, :3].copy()
    O = np.stack([-(R[:, 0, i] * t[:, 0] + R[:, 1, i] * t[:, 1] + R[:, 2, i] * t[:, 2]) for i in range(3)], axis=1)
    return R, t, O


def _back(R, x):
    """R^T x"""
    return np.stack([R[:, 0, i] * x[:, 0] + R[:, 1, i] * x[:, 1] + R[:, 2, i] * x[:, 2] for i in range(3)], axis=1)


def _to_camera(R, t, X):
    return np.stack([(R[:, i, 0] * X[:, 0] + R[:, i, 1] * X[:, 1] + R[:, i, 2] * X[:, 2]) + t[:, i] for i in range(3)], axis=1)


def _norm3(v):
    return np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1] + v[:, 2] * v[:, 2])


def _col(a, j):
    return a[:, 0, j] * a[:, 0, j] + a[:, 1, j] * a[:, 1, j] + a[:, 2, j] * a[:, 2, j] + a[:, 3, j] * a[:, 3, j]


def smallest_singular_vector(a):
    """a: (n, 4, 4), used up.  -> (n, 4): one-sided Jacobi on the columns."""
    dt = a.dtype.type
    v = np.zeros_like(a)
    for i in range(4):
        v[:, i, i] = dt(1)
    for _ in range(SWEEPS):
        for p, q in PAIRS:
            alpha, beta = _col(a, p), _col(a, q)
            gamma = a[:, 0, p] * a[:, 0, q] + a[:, 1, p] * a[:, 1, q] + a[:, 2, p] * a[:, 2, q] + a[:, 3, p] * a[:, 3, q]
            skip = gamma == 0
            zeta = (beta - alpha) / np.where(skip, dt(1), dt(2) * gamma)
            r = dt(1) / (np.abs(zeta) + np.sqrt(zeta * zeta + dt(1)))
            t = np.where(skip, dt(0), np.where(zeta < 0, -r, r))
            c = dt(1) / np.sqrt(t * t + dt(1))
            s = t * c
            for m in (a, v):
                g, h = m[:, :, p].copy(), m[:, :, q].copy()
                m[:, :, p] = c[:, None] * g - s[:, None] * h
                m[:, :, q] = s[:, None] * g + c[:, None] * h
    best = _col(a, 0)
    h4 = v[:, :, 0].copy()
    for k in range(1, 4):
        nk = _col(a, k)
        down = nk < best
        best = np.where(down, nk, best)
        h4 = np.where(down[:, None], v[:, :, k], h4)
    return h4


def dehomogenize(h4):
    """-> X (n, 3), ok (n)"""
    with np.errstate(all="ignore"):
        X = h4[:, :3] / h4[:, 3:4]
    return X, (h4[:, 3] != 0) & np.isfinite(X.astype(np.float64)).all(axis=1)


def _cos_stereo(d, b):
    q = (b * b) * d.dtype.type(0.25)
    return (d * d - q) / (d * d + q)


def pair_records(batch, prm, dt=np.float64):
    """Per pair: R, t, O of both cameras, baseline and ran; `pair_cmp` the difference its eligibility comparison decided on."""
    R1, t1, O1 = camera(batch["Tcw1"], dt)
    R2, t2, O2 = camera(batch["Tcw2"], dt)
    d = O2 - O1
    baseline = _norm3(d)
    md = np.asarray(batch["median_depth2"], np.float64).astype(dt)
    b2 = np.asarray(batch["cam2"], np.float64).astype(dt)[:, 5]
    mono = md > 0
    with np.errstate(all="ignore"):
        diff = np.where(mono, baseline / np.where(mono, md, dt(1)) - dt(prm["min_baseline_ratio"]), baseline - b2)
    return dict(R1=R1, t1=t1, O1=O1, R2=R2, t2=t2, O2=O2, baseline=baseline, ran=~(diff < 0), pair_cmp=diff)


def run(batch, prm=None, dt=np.float64):
    """-> dict over the batch's N matches: status, route, X, normal, min_distance, max_distance, cosRays, cosS1, cosS2, and per pair ran and
    n_accepted; `comparisons`: a list of (name, made (N, bool), diff (N)) -- every threshold comparison of the statement, on which matches
    it was reached, and lhs - rhs as it was computed; `pair_cmp` (n) the same for the pair's eligibility."""
    prm = params() if prm is None else prm
    dt = np.dtype(dt).type
    P = pair_records(batch, prm, dt)
    ptr = np.asarray(batch["match_ptr"])
    n, N = len(ptr) - 1, int(ptr[-1])
    pm = np.repeat(np.arange(n), np.diff(ptr))
    R1, t1, O1, R2, t2, O2 = (P[k][pm] for k in ("R1", "t1", "O1", "R2", "t2", "O2"))
    cam1, cam2 = np.asarray(batch["cam1"], np.float64).astype(dt)[pm], np.asarray(batch["cam2"], np.float64).astype(dt)[pm]
    k1, k2 = np.asarray(batch["kp1"], np.float64).astype(dt).reshape(N, 6), np.asarray(batch["kp2"], np.float64).astype(dt).reshape(N, 6)
    ran = P["ran"][pm]
    one = dt(1)
    comparisons = []
    with np.errstate(all="ignore"):
        # 1 rays and parallax
        xn1 = np.stack([(k1[:, 0] - cam1[:, 2]) / cam1[:, 0], (k1[:, 1] - cam1[:, 3]) / cam1[:, 1], np.full(N, one)], axis=1)
        xn2 = np.stack([(k2[:, 0] - cam2[:, 2]) / cam2[:, 0], (k2[:, 1] - cam2[:, 3]) / cam2[:, 1], np.full(N, one)], axis=1)
        ray1, ray2 = _back(R1, xn1), _back(R2, xn2)
        dot = ray1[:, 0] * ray2[:, 0] + ray1[:, 1] * ray2[:, 1] + ray1[:, 2] * ray2[:, 2]
        cosRays = dot / (_norm3(ray1) * _norm3(ray2))
        st1, st2 = k1[:, 2] >= 0, k2[:, 2] >= 0
        cosS1 = np.where(st1, _cos_stereo(k1[:, 3], cam1[:, 5]), cosRays + one)
        cosS2 = np.where(~st1 & st2, _cos_stereo(k2[:, 3], cam2[:, 5]), cosRays + one)      # (the else is ORB-SLAM2's own)
        cosS = np.where(cosS2 < cosS1, cosS2, cosS1)
        # 2 route
        c_a, c_b = cosRays < cosS, cosRays > 0
        c_c = st1 | st2 | (cosRays < dt(prm["max_cos_parallax"]))
        tri = ran & c_a & c_b & c_c
        comparisons.append(("cosRays < cosS", ran, cosRays - cosS))
        comparisons.append(("cosRays > 0", ran & c_a, cosRays))
        comparisons.append(("cosRays < max_cos_parallax", ran & c_a & c_b & ~st1 & ~st2, cosRays - dt(prm["max_cos_parallax"])))
        s1 = ran & ~tri & st1 & (cosS1 < cosS2)
        comparisons.append(("cosS1 < cosS2", ran & ~tri & st1, cosS1 - cosS2))
        s2 = ran & ~tri & ~s1 & st2 & (cosS2 < cosS1)
        comparisons.append(("cosS2 < cosS1", ran & ~tri & ~s1 & st2, cosS2 - cosS1))
        route = np.where(tri, TRIANGULATED, np.where(s1, STEREO1, np.where(s2, STEREO2, ROUTE_NONE)))
        a = np.empty((N, 4, 4), dt)
        T1 = np.concatenate([R1, t1[:, :, None]], axis=2)      # (N, 3, 4)
        T2 = np.concatenate([R2, t2[:, :, None]], axis=2)
        for j in range(4):
            a[:, 0, j] = xn1[:, 0] * T1[:, 2, j] - T1[:, 0, j]
            a[:, 1, j] = xn1[:, 1] * T1[:, 2, j] - T1[:, 1, j]
            a[:, 2, j] = xn2[:, 0] * T2[:, 2, j] - T2[:, 0, j]
            a[:, 3, j] = xn2[:, 1] * T2[:, 2, j] - T2[:, 1, j]
        Xt, w_ok = dehomogenize(smallest_singular_vector(a))

        def unproject(R, O, cam, k):
            x = np.stack([(k[:, 0] - cam[:, 2]) * k[:, 3] / cam[:, 0], (k[:, 1] - cam[:, 3]) * k[:, 3] / cam[:, 1], k[:, 3]], axis=1)
            return _back(R, x) + O

        X = np.where(tri[:, None], Xt, np.where(s1[:, None], unproject(R1, O1, cam1, k1), unproject(R2, O2, cam2, k2)))
        has_X = (tri & w_ok) | s1 | s2
        # 3 depths
        pc1, pc2 = _to_camera(R1, t1, X), _to_camera(R2, t2, X)
        z1_ok, z2_ok = pc1[:, 2] > 0, pc2[:, 2] > 0
        comparisons.append(("z1 > 0", has_X, pc1[:, 2]))
        comparisons.append(("z2 > 0", has_X & z1_ok, pc2[:, 2]))

        # 4 reprojection
        def reproj(pc, cam, k, st):
            u = cam[:, 0] * pc[:, 0] / pc[:, 2] + cam[:, 2]
            v = cam[:, 1] * pc[:, 1] / pc[:, 2] + cam[:, 3]
            ex, ey = u - k[:, 0], v - k[:, 1]
            exr = (u - cam[:, 4] / pc[:, 2]) - k[:, 2]
            e2 = ex * ex + ey * ey
            e = np.where(st, e2 + exr * exr, e2)
            th = np.where(st, dt(prm["chi2_stereo"]), dt(prm["chi2_mono"])) * k[:, 4]
            return e, th

        e1, th1 = reproj(pc1, cam1, k1, st1)
        e2, th2 = reproj(pc2, cam2, k2, st2)
        r1_ok, r2_ok = e1 <= th1, e2 <= th2
        at4 = has_X & z1_ok & z2_ok
        comparisons.append(("e1 <= th1", at4, e1 - th1))
        comparisons.append(("e2 <= th2", at4 & r1_ok, e2 - th2))
        # 5 scale consistency
        n1, n2 = X - O1, X - O2
        dist1, dist2 = _norm3(n1), _norm3(n2)
        at5 = at4 & r1_ok & r2_ok
        zero = (dist1 == 0) | (dist2 == 0)
        ratioDist, ratioOctave = dist2 / dist1, k1[:, 5] / k2[:, 5]
        rf = dt(prm["ratio_factor"])
        lo, hi = ratioDist * rf < ratioOctave, ratioDist > ratioOctave * rf
        comparisons.append(("ratioDist * ratio_factor < ratioOctave", at5 & ~zero, ratioDist * rf - ratioOctave))
        comparisons.append(("ratioDist > ratioOctave * ratio_factor", at5 & ~zero & ~lo, ratioDist - ratioOctave * rf))
        ok = at5 & ~zero & ~lo & ~hi
        # 6 accepted
        normal = (n1 / dist1[:, None] + n2 / dist2[:, None]) / dt(2)
        max_distance = dist1 * k1[:, 5]
        min_distance = max_distance / dt(prm["scale_range"])

    status = np.full(N, OK, np.int64)
    for cond, code in ((at5 & ~zero & ~lo & hi, SCALE), (at5 & ~zero & lo, SCALE), (at5 & zero, ZERO_DIST), (at4 & r1_ok & ~r2_ok, REPROJ2), (at4 & ~r1_ok, REPROJ1),
                       (has_X & z1_ok & ~z2_ok, DEPTH2), (has_X & ~z1_ok, DEPTH1), (tri & ~w_ok, W_ZERO), (ran & (route == ROUTE_NONE), LOW_PARALLAX), (~ran, PAIR_NOT_RUN)):
        status[cond] = code
    assert np.array_equal(status == OK, ok)
    z = dt(0)
    out = dict(status=status, route=np.where(ran, route, ROUTE_NONE).astype(np.int64),
               X=np.where(has_X[:, None], X, z), normal=np.where(ok[:, None], normal, z), min_distance=np.where(ok, min_distance, z), max_distance=np.where(ok, max_distance, z),
               cosRays=np.where(ran, cosRays, z), cosS1=np.where(ran, cosS1, z), cosS2=np.where(ran, cosS2, z),
               ran=P["ran"].astype(np.uint8), n_accepted=np.array([int(ok[ptr[f]:ptr[f + 1]].sum()) for f in range(n)], np.int64),
               comparisons=comparisons, pair_cmp=P["pair_cmp"], pair_of_match=pm, e1=e1, e2=e2)
    return out


def scale_stage(O1, O2, scale1, scale2, X, prm=None):
    """Steps 5 and 6 alone at the point X, in float64 -> (status, normal, min_distance, max_distance)."""
    prm = params() if prm is None else prm
    O1, O2, X = (np.asarray(v, np.float64) for v in (O1, O2, X))
    n1, n2 = X - O1, X - O2
    d1 = np.sqrt(n1[0] * n1[0] + n1[1] * n1[1] + n1[2] * n1[2])
    d2 = np.sqrt(n2[0] * n2[0] + n2[1] * n2[1] + n2[2] * n2[2])
    if d1 == 0 or d2 == 0:
        return ZERO_DIST, np.zeros(3), 0.0, 0.0
    rd, ro = d2 / d1, scale1 / scale2
    if rd * prm["ratio_factor"] < ro or rd > ro * prm["ratio_factor"]:
        return SCALE, np.zeros(3), 0.0, 0.0
    return OK, (n1 / d1 + n2 / d2) / 2.0, d1 * scale1 / prm["scale_range"], d1 * scale1
