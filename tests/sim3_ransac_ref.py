"""numpy statement of the Sim(3) RANSAC of one keyframe pair (cs_sim3_ransac_*): ORB-SLAM2's Sim3Solver -- SetRansacParameters, iterate
called until it succeeds or says bNoMore, ComputeSim3 (Horn 1987), CheckInliers -- as include/cubeslam_hip.h states it.

Generic in dtype: the same code runs in float64 and in np.longdouble.  The draws come from real lists (take a position, overwrite it with
the last entry, pop), the eigenvector from this file's own cyclic Jacobi, and the hypotheses are evaluated one at a time in the solver's
order; a hypothesis is tested against a pair's matches as one array."""
import math

import numpy as np

GOLDEN = 0x9E3779B97F4A7C15
MASK = (1 << 64) - 1
SWEEPS = 12
IDENTITY = (0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)

DEFAULTS = dict(probability=0.99, min_inliers=20, max_iterations=300)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def splitmix64(z):
    z &= MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw(seed, h, n):
    """The three matches of hypothesis h, from the list."""
    avail, out = list(range(n)), []
    for k in range(3):
        r = splitmix64(int(seed) + (3 * h + k) * GOLDEN) % len(avail)
        out.append(avail[r])
        avail[r] = avail[-1]
        avail.pop()
    return out


def budget(n, probability, min_inliers, max_iterations):
    """max_its of a pair of n matches; 0: the pair is not run."""
    if n < max(3, min_inliers):
        return 0
    eps = min_inliers / n
    if eps >= 1:
        its = 1
    else:
        den = math.log(1.0 - eps * eps * eps)
        its = max_iterations if den == 0.0 else min(math.ceil(math.log(1.0 - probability) / den), max_iterations)
    return max(1, min(its, max_iterations))


def pair_of(batch, f, dtype=np.float64):
    """Pair f of a synth_sim3_ransac batch, in `dtype`."""
    a, b = int(batch["match_ptr"][f]), int(batch["match_ptr"][f + 1])
    c = lambda k: np.array(batch[k][a:b], dtype=dtype)
    return dict(intr=np.array(batch["intr"][f], dtype=dtype), fix_scale=bool(batch["fix_scale"][f]), seed=int(batch["seed"][f]), n=b - a,
                P1=c("P1"), P2=c("P2"), th1=c("max_err1"), th2=c("max_err2"))


def project(P, K):
    with np.errstate(all="ignore"):
        iz = P.dtype.type(1) / P[..., 2]
        return np.stack([K[0] * P[..., 0] * iz + K[2], K[1] * P[..., 1] * iz + K[3]], -1)


def top_eigenvector(N):
    """(w, x, y, z): the unit eigenvector of the largest eigenvalue of the symmetric 4 x 4 N, by SWEEPS cyclic Jacobi sweeps, sign fixed."""
    T = N.dtype.type
    a = [[T(N[i, j]) for j in range(4)] for i in range(4)]
    v = [[T(1) if i == j else T(0) for j in range(4)] for i in range(4)]
    one = T(1)
    for _ in range(SWEEPS):
        for p in range(3):
            for q in range(p + 1, 4):
                apq = a[p][q]
                if apq == 0:
                    continue
                theta = (a[q][q] - a[p][p]) / (T(2) * apq)
                with np.errstate(over="ignore"):
                    r = one / (abs(theta) + np.sqrt(theta * theta + one))
                t = -r if theta < 0 else r
                c = one / np.sqrt(t * t + one)
                s = t * c
                tau = s / (one + c)
                a[p][p] = a[p][p] - t * apq
                a[q][q] = a[q][q] + t * apq
                a[p][q] = a[q][p] = T(0)
                for k in range(4):
                    if k != p and k != q:
                        g, hq = a[k][p], a[k][q]
                        a[k][p] = a[p][k] = g - s * (hq + g * tau)
                        a[k][q] = a[q][k] = hq + s * (g - hq * tau)
                for k in range(4):
                    g, hq = v[k][p], v[k][q]
                    v[k][p] = g - s * (hq + g * tau)
                    v[k][q] = hq + s * (g - hq * tau)
    k = 0
    for j in range(1, 4):
        if a[j][j] > a[k][k]:
            k = j
    q = np.array([v[i][k] for i in range(4)], dtype=N.dtype)
    q = q * (one / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]))
    nz = [x for x in q if x != 0]
    return -q if nz and nz[0] < 0 else q


def rotation(q):
    w, x, y, z = q
    two, one = q.dtype.type(2), q.dtype.type(1)
    return np.array([[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
                     [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
                     [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]], dtype=q.dtype)


def hypothesis(X1, X2, fix_scale):
    """Horn's alignment of three matches (rows of X1 / X2) -> (q (w, x, y, z), t, s), or None when it is refused."""
    T = X1.dtype.type
    O1, O2 = (X1[0] + X1[1] + X1[2]) / T(3), (X2[0] + X2[1] + X2[2]) / T(3)
    Pr1, Pr2 = X1 - O1, X2 - O2
    M = np.array([[Pr2[0, i] * Pr1[0, j] + Pr2[1, i] * Pr1[1, j] + Pr2[2, i] * Pr1[2, j] for j in range(3)] for i in range(3)], dtype=X1.dtype)
    N = np.zeros((4, 4), dtype=X1.dtype)
    N[0, 0] = M[0, 0] + M[1, 1] + M[2, 2]; N[0, 1] = M[1, 2] - M[2, 1]; N[0, 2] = M[2, 0] - M[0, 2]; N[0, 3] = M[0, 1] - M[1, 0]
    N[1, 1] = M[0, 0] - M[1, 1] - M[2, 2]; N[1, 2] = M[0, 1] + M[1, 0]; N[1, 3] = M[2, 0] + M[0, 2]
    N[2, 2] = -M[0, 0] + M[1, 1] - M[2, 2]; N[2, 3] = M[1, 2] + M[2, 1]
    N[3, 3] = -M[0, 0] - M[1, 1] + M[2, 2]
    for i in range(4):
        for j in range(i):
            N[i, j] = N[j, i]
    with np.errstate(all="ignore"):
        q = top_eigenvector(N)
        R = rotation(q)
        s = T(1)
        if not fix_scale:
            nom, den = T(0), T(0)
            for k in range(3):
                for i in range(3):
                    p3 = R[i, 0] * Pr2[k, 0] + R[i, 1] * Pr2[k, 1] + R[i, 2] * Pr2[k, 2]
                    nom = nom + Pr1[k, i] * p3
                    den = den + p3 * p3
            s = nom / den
        t = np.array([O1[i] - s * (R[i, 0] * O2[0] + R[i, 1] * O2[1] + R[i, 2] * O2[2]) for i in range(3)], dtype=X1.dtype)
    if not (s > 0 and np.isfinite(s)):
        return None
    return q, t, s


def _map(A, b, P):
    return np.stack([A[i, 0] * P[:, 0] + A[i, 1] * P[:, 1] + A[i, 2] * P[:, 2] + b[i] for i in range(3)], -1)


def errors(p, hyp):
    """The two squared errors of every match of the pair against a hypothesis."""
    q, t, s = hyp
    T = q.dtype.type
    R = rotation(q)
    with np.errstate(all="ignore"):
        A12, A21 = s * R, R.T * (T(1) / s)
        b21 = np.array([-(A21[i, 0] * t[0] + A21[i, 1] * t[1] + A21[i, 2] * t[2]) for i in range(3)], dtype=q.dtype)
        p1, p2 = project(p["P1"], p["intr"][:4]), project(p["P2"], p["intr"][4:])
        d1 = p1 - project(_map(A12, t, p["P2"]), p["intr"][:4])
        d2 = p2 - project(_map(A21, b21, p["P1"]), p["intr"][4:])
        return d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1], d2[:, 0] * d2[:, 0] + d2[:, 1] * d2[:, 1]


def inliers(p, e1, e2):
    with np.errstate(invalid="ignore"):
        return (e1 < p["th1"]) & (e2 < p["th2"])


def evaluate(p, h):
    """Hypothesis h of the pair -> (hyp or None, e1, e2, inlier flags)."""
    idx = draw(p["seed"], h, p["n"])
    hyp = hypothesis(p["P1"][idx], p["P2"][idx], p["fix_scale"])
    if hyp is None:
        return None, None, None, np.zeros(p["n"], bool)
    e1, e2 = errors(p, hyp)
    return hyp, e1, e2, inliers(p, e1, e2)


def s12_of(hyp, dtype=np.float64):
    if hyp is None:
        return np.array(IDENTITY, dtype=dtype)
    q, t, s = hyp
    return np.array([q[1], q[2], q[3], q[0], t[0], t[1], t[2], s], dtype=dtype)


def run_pair(p, prm, trace=None):
    """Sim3Solver::iterate's sequential selection.  trace: a list that receives (h, hyp, e1, e2, flags) of every hypothesis evaluated."""
    max_its = budget(p["n"], prm["probability"], prm["min_inliers"], prm["max_iterations"])
    res = dict(found=0, hyp=-1, iterations=max_its, n_inliers=0, S12=s12_of(None, p["P1"].dtype), inlier=np.zeros(p["n"], np.uint8), max_its=max_its, counts=[])
    best, best_count, best_flags = None, 0, None
    for h in range(max_its):
        hyp, e1, e2, fl = evaluate(p, h)
        if trace is not None:
            trace.append((h, hyp, e1, e2, fl))
        res["counts"].append(-1 if hyp is None else int(fl.sum()))
        if hyp is None:
            continue
        count = int(fl.sum())
        if count >= best_count:
            best, best_count, best_flags = hyp, count, fl
            res["hyp"] = h
            if count > prm["min_inliers"]:
                res["found"], res["iterations"] = 1, h + 1
                break
    if best is not None:
        res.update(n_inliers=best_count, S12=s12_of(best, p["P1"].dtype), inlier=best_flags.astype(np.uint8))
    return res


def s12_deviation(a, b):
    """max |a - b| relative to the largest entry of a (per pair: the last axis)."""
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    return np.float64(np.abs(a - b).max(-1) / np.abs(a).max(-1))
