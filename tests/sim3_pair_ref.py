"""numpy statement of the Sim(3) alignment of one keyframe pair (cs_sim3_*): ORB-SLAM2's Optimizer::OptimizeSim3 over g2o's
VertexSim3Expmap, EdgeSim3ProjectXYZ and EdgeInverseSim3ProjectXYZ (types/types_seven_dof_expmap.h:48-171) with BaseBinaryEdge's numeric
Jacobians (core/base_binary_edge.hpp:130-205), RobustKernelHuber with its single-precision delta^2 and OptimizationAlgorithmLevenberg
(core/optimization_algorithm_levenberg.cpp:61-189) over a 7 x 7 LDL^T without pivoting.

Generic in dtype: the same code runs in float64 and in np.longdouble; the Sim3 functions are tests/pgo_ref.py's.  A pair is solved with
its matches as the leading axis; the 15 states of a linearisation are one more axis in front of it."""
import numpy as np

import pgo_ref as pr

DELTA = pr.DELTA
MAX_TRIALS = 10

DEFAULTS = dict(iterations_first=5, iterations_more_clean=5, iterations_more_outliers=10, th2=10.0, huber_delta=None, robust_second_round=1, min_inliers=10)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    if p["huber_delta"] is None:
        p["huber_delta"] = float(np.sqrt(np.float64(p["th2"])))
    return p


def pair_of(batch, f, dtype=np.float64):
    """Pair f of a synth_sim3_pairs batch, in `dtype`."""
    a, b = int(batch["match_ptr"][f]), int(batch["match_ptr"][f + 1])
    c = lambda k: np.array(batch[k][a:b], dtype=dtype)
    n = b - a
    eye = np.tile(np.array([1, 0, 0, 1], dtype=dtype), (n, 1))
    return dict(S=np.array(batch["S12"][f], dtype=dtype), intr=np.array(batch["intr"][f], dtype=dtype), fix_scale=bool(batch["fix_scale"][f]), n=n,
                P1=c("P1"), P2=c("P2"), obs1=c("obs1"), obs2=c("obs2"),
                W12=(c("info12") if batch.get("info12") is not None else eye).reshape(n, 2, 2), W21=(c("info21") if batch.get("info21") is not None else eye).reshape(n, 2, 2))


def _project(T, P, obs, K):
    """obs - cam_map(project(T.map(P))); T (..., 8) broadcasts against P (n, 3)."""
    pc = pr.sim3_map(T[..., None, :], P)
    return np.stack([obs[..., 0] - (pc[..., 0] / pc[..., 2] * K[0] + K[2]), obs[..., 1] - (pc[..., 1] / pc[..., 2] * K[1] + K[3])], -1)


def errors(p, S):
    """e12, e21 (each (..., n, 2)) at the state(s) S (..., 8)."""
    return _project(S, p["P2"], p["obs1"], p["intr"][:4]), _project(pr.sim3_inv(S), p["P1"], p["obs2"], p["intr"][4:])


def chi2_each(W, e):
    We = np.stack([W[..., 0, 0] * e[..., 0] + W[..., 0, 1] * e[..., 1], W[..., 1, 0] * e[..., 0] + W[..., 1, 1] * e[..., 1]], -1)
    return e[..., 0] * We[..., 0] + e[..., 1] * We[..., 1], We


def huber(c, delta):
    """RobustKernelHuber::robustify with `float dsqr` (cs_robust.h: huber_rho); delta <= 0: no kernel."""
    if not delta > 0:
        return c, np.ones_like(c)
    T = c.dtype.type
    d = T(delta)
    dsqr = T(np.float32(d * d))
    with np.errstate(all="ignore"):
        sq = np.sqrt(c)
        inl = c <= dsqr
        return np.where(inl, c, 2 * sq * d - dsqr), np.where(inl, T(1), d / sq)


def states(S, fix_scale):
    """(15, 8): S, then S (+) +delta e_d and S (+) -delta e_d for d = 0 .. 6."""
    u = np.zeros((14, 7), S.dtype)
    for d in range(7):
        u[2 * d, d] = S.dtype.type(DELTA)
        u[2 * d + 1, d] = -S.dtype.type(DELTA)
    return np.concatenate([S[None], pr.sim3_oplus(S[None], u, fix_scale)], 0)


def linearize(p, S):
    """e12, e21 (n, 2) and J12, J21 (n, 2, 7) at S."""
    T = S.dtype.type
    scalar = 1 / (2 * T(DELTA))
    e12, e21 = errors(p, states(S, p["fix_scale"]))
    J12 = np.moveaxis(scalar * (e12[1::2] - e12[2::2]), 0, -1)
    J21 = np.moveaxis(scalar * (e21[1::2] - e21[2::2]), 0, -1)
    return e12[0], e21[0], J12, J21


def active_chi2(p, S, act, delta):
    e12, e21 = errors(p, S)
    c12, c21 = chi2_each(p["W12"], e12)[0], chi2_each(p["W21"], e21)[0]
    return (huber(c12[act], delta)[0] + huber(c21[act], delta)[0]).sum()


def build_system(p, S, act, delta):
    e12, e21, J12, J21 = linearize(p, S)
    H = np.zeros((7, 7), S.dtype)
    b = np.zeros(7, S.dtype)
    chi = S.dtype.type(0)
    for e, J, W in ((e12, J12, p["W12"]), (e21, J21, p["W21"])):
        e, J, W = e[act], J[act], W[act]
        c, We = chi2_each(W, e)
        r0, r1 = huber(c, delta)
        chi = chi + r0.sum()
        WJ = r1[:, None, None] * (W @ J)
        H = H + (np.swapaxes(J, 1, 2) @ WJ).sum(0)
        b = b - (r1[:, None] * (np.swapaxes(J, 1, 2) @ We[..., None])[..., 0]).sum(0)
    return H, b, chi


def solve7(A, b):
    """LDL^T without pivoting; None when a pivot is not positive (solvers/linear_solver_dense.h:104-111)."""
    n = len(b)
    L = np.zeros_like(A)
    D = np.zeros_like(b)
    for j in range(n):
        d = A[j, j] - (L[j, :j] * L[j, :j] * D[:j]).sum()
        if not d > 0:
            return None
        D[j] = d
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * D[:j]).sum()) / d
    y = np.zeros_like(b)
    for i in range(n):
        y[i] = b[i] - (L[i, :i] * y[:i]).sum()
    y = y / D
    x = np.zeros_like(b)
    for i in range(n - 1, -1, -1):
        x[i] = y[i] - (L[i + 1:, i] * x[i + 1:]).sum()
    return x


def lm_round(p, S, act, delta, iterations):
    """SparseOptimizer::optimize(iterations) on the active matches, from S -> (S, iterations_done, trials per iteration, rhos, chi2)."""
    T = S.dtype.type
    if iterations <= 0:
        return S, 0, [], [], active_chi2(p, S, act, delta)
    lam, ni, n_bad, done = T(0), T(2), 0, 0
    trials, rhos = [], []
    current = T(0)
    for it in range(iterations):
        H, b, current = build_system(p, S, act, delta)
        ini = current
        if it == 0:
            lam = T(1e-5) * np.abs(np.diag(H)).max()
            ni, n_bad = T(2), 0
        rho, qmax = T(0), 0
        while True:
            x = solve7(H + lam * np.eye(7, dtype=S.dtype), b)
            if x is None:
                temp, scale, Sn = T(np.finfo(np.float64).max), T(0), S
            else:
                Sn = pr.sim3_oplus(S[None], x[None], p["fix_scale"])[0]
                temp = active_chi2(p, Sn, act, delta)
                scale = (x * (lam * x + b)).sum()
            rho = (current - temp) / (scale + T(1e-3))
            rhos.append(float(rho))
            if rho > 0 and np.isfinite(temp):
                alpha = min(1 - (2 * rho - 1) ** 3, T(2) / 3)
                lam = lam * max(T(1) / 3, alpha)
                ni = T(2)
                current = temp
                S = Sn
            else:
                lam = lam * ni
                ni = ni * 2
            qmax += 1
            if not (rho < 0 and qmax < MAX_TRIALS):
                break
        trials.append(qmax)
        done += 1
        if qmax == MAX_TRIALS or rho == 0:
            break
        n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
        if n_bad >= 3:
            break
    return S, done, trials, rhos, current


def classify(p, S, act, th2):
    """-> (flags, margin): an active match with e^T Omega e > th2 on either edge goes; margin = the smallest |chi2 / th2 - 1| met."""
    e12, e21 = errors(p, S)
    c12, c21 = chi2_each(p["W12"], e12)[0], chi2_each(p["W21"], e21)[0]
    T = S.dtype.type
    keep = act & ~((c12 > T(th2)) | (c21 > T(th2)))
    both = np.concatenate([c12[act], c21[act]])
    margin = float(np.abs(both / T(th2) - 1).min()) if len(both) else np.inf
    return keep, margin


def optimize_pair(p, prm):
    """Optimizer::OptimizeSim3 for one pair -> dict: S, iterations (2), trials (2 lists), rhos (2 lists), chi2 (2), inlier, n_inliers, margin."""
    S = p["S"].copy()
    act = np.ones(p["n"], bool)
    out = dict(iterations=[0, 0], trials=[[], []], rhos=[[], []], chi2=[S.dtype.type(0), S.dtype.type(0)], margin=np.inf)
    left = p["n"]
    for r in range(2):
        delta = prm["huber_delta"] if (r == 0 or prm["robust_second_round"]) else 0.0
        iterations = prm["iterations_first"] if r == 0 else (prm["iterations_more_outliers"] if left < p["n"] else prm["iterations_more_clean"])
        if left > 0:
            S, out["iterations"][r], out["trials"][r], out["rhos"][r], out["chi2"][r] = lm_round(p, S, act, delta, iterations)
        act, m = classify(p, S, act, prm["th2"])
        out["margin"] = min(out["margin"], m)
        left = int(act.sum())
        if r == 0 and left < prm["min_inliers"]:
            act = np.zeros(p["n"], bool)
            left = 0
            break
    out.update(S=S, inlier=act.astype(np.uint8), n_inliers=left)
    return out


def optimize_batch(batch, prm, dtype=np.float64, pairs=None):
    idx = range(len(batch["S12"])) if pairs is None else pairs
    return [optimize_pair(pair_of(batch, f, dtype), prm) for f in idx]


def min_abs_rho(res):
    v = [abs(x) for r in res for rr in r["rhos"] for x in rr]
    return min(v) if v else np.inf


def block_deviation(a, b):
    """Per match: the largest difference against the largest entry of b's block (blocks = everything behind the leading axis)."""
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return (np.abs(a - b).max(-1) / np.abs(b).max(-1)).astype(np.float64)
