"""A float64 numpy reference of bundle adjustment over cameras and points with mono AND stereo projection edges (test infrastructure, not a
test file; nothing of the product is imported).

Restated from g2o as vendored by the reference: EdgeSE3ProjectXYZ and EdgeStereoSE3ProjectXYZ (types/types_six_dof_expmap.h:145-206,
.cpp:148-202, :233-281), the robustified quadratic form (core/base_binary_edge.hpp:54-120, robust_kernel_impl.cpp:78-165), the Schur
complement and back-substitution (core/block_solver.hpp:367-486) and the Levenberg-Marquardt loop
(core/optimization_algorithm_levenberg.cpp:61-189, sparse_optimizer.cpp:354-419).

The stereo error has single precision in exactly three places, as the reference's cam_project(trans_xyz, const float& bf) has: bf is rounded to
float on the way in, `const float invz = 1.0f / z` holds the double quotient rounded once (and is promoted again in u and v), and bf * invz is a
float product.  Both analytic Jacobians are all double; rows 0 and 1 of the stereo point Jacobian keep their own form
(-fx R(0,j) / z + fx x R(2,j) / z^2), not the mono edge's -1/z * tmp * R.

Edges live in one list, mono first, stereo behind them (g2o's edge order in the device library); a mono edge uses rows 0 and 1 of the 3-row
arrays and leaves row 2 zero, which adds exact zeros to every sum.
"""
import numpy as np

RK_NONE, RK_HUBER, RK_PSEUDO_HUBER, RK_CAUCHY = 0, 1, 2, 3


def quat_to_R(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def R_to_quat(R):
    """Eigen's Quaterniond(Matrix3d), w >= 0, normalised (SE3Quat's constructor)."""
    t = np.trace(R)
    if t > 0:
        s = np.sqrt(t + 1.0)
        w = 0.5 * s
        s = 0.5 / s
        q = np.array([(R[2, 1] - R[1, 2]) * s, (R[0, 2] - R[2, 0]) * s, (R[1, 0] - R[0, 1]) * s, w])
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q = np.zeros(4)
        q[i] = 0.5 * s
        s = 0.5 / s
        q[3] = (R[k, j] - R[j, k]) * s
        q[j] = (R[j, i] + R[i, j]) * s
        q[k] = (R[k, i] + R[i, k]) * s
    if q[3] < 0:
        q = -q
    return q / np.linalg.norm(q)


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0.0]])


def se3_exp(u):
    """SE3Quat::exp (se3quat.h:272-324): u = (omega, upsilon) -> (R, t)."""
    omega, ups = u[:3], u[3:]
    th = np.linalg.norm(omega)
    Om = skew(omega)
    Om2 = Om @ Om
    if th < 1e-5:
        R = np.eye(3) + Om + Om2
        V = R
    else:
        R = np.eye(3) + np.sin(th) / th * Om + (1 - np.cos(th)) / (th * th) * Om2
        V = np.eye(3) + (1 - np.cos(th)) / (th * th) * Om + (th - np.sin(th)) / th ** 3 * Om2
    return quat_to_R(R_to_quat(R)), V @ ups


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32)


def stereo_project(Xc, intr4, bf, double_invz=False):
    """cam_project of the stereo edge on camera-frame points Xc (n, 3) -> (u_left, v, u_right).  double_invz: the same with invz, bf and
    their product kept double (the smooth function the analytic Jacobians differentiate)."""
    if double_invz:
        invz = 1.0 / Xc[:, 2]
        ul = Xc[:, 0] * invz * intr4[:, 0] + intr4[:, 2]
        return np.stack([ul, Xc[:, 1] * invz * intr4[:, 1] + intr4[:, 3], ul - bf * invz], 1)
    invz = f32(1.0 / Xc[:, 2])                     # const float invz = 1.0f / z: the double quotient, rounded once
    invz64 = invz.astype(np.float64)
    ul = Xc[:, 0] * invz64 * intr4[:, 0] + intr4[:, 2]
    v = Xc[:, 1] * invz64 * intr4[:, 1] + intr4[:, 3]
    disp = f32(bf) * invz                          # const float& bf times float invz: a float product
    return np.stack([ul, v, ul - disp.astype(np.float64)], 1)


def robustify(kind, delta, e):
    """rho(e), rho'(e) per edge (robust_kernel_impl.cpp:78-165); Huber's delta^2 is a float member."""
    rho0, rho1 = e.copy(), np.ones_like(e)
    h = (kind == RK_HUBER) & (delta > 0)
    dsq = f32(delta * delta).astype(np.float64)
    out = h & (e > dsq)
    s = np.sqrt(e[out])
    rho0[out] = 2 * s * delta[out] - dsq[out]
    rho1[out] = delta[out] / s
    for k in (RK_PSEUDO_HUBER, RK_CAUCHY):
        m = kind == k
        d2 = delta[m] * delta[m]
        aux = (1.0 / d2) * e[m] + 1.0
        if k == RK_PSEUDO_HUBER:
            rho0[m] = 2 * d2 * (np.sqrt(aux) - 1); rho1[m] = 1.0 / np.sqrt(aux)
        else:
            rho0[m] = d2 * np.log(aux); rho1[m] = 1.0 / aux
    return rho0, rho1


class Graph:
    """mono: (pt, cam, uv (n,2), info4 (n,4), intr4 (n,4), huber (n)); stereo: (pt, cam, uvr (n,3), info9 (n,9), intr5 (n,5), huber (n));
    either may be None.  rk_mono / rk_stereo: optional (kinds, deltas) replacing the Huber deltas of the class."""

    def __init__(self, cams7, cam_fixed, points, pt_fixed, mono=None, stereo=None, rk_mono=None, rk_stereo=None):
        cams7 = np.asarray(cams7, float)
        self.R = np.array([quat_to_R(c[3:7]) for c in cams7])
        self.t = cams7[:, :3].copy()
        self.cam_fixed = np.asarray(cam_fixed).astype(bool)
        self.pt_fixed = np.asarray(pt_fixed).astype(bool)
        self.X = np.asarray(points, float).copy()
        self.nc, self.npt = len(cams7), len(self.X)
        z = lambda *s: np.zeros(s)
        m = mono if mono is not None else (np.zeros(0, int), np.zeros(0, int), z(0, 2), z(0, 4), z(0, 4), z(0))
        s = stereo if stereo is not None else (np.zeros(0, int), np.zeros(0, int), z(0, 3), z(0, 9), z(0, 5), z(0))
        nm, ns = len(m[0]), len(s[0])
        self.n_mono, self.n_stereo, self.ne = nm, ns, nm + ns
        self.e_pt = np.concatenate([np.asarray(m[0], int), np.asarray(s[0], int)])
        self.e_cam = np.concatenate([np.asarray(m[1], int), np.asarray(s[1], int)])
        self.stereo = np.concatenate([np.zeros(nm, bool), np.ones(ns, bool)])
        self.meas = np.zeros((self.ne, 3)); self.meas[:nm, :2] = np.asarray(m[2], float).reshape(-1, 2); self.meas[nm:] = np.asarray(s[2], float).reshape(-1, 3)
        self.info = np.zeros((self.ne, 3, 3)); self.info[:nm, :2, :2] = np.asarray(m[3], float).reshape(-1, 2, 2); self.info[nm:] = np.asarray(s[3], float).reshape(-1, 3, 3)
        s5 = np.asarray(s[4], float).reshape(-1, 5)
        self.intr = np.concatenate([np.asarray(m[4], float).reshape(-1, 4), s5[:, :4]])
        self.bf = np.concatenate([np.zeros(nm), s5[:, 4]])
        hub_m = np.asarray(m[5], float) if m[5] is not None else np.zeros(nm)
        hub_s = np.asarray(s[5], float) if s[5] is not None else np.zeros(ns)
        km, dm = rk_mono if rk_mono is not None else (np.where(hub_m > 0, RK_HUBER, RK_NONE), hub_m)
        ks, ds = rk_stereo if rk_stereo is not None else (np.where(hub_s > 0, RK_HUBER, RK_NONE), hub_s)
        self.rk = np.concatenate([np.asarray(km, int), np.asarray(ks, int)])
        self.delta = np.concatenate([np.asarray(dm, float), np.asarray(ds, float)])
        self.cam_col = np.full(self.nc, -1)
        self.cam_col[~self.cam_fixed] = 6 * np.arange((~self.cam_fixed).sum())
        self.n_pose = 6 * int((~self.cam_fixed).sum())
        self.lm = np.full(self.npt, -1)
        self.lm[~self.pt_fixed] = np.arange(int((~self.pt_fixed).sum()))
        self.rho_log = []          # every LM trial's gain ratio

    # ---- errors
    def camera_frame(self):
        return np.einsum("eij,ej->ei", self.R[self.e_cam], self.X[self.e_pt]) + self.t[self.e_cam]

    def errors(self, double_invz=False):
        Xc = self.camera_frame()
        e = np.zeros((self.ne, 3))
        m, s = ~self.stereo, self.stereo
        fx, fy, cx, cy = self.intr[m].T
        e[m, 0] = self.meas[m, 0] - (Xc[m, 0] / Xc[m, 2] * fx + cx)
        e[m, 1] = self.meas[m, 1] - (Xc[m, 1] / Xc[m, 2] * fy + cy)
        e[s] = self.meas[s] - stereo_project(Xc[s], self.intr[s], self.bf[s], double_invz)
        return e, Xc

    def edge_chi2(self):
        e, _ = self.errors()
        return np.einsum("ei,eij,ej->e", e, self.info, e)

    def chi2(self):
        return float(robustify(self.rk, self.delta, self.edge_chi2())[0].sum())

    compute_errors = chi2

    # ---- Jacobians (d error / d point (n, 3, 3), d error / d camera (n, 3, 6): omega, upsilon)
    def jacobians(self):
        Xc = self.camera_frame()
        x, y, z = Xc.T
        z2 = z * z
        fx, fy = self.intr[:, 0], self.intr[:, 1]
        R = self.R[self.e_cam]
        Ji = np.zeros((self.ne, 3, 3)); Jj = np.zeros((self.ne, 3, 6))
        m, s = ~self.stereo, self.stereo
        tmp = np.zeros((self.ne, 2, 3))
        tmp[:, 0, 0] = fx; tmp[:, 0, 2] = -x / z * fx
        tmp[:, 1, 1] = fy; tmp[:, 1, 2] = -y / z * fy
        Ji[m, :2] = (-1.0 / z[:, None, None] * np.einsum("eij,ejk->eik", tmp, R))[m]
        for j in range(3):
            Ji[s, 0, j] = (-fx * R[:, 0, j] / z + fx * x * R[:, 2, j] / z2)[s]
            Ji[s, 1, j] = (-fy * R[:, 1, j] / z + fy * y * R[:, 2, j] / z2)[s]
            Ji[s, 2, j] = Ji[s, 0, j] - (self.bf * R[:, 2, j] / z2)[s]
        Jj[:, 0, 0] = x * y / z2 * fx; Jj[:, 0, 1] = -(1 + x * x / z2) * fx; Jj[:, 0, 2] = y / z * fx
        Jj[:, 0, 3] = -1.0 / z * fx; Jj[:, 0, 5] = x / z2 * fx
        Jj[:, 1, 0] = (1 + y * y / z2) * fy; Jj[:, 1, 1] = -x * y / z2 * fy; Jj[:, 1, 2] = -x / z * fy
        Jj[:, 1, 4] = -1.0 / z * fy; Jj[:, 1, 5] = y / z2 * fy
        Jj[s, 2, 0] = Jj[s, 0, 0] - (self.bf * y / z2)[s]
        Jj[s, 2, 1] = Jj[s, 0, 1] + (self.bf * x / z2)[s]
        Jj[s, 2, 2] = Jj[s, 0, 2]; Jj[s, 2, 3] = Jj[s, 0, 3]
        Jj[s, 2, 5] = Jj[s, 0, 5] - (self.bf / z2)[s]
        return Ji, Jj

    # ---- linearisation + quadratic form: per-vertex blocks (Hcam (nc,6,6), bcam, Hpt (npt,3,3), bpt, Hpl (ne,6,3))
    def build(self):
        e, _ = self.errors()
        chi = np.einsum("ei,eij,ej->e", e, self.info, e)
        _, rho1 = robustify(self.rk, self.delta, chi)
        Ji, Jj = self.jacobians()
        W = rho1[:, None, None] * self.info
        omega_r = -rho1[:, None] * np.einsum("eij,ej->ei", self.info, e)
        Hcam = np.zeros((self.nc, 6, 6)); bcam = np.zeros((self.nc, 6))
        Hpt = np.zeros((self.npt, 3, 3)); bpt = np.zeros((self.npt, 3))
        Hpl = np.einsum("eki,ekl,elj->eij", Jj, W, Ji)
        np.add.at(Hcam, self.e_cam, np.einsum("eki,ekl,elj->eij", Jj, W, Jj))
        np.add.at(bcam, self.e_cam, np.einsum("eki,ek->ei", Jj, omega_r))
        np.add.at(Hpt, self.e_pt, np.einsum("eki,ekl,elj->eij", Ji, W, Ji))
        np.add.at(bpt, self.e_pt, np.einsum("eki,ek->ei", Ji, omega_r))
        Hcam[self.cam_fixed] = 0; bcam[self.cam_fixed] = 0
        Hpt[self.pt_fixed] = 0; bpt[self.pt_fixed] = 0
        Hpl[self.cam_fixed[self.e_cam] | self.pt_fixed[self.e_pt]] = 0
        self.sys = (Hcam, bcam, Hpt, bpt, Hpl)
        return self.sys

    def build_system(self):
        """(dense H_pp, H_ll (n_lm, 9), H_pl (n_edges, 18), b = [b_p, b_l]) in g2o's order, as cs_ba_get_system hands them out."""
        Hcam, bcam, Hpt, bpt, Hpl = self.build()
        n = self.n_pose
        Hpp = np.zeros((n, n))
        for c in np.nonzero(~self.cam_fixed)[0]:
            k = self.cam_col[c]
            Hpp[k:k + 6, k:k + 6] = Hcam[c]
        free = ~self.pt_fixed
        b = np.concatenate([bcam[~self.cam_fixed].ravel(), bpt[free].ravel()])
        return Hpp, Hpt[free].reshape(-1, 9), Hpl.reshape(-1, 18), b

    # ---- Schur complement and back-substitution, lambda on every diagonal
    def solve_blocks(self, lam):
        Hcam, bcam, Hpt, bpt, Hpl = self.sys
        n = self.n_pose
        S = np.zeros((n, n)); r = np.zeros(n)
        for c in range(self.nc):
            k = self.cam_col[c]
            if k >= 0:
                S[k:k + 6, k:k + 6] = Hcam[c] + lam * np.eye(6)
                r[k:k + 6] = bcam[c]
        Dinv = np.zeros((self.npt, 3, 3))
        free = ~self.pt_fixed
        Dinv[free] = np.linalg.inv(Hpt[free] + lam * np.eye(3))
        order = np.argsort(self.e_pt, kind="stable")
        bounds = np.searchsorted(self.e_pt[order], np.arange(self.npt + 1))
        for p in np.nonzero(free)[0]:
            es = order[bounds[p]:bounds[p + 1]]
            es = es[self.cam_col[self.e_cam[es]] >= 0]
            if len(es) == 0:
                continue
            cols = self.cam_col[self.e_cam[es]]
            Wp = Hpl[es].reshape(-1, 3)                        # (6 k, 3)
            WD = Wp @ Dinv[p]
            idx = (cols[:, None] + np.arange(6)[None, :]).ravel()
            S[np.ix_(idx, idx)] -= WD @ Wp.T
            r[idx] -= WD @ bpt[p]
        S = 0.5 * (S + S.T)
        try:
            np.linalg.cholesky(S)
        except np.linalg.LinAlgError:
            return False, None, None
        xp = np.linalg.solve(S, r)
        cl = bpt.copy()
        ok = self.cam_col[self.e_cam] >= 0
        np.subtract.at(cl, self.e_pt[ok], np.einsum("eij,ei->ej", Hpl[ok], xp[(self.cam_col[self.e_cam[ok]][:, None] + np.arange(6)[None, :])]))
        xl = np.einsum("pij,pj->pi", Dinv, cl)
        return True, xp, xl

    def solve(self, lam):
        ok, xp, xl = self.solve_blocks(lam)
        return (True, np.concatenate([xp, xl[~self.pt_fixed].ravel()])) if ok else (False, None)

    def update(self, xp, xl):
        for c in range(self.nc):
            k = self.cam_col[c]
            if k >= 0:
                dR, dt = se3_exp(xp[k:k + 6])
                self.t[c] = dt + dR @ self.t[c]
                self.R[c] = quat_to_R(R_to_quat(dR @ self.R[c]))      # the product is re-normalised (se3quat.h:346-351)
        self.X += xl

    # ---- OptimizationAlgorithmLevenberg::solve inside SparseOptimizer::optimize
    def optimize(self, iters):
        chi_h, lam_h, tr_h = [], [], []
        lam, ni, n_bad = 0.0, 2.0, 0
        for it in range(iters):
            cur = self.chi2()
            ini = cur
            Hcam, bcam, Hpt, bpt, _ = self.build()
            if it == 0:      # computeLambdaInit: 1e-5 * the largest diagonal entry of the Hessian (:165-180)
                md = 0.0
                for c in range(self.nc):
                    if self.cam_col[c] >= 0:
                        md = max(md, np.abs(np.diag(Hcam[c])).max())
                if (~self.pt_fixed).any():
                    md = max(md, np.abs(np.einsum("pii->pi", Hpt[~self.pt_fixed])).max())
                lam, ni, n_bad = 1e-5 * md, 2.0, 0
            rho, q = 0.0, 0
            while True:
                saved = (self.R.copy(), self.t.copy(), self.X.copy())
                ok, xp, xl = self.solve_blocks(lam)
                scale = 0.0
                if ok:
                    self.update(xp, xl)
                    free = ~self.pt_fixed
                    b_all = np.concatenate([bcam[~self.cam_fixed].ravel(), bpt[free].ravel()])
                    x_all = np.concatenate([xp, xl[free].ravel()])
                    scale = float(np.sum(x_all * (lam * x_all + b_all)))      # computeScale (:182-189)
                tmp = self.chi2() if ok else np.finfo(float).max
                rho = (cur - tmp) / (scale + 1e-3)
                self.rho_log.append(rho)
                if rho > 0 and np.isfinite(tmp):
                    alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    cur = tmp
                else:
                    lam *= ni
                    ni *= 2
                    self.R, self.t, self.X = saved
                q += 1
                if not (rho < 0 and q < 10):
                    break
            chi_h.append(cur); lam_h.append(lam); tr_h.append(q)
            if q == 10 or rho == 0:
                break
            n_bad = n_bad + 1 if (ini - cur) * 1e3 < ini else 0      # the gain check of SparseOptimizer::optimize's caller convention
            if n_bad >= 3:
                break
        self._hist = (np.array(chi_h), np.array(lam_h), np.array(tr_h, np.int32))
        return len(chi_h)

    def history(self):
        return self._hist

    def cams7(self):
        return np.concatenate([self.t, np.array([R_to_quat(R) for R in self.R])], 1)

    def state(self):
        return self.cams7(), np.zeros((0, 10)), self.X.copy()

    def close(self):
        pass


# ---------------------------------------------------------------------------------------------------------------------------------------
# The GPU tests' graph family: ~24 cameras on a street, ~600 landmarks whose tracks hit every code path of the device's Schur schedule.
FX = FY = 718.856
CX, CY = 607.19, 185.22
BF = 386.1448


def make_family(seed=1, stereo_share=0.5, long_track=True, n_cams=24, perturb=(0.004, 0.02, 0.03)):
    """cams7 (world-to-camera), points, fixed flags, mono and stereo edge tuples for Graph().  Camera 0 and landmark 0 are fixed.  Track lengths
    2, 3, 5, 6, 7, 8, 10, 11, 13 (every segment class of the fused schedule: k <= 2, 5, 7, 10, 13), one track of 18 cameras (long_track), one camera
    set seen by 40 landmarks (two segments of 32), one seen by exactly one landmark, one landmark with a single stereo edge only, one with mono
    edges only; elsewhere a fair coin with probability stereo_share decides each edge's kind, so kinds mix inside tracks.  Measurements: the
    edge's own projection of the true point + N(0, 0.5) pixels.  perturb = sigma of (rotation rad, translation m, point m) at the start."""
    rng = np.random.default_rng(seed)
    pos = np.stack([0.35 * np.arange(n_cams), 0.02 * np.sin(0.7 * np.arange(n_cams)), np.zeros(n_cams)], 1)      # x forward
    # camera axes in the world: z (optical) = +x world, x (right) = -y world, y (down) = -z world
    R_wc = np.array([[0.0, 0, 1], [-1, 0, 0], [0, -1, 0]])
    R_cw = R_wc.T
    t_cw = -(R_cw @ pos.T).T
    tracks = []
    def add(first, k, n):
        for _ in range(n):
            tracks.append(np.arange(first, first + k))
    lens = [2, 3, 5, 6, 7, 8, 10, 11, 13]
    for i in range(540):
        k = lens[i % len(lens)]
        add(int(rng.integers(0, n_cams - k + 1)), k, 1)
    add(3, 4, 40)                  # one camera set, 40 landmarks: two segments
    tracks.append(np.array([1, 3, 5, 7]))        # a camera set of its own (not consecutive): one landmark
    if long_track:
        tracks.append(np.arange(2, 20))          # k = 18
    single_stereo = len(tracks); tracks.append(np.array([5]))
    mono_only = len(tracks); tracks.append(np.arange(6, 11))
    npt = len(tracks)
    X = np.zeros((npt, 3))
    for p, cams in enumerate(tracks):
        mid = pos[cams].mean(0)
        X[p] = mid + np.array([rng.uniform(9, 30), rng.uniform(-4, 4), rng.uniform(-1.5, 1.5)])
    e_pt = np.concatenate([np.full(len(c), p) for p, c in enumerate(tracks)])
    e_cam = np.concatenate(tracks)
    st = rng.random(len(e_pt)) < stereo_share
    if 0.0 < stereo_share < 1.0:
        st[e_pt == single_stereo] = True
        st[e_pt == mono_only] = False
    perm = rng.permutation(len(e_pt))
    e_pt, e_cam, st = e_pt[perm], e_cam[perm], st[perm]
    Xc = (R_cw @ X[e_pt].T).T + t_cw[e_cam]
    intr = np.tile([FX, FY, CX, CY], (len(e_pt), 1))
    uvr = stereo_project(Xc, intr, np.full(len(e_pt), BF)) + rng.normal(0, 0.5, (len(e_pt), 3))
    uv = np.stack([Xc[:, 0] / Xc[:, 2] * FX + CX, Xc[:, 1] / Xc[:, 2] * FY + CY], 1) + rng.normal(0, 0.5, (len(e_pt), 2))
    q0 = R_to_quat(R_cw)
    cams7 = np.concatenate([t_cw, np.tile(q0, (n_cams, 1))], 1)
    for c in range(1, n_cams):
        dR, dt = se3_exp(np.concatenate([rng.normal(0, perturb[0], 3), rng.normal(0, perturb[1], 3)]))
        cams7[c, :3] = dt + dR @ t_cw[c]
        cams7[c, 3:] = R_to_quat(dR @ R_cw)
    pts = X + rng.normal(0, perturb[2], X.shape)
    pts[0] = X[0]
    cam_fixed = np.zeros(n_cams, np.int32); cam_fixed[0] = 1
    pt_fixed = np.zeros(npt, np.int32); pt_fixed[0] = 1
    m, s = ~st, st
    nm, ns = int(m.sum()), int(s.sum())
    mono = (e_pt[m].astype(np.int32), e_cam[m].astype(np.int32), uv[m], np.tile(np.eye(2).ravel(), (nm, 1)), intr[m], np.zeros(nm))
    stereo = (e_pt[s].astype(np.int32), e_cam[s].astype(np.int32), uvr[s], np.tile(np.eye(3).ravel(), (ns, 1)),
              np.concatenate([intr[s], np.full((ns, 1), BF)], 1), np.zeros(ns))
    return dict(cams=cams7, cam_fixed=cam_fixed, points=pts, pt_fixed=pt_fixed, mono=mono, stereo=stereo, tracks=tracks,
                single_stereo=single_stereo, mono_only=mono_only)


def graph_of(f, huber=None, rk_mono=None, rk_stereo=None):
    """Graph() of a make_family() dict; huber = (delta mono, delta stereo) puts Huber kernels on both classes."""
    m, s = list(f["mono"]), list(f["stereo"])
    if huber is not None:
        m[5] = np.full(len(m[0]), huber[0]); s[5] = np.full(len(s[0]), huber[1])
    return Graph(f["cams"], f["cam_fixed"], f["points"], f["pt_fixed"], tuple(m) if len(m[0]) else None, tuple(s) if len(s[0]) else None, rk_mono, rk_stereo)
