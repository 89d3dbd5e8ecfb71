"""numpy statement of the Sim(3) pose-graph optimisation (cs_pgo_*): g2o's Sim3 (types/sim3.h), VertexSim3Expmap / EdgeSim3
(types/types_seven_dof_expmap.h) with BaseBinaryEdge's numeric Jacobians (core/base_binary_edge.hpp:130-205) and
OptimizationAlgorithmLevenberg (core/optimization_algorithm_levenberg.cpp:61-189), over a dense H + lambda I.

Generic in dtype: the same code runs in float64 and in np.longdouble (numpy.linalg has no long double, hence the hand-written 3 x 3 LU and
dense Cholesky).  Every function works on a batch (leading axis) -- the branches are masks, so a batch can be asked how many of its members
took which one.  A state is qx qy qz qw tx ty tz s (Sim3::operator[] order)."""
import numpy as np

EPS = 0.00001      # sim3.h:90, :158
DELTA = 1e-9       # base_binary_edge.hpp:147


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def rotate(q, v):
    """Eigen's QuaternionBase::_transformVector."""
    uv = _cross(q[..., :3], v)
    uv = uv + uv
    return v + q[..., 3:4] * uv + _cross(q[..., :3], uv)


def sim3_map(S, x):
    return S[..., 7:8] * rotate(S[..., :4], x) + S[..., 4:7]


def sim3_mul(a, b):
    ax, ay, az, aw = (a[..., i] for i in range(4))
    bx, by, bz, bw = (b[..., i] for i in range(4))
    q = np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                  aw * bw - ax * bx - ay * by - az * bz], -1)
    t = a[..., 7:8] * rotate(a[..., :4], b[..., 4:7]) + a[..., 4:7]
    return np.concatenate([q, t, a[..., 7:8] * b[..., 7:8]], -1)


def sim3_inv(a):
    qc = np.concatenate([-a[..., :3], a[..., 3:4]], -1)
    t = rotate(qc, (-1 / a[..., 7:8]) * a[..., 4:7])
    return np.concatenate([qc, t, 1 / a[..., 7:8]], -1)


def _skew(v):
    z = np.zeros_like(v[..., 0])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1), np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def _eye(like):
    return np.broadcast_to(np.eye(3, dtype=like.dtype), like.shape)


def quat_from_rotmat(R, branch_out=None):
    """Eigen's Quaterniond(Matrix3d): the trace branch and the three largest-diagonal branches, no normalisation.  x y z w."""
    r = lambda i, j: R[..., i, j]
    tr = r(0, 0) + r(1, 1) + r(2, 2)
    with np.errstate(all="ignore"):
        t0 = np.sqrt(tr + 1)
        h0 = 0.5 / t0
        q0 = np.stack([(r(2, 1) - r(1, 2)) * h0, (r(0, 2) - r(2, 0)) * h0, (r(1, 0) - r(0, 1)) * h0, 0.5 * t0], -1)
        qs = [q0]
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            t = np.sqrt(r(i, i) - r(j, j) - r(k, k) + 1)
            h = 0.5 / t
            v = [None] * 4
            v[i] = 0.5 * t
            v[3] = (r(k, j) - r(j, k)) * h
            v[j] = (r(j, i) + r(i, j)) * h
            v[k] = (r(k, i) + r(i, k)) * h
            qs.append(np.stack(v, -1))
    i_big = np.where(r(1, 1) > r(0, 0), 1, 0)
    i_big = np.where(r(2, 2) > np.where(i_big == 1, r(1, 1), r(0, 0)), 2, i_big)
    branch = np.where(tr > 0, 0, i_big + 1)
    if branch_out is not None:
        branch_out.append(branch)
    out = qs[0]
    for b in (1, 2, 3):
        out = np.where((branch == b)[..., None], qs[b], out)
    return out


def _abc(sigma, s, theta, small_rot):
    """A, B, C of W = A Omega + B Omega^2 + C I, all four branches (sim3.h:92-133, :162-206); also the mask of the branch with
    |sigma| >= eps and a small rotation, whose B is the reference's ((0.5 sigma^2 - sigma + 1) s) / sigma^3."""
    one = np.ones_like(sigma)
    small_sig = np.abs(sigma) < EPS
    with np.errstate(all="ignore"):
        theta2 = theta * theta
        sigma2 = sigma * sigma
        A00, B00 = one / 2, one / 6
        A01 = (1 - np.cos(theta)) / theta2
        B01 = (theta - np.sin(theta)) / (theta2 * theta)
        C1 = (s - 1) / sigma
        A10 = ((sigma - 1) * s + 1) / sigma2
        B10 = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma)
        a, b = s * np.sin(theta), s * np.cos(theta)
        c = theta2 + sigma2
        A11 = (a * sigma + (1 - b) * theta) / (theta * c)
        B11 = (C1 - ((b - 1) * sigma + a * theta) / c) * 1 / theta2
    A = np.where(small_sig, np.where(small_rot, A00, A01), np.where(small_rot, A10, A11))
    B = np.where(small_sig, np.where(small_rot, B00, B01), np.where(small_rot, B10, B11))
    C = np.where(small_sig, one, C1)
    return A, B, C, (~small_sig) & small_rot


def sim3_exp(u):
    """sim3.h:70-138."""
    omega, ups, sigma = u[..., :3], u[..., 3:6], u[..., 6]
    theta = np.sqrt(omega[..., 0] * omega[..., 0] + omega[..., 1] * omega[..., 1] + omega[..., 2] * omega[..., 2])
    Om = _skew(omega)
    Om2 = Om @ Om
    s = np.exp(sigma)
    small_rot = theta < EPS
    A, B, C, _ = _abc(sigma, s, theta, small_rot)
    I = _eye(Om)
    with np.errstate(all="ignore"):
        ra, rb = np.sin(theta) / theta, (1 - np.cos(theta)) / (theta * theta)
    ra, rb = np.where(small_rot, 1, ra).astype(u.dtype), np.where(small_rot, 1, rb).astype(u.dtype)      # I + Omega + Omega^2 (not 1/2 Omega^2)
    R = (I + ra[..., None, None] * Om) + rb[..., None, None] * Om2
    q = quat_from_rotmat(R)
    W = (A[..., None, None] * Om + B[..., None, None] * Om2) + C[..., None, None] * I
    t = (W @ ups[..., None])[..., 0]
    return np.concatenate([q, t, s[..., None]], -1)


def rotmat(q):
    """Eigen's toRotationMatrix: the unit-quaternion formula, whatever |q| is."""
    x, y, z, w = (q[..., i] for i in range(4))
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return np.stack([np.stack([1 - (tyy + tzz), txy - twz, txz + twy], -1), np.stack([txy + twz, 1 - (txx + tzz), tyz - twx], -1),
                     np.stack([txz - twy, tyz + twx, 1 - (txx + tyy)], -1)], -2)


def lu3_solve(W, b):
    """W x = b by 3 x 3 LU with partial pivoting (Eigen's Matrix3d::lu())."""
    M = np.concatenate([W, b[..., None]], -1).copy()       # (..., 3, 4)

    def swap(M, i, j, m):
        ri, rj = M[..., i, :].copy(), M[..., j, :].copy()
        M[..., i, :] = np.where(m[..., None], rj, ri)
        M[..., j, :] = np.where(m[..., None], ri, rj)

    a0, a1, a2 = (np.abs(M[..., i, 0]) for i in range(3))
    p1 = a1 > a0
    p2 = a2 > np.where(p1, a1, a0)
    swap(M, 0, 1, p1 & ~p2)
    swap(M, 0, 2, p2)
    with np.errstate(all="ignore"):
        l10, l20 = M[..., 1, 0] / M[..., 0, 0], M[..., 2, 0] / M[..., 0, 0]
        for c in (1, 2):
            M[..., 1, c] = M[..., 1, c] - l10 * M[..., 0, c]
            M[..., 2, c] = M[..., 2, c] - l20 * M[..., 0, c]
        swap(M, 1, 2, np.abs(M[..., 2, 1]) > np.abs(M[..., 1, 1]))
        m1, m2 = M[..., 1, 0] / M[..., 0, 0], M[..., 2, 0] / M[..., 0, 0]
        l21 = M[..., 2, 1] / M[..., 1, 1]
        u22 = M[..., 2, 2] - l21 * M[..., 1, 2]
        y0 = M[..., 0, 3]
        y1 = M[..., 1, 3] - m1 * y0
        y2 = (M[..., 2, 3] - m2 * y0) - l21 * y1
        x2 = y2 / u22
        x1 = (y1 - M[..., 1, 2] * x2) / M[..., 1, 1]
        x0 = ((y0 - M[..., 0, 1] * x1) - M[..., 0, 2] * x2) / M[..., 0, 0]
    return np.stack([x0, x1, x2], -1)


def sim3_log(S, stats=None):
    """sim3.h:144-223.  stats (a dict): 'quirk' counts the members in the |sigma| >= eps, small-rotation branch, 'log' all members."""
    sigma = np.log(S[..., 7])
    R = rotmat(S[..., :4])
    d = 0.5 * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1)
    dR = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    small_rot = d > 1 - EPS
    with np.errstate(all="ignore"):
        theta = np.arccos(d)
        f = theta / (2 * np.sqrt(1 - d * d))
    theta = np.where(small_rot, 0, theta).astype(S.dtype)
    omega = np.where(small_rot[..., None], 0.5 * dR, f[..., None] * dR)
    A, B, C, quirk = _abc(sigma, S[..., 7], theta, small_rot)
    if stats is not None:
        stats["quirk"] = stats.get("quirk", 0) + int(np.sum(quirk))
        stats["log"] = stats.get("log", 0) + int(np.size(quirk))
    Om = _skew(omega)
    W = (A[..., None, None] * Om + B[..., None, None] * (Om @ Om)) + C[..., None, None] * _eye(Om)
    ups = lu3_solve(W, S[..., 4:7])
    return np.concatenate([omega, ups, sigma[..., None]], -1)


def sim3_oplus(S, u, fix_scale):
    """VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69)."""
    u = u.copy()
    u[..., 6] = np.where(fix_scale, 0, u[..., 6])
    return sim3_mul(sim3_exp(u), S)


def edge_error(C, Si, Sj, stats=None):
    """EdgeSim3::computeError (types_seven_dof_expmap.h:106-114)."""
    return sim3_log(sim3_mul(sim3_mul(C, Si), sim3_inv(Sj)), stats)


def cholesky_solve(A, b):
    """Dense Cholesky of the lower triangle of A; None when a pivot is not positive."""
    n = len(b)
    L = np.zeros_like(A)
    for j in range(n):
        d = A[j, j] - L[j, :j] @ L[j, :j]
        if not d > 0:
            return None
        L[j, j] = np.sqrt(d)
        if j + 1 < n:
            L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    y = np.zeros_like(b)
    for j in range(n):
        y[j] = (b[j] - L[j, :j] @ y[:j]) / L[j, j]
    x = np.zeros_like(b)
    for j in range(n - 1, -1, -1):
        x[j] = (y[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    return x


class Graph:
    """The graph of cs_pgo_set_vertices / cs_pgo_set_edges, in `dtype`."""

    def __init__(self, sim8, fixed, fix_scale, vi, vj, meas8, info49=None, dtype=np.float64):
        self.dtype = np.dtype(dtype)
        self.est = np.array(sim8, dtype=self.dtype).reshape(-1, 8)
        self.est_init = self.est.copy()
        self.nv = len(self.est)
        self.fixed = np.zeros(self.nv, bool) if fixed is None else np.asarray(fixed).astype(bool)
        self.fix_scale = np.zeros(self.nv, bool) if fix_scale is None else np.asarray(fix_scale).astype(bool)
        self.vi, self.vj = np.asarray(vi, int), np.asarray(vj, int)
        self.ne = len(self.vi)
        self.meas = np.array(meas8, dtype=self.dtype).reshape(-1, 8)
        self.info = np.broadcast_to(np.eye(7, dtype=self.dtype), (self.ne, 7, 7)).copy() if info49 is None else np.array(info49, dtype=self.dtype).reshape(-1, 7, 7)
        deg = np.bincount(np.concatenate([self.vi, self.vj]), minlength=self.nv)
        self.vcol = np.full(self.nv, -1)
        free = (~self.fixed) & (deg > 0)
        self.vcol[free] = 7 * np.arange(int(free.sum()))
        self.n = 7 * int(free.sum())
        self.stats = {}
        self.user_lambda_init, self.max_trials = 0.0, 10
        self.chi2_hist, self.lambda_hist, self.trials_hist, self.rho_log, self.quirk_per_linearisation = [], [], [], [], []

    def set_estimates(self, sim8):
        self.est = np.array(sim8, dtype=self.dtype).reshape(-1, 8)
        self.est_init = self.est.copy()

    def errors(self, est=None):
        est = self.est if est is None else est
        return edge_error(self.meas, est[self.vi], est[self.vj], self.stats)

    def chi2(self):
        e = self.errors()
        each = np.einsum("ka,kab,kb->k", e, self.info, e)
        return each.sum(), each

    def linearize_edges(self):
        """err (E, 7), Ji, Jj (E, 7, 7; row = error component): central differences through oplusImpl, zero for a fixed vertex."""
        T = self.dtype.type
        delta = T(DELTA)
        scalar = 1 / (2 * delta)
        Si, Sj = self.est[self.vi], self.est[self.vj]
        q0 = self.stats.get("quirk", 0)
        e = edge_error(self.meas, Si, Sj, self.stats)
        J = [np.zeros((self.ne, 7, 7), self.dtype), np.zeros((self.ne, 7, 7), self.dtype)]
        for side, idx in ((0, self.vi), (1, self.vj)):
            free = (self.vcol[idx] >= 0)
            fs = self.fix_scale[idx]
            for d in range(7):
                u = np.zeros((self.ne, 7), self.dtype)
                u[:, d] = delta
                Sp = sim3_oplus(Si if side == 0 else Sj, u, fs)
                Sm = sim3_oplus(Si if side == 0 else Sj, -u, fs)
                ep = edge_error(self.meas, Sp, Sj, self.stats) if side == 0 else edge_error(self.meas, Si, Sp, self.stats)
                em = edge_error(self.meas, Sm, Sj, self.stats) if side == 0 else edge_error(self.meas, Si, Sm, self.stats)
                J[side][:, :, d] = np.where(free[:, None], scalar * (ep - em), 0)
        self.quirk_per_linearisation.append(self.stats.get("quirk", 0) - q0)
        return e, J[0], J[1]

    def build_system(self):
        e, Ji, Jj = self.linearize_edges()
        H = np.zeros((self.n, self.n), self.dtype)
        b = np.zeros(self.n, self.dtype)
        chi2 = self.dtype.type(0)
        for k in range(self.ne):
            Om = self.info[k]
            chi2 = chi2 + e[k] @ (Om @ e[k])
            ci, cj = self.vcol[self.vi[k]], self.vcol[self.vj[k]]
            Oe = Om @ e[k]
            if ci >= 0:
                H[ci:ci + 7, ci:ci + 7] += Ji[k].T @ (Om @ Ji[k])
                b[ci:ci + 7] -= Ji[k].T @ Oe
            if cj >= 0:
                H[cj:cj + 7, cj:cj + 7] += Jj[k].T @ (Om @ Jj[k])
                b[cj:cj + 7] -= Jj[k].T @ Oe
            if ci >= 0 and cj >= 0:
                blk = Ji[k].T @ (Om @ Jj[k])
                H[ci:ci + 7, cj:cj + 7] = blk
                H[cj:cj + 7, ci:ci + 7] = blk.T
        return H, b, chi2

    def update(self, x):
        free = self.vcol >= 0
        u = np.zeros((self.nv, 7), self.dtype)
        u[free] = x.reshape(-1, 7)
        new = sim3_oplus(self.est, u, self.fix_scale)
        self.est = np.where(free[:, None], new, self.est)

    def optimize(self, iterations):
        """OptimizationAlgorithmLevenberg::solve per iteration, as cs_pgo_optimize; returns iterations_done."""
        T = self.dtype.type
        done, n_bad = 0, 0
        lam, ni = T(0), T(2)
        self.chi2_hist, self.lambda_hist, self.trials_hist, self.rho_log = [], [], [], []
        for it in range(iterations):
            if self.n == 0:
                break
            H, b, current = self.build_system()
            ini = current
            if it == 0:
                lam = T(self.user_lambda_init) if self.user_lambda_init > 0 else T(1e-5) * np.abs(np.diag(H)).max()
                ni, n_bad = T(2), 0
            rho, qmax, rhos = T(0), 0, []
            while True:
                backup = self.est.copy()
                x = cholesky_solve(H + lam * np.eye(self.n, dtype=self.dtype), b)
                if x is None:
                    temp = T(np.finfo(np.float64).max)
                    scale = T(0)     # (x is whatever the failed factorisation left: the trial is rejected whatever the scale term says)
                else:
                    self.update(x)
                    temp = self.chi2()[0]
                    scale = (x * (lam * x + b)).sum()
                rho = (current - temp) / (scale + T(1e-3))
                rhos.append(float(rho))
                if rho > 0 and np.isfinite(temp):
                    alpha = min(1 - (2 * rho - 1) ** 3, T(2) / 3)
                    lam = lam * max(T(1) / 3, alpha)
                    ni = T(2)
                    current = temp
                else:
                    lam = lam * ni
                    ni = ni * 2
                    self.est = backup
                qmax += 1
                if not (rho < 0 and qmax < self.max_trials):
                    break
            self.chi2_hist.append(current); self.lambda_hist.append(lam); self.trials_hist.append(qmax); self.rho_log.append(rhos)
            done += 1
            if qmax == self.max_trials or rho == 0:
                break
            n_bad = n_bad + 1 if (ini - current) * 1e3 < ini else 0
            if n_bad >= 3:
                break
        return done

    def get_se3(self):
        """[sR t] -> [R t / s] in SE3Quat::toVector order, the rotation normalised with w >= 0."""
        q = self.est[:, :4] * np.where(self.est[:, 3:4] < 0, -1, 1)
        q = q / np.sqrt((q * q).sum(-1, keepdims=True))
        return np.concatenate([self.est[:, 4:7] * (1 / self.est[:, 7:8]), q], -1)

    def correct_points(self, ref, xyz):
        xyz = np.asarray(xyz, self.dtype).reshape(-1, 3)
        return sim3_map(sim3_inv(self.est[ref]), sim3_map(self.est_init[ref], xyz))


def state_deviation(a, b):
    """Worst relative state difference, each vertex against its largest component."""
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    return float((np.abs(a - b).max(-1) / np.abs(b).max(-1)).max())
