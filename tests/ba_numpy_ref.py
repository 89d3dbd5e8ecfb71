"""A plain float64 reference of the bundle adjustment's damped solve (test infrastructure, not a test file).

Input: what cs_ba_build_system / ba_oracle_build_system hand out -- dense H_pp in g2o's order, one 3x3 H_ll per free landmark (n_lm, 9),
one 6x3 H_pl per projection edge (n_proj, 18, row-major; zero unless both ends are free), b = [b_p, b_l] -- and the problem dict of
synth_ba.make_problem().  Damping is g2o's setLambda (block_solver.hpp:563-589, oracle/ba_oracle.cpp:set_lambda): lambda on every
diagonal entry of H_pp and of every H_ll.  The system is H x = b; the landmarks are eliminated with a block-diagonal D = H_ll + lambda I,
S = H_pp + lambda I - W D^-1 W^T, r = b_p - W D^-1 b_l, x_l = D^-1 (b_l - W^T x_p) (block_solver.hpp:373-482).

No edge couples a landmark to a cuboid, so a cuboid eliminated after the landmarks (what the device does when cs_ba_reduced_size says
so) is a second Schur complement of S onto the remaining pose columns.  Everything is vectorised (scipy.sparse products over the edges):
20 000 landmarks take well under a second per damping value.
"""
import numpy as np
import scipy.linalg
import scipy.sparse as sp


def pose_columns(pr, cuboids_first=False):
    """g2o column of every camera / cuboid (-1: fixed), the order ba_oracle.cpp:build_index gives the poses."""
    cf, of = np.asarray(pr["cam_fixed"]).astype(bool), np.asarray(pr["cub_fixed"]).astype(bool)
    cam_g, cub_g = np.full(len(cf), -1), np.full(len(of), -1)
    col = 0
    for kind in ((1, 0) if cuboids_first else (0, 1)):
        fixed, out, dim = (cf, cam_g, 6) if kind == 0 else (of, cub_g, 9)
        free = np.nonzero(~fixed)[0]
        out[free] = col + dim * np.arange(len(free))
        col += dim * len(free)
    return cam_g, cub_g


def solver_permutation(pr, cam_col, cub_col, n_red, cuboids_first=False):
    """perm with perm[s] = the g2o pose column of solver column s, for the n_red columns of the reduced system (cam_col / cub_col as
    reduced_system() returns them; a cuboid column >= n_red is an eliminated cuboid), and the g2o columns of the eliminated cuboids."""
    cam_g, cub_g = pose_columns(pr, cuboids_first)
    perm = np.full(n_red, -1)
    elim = []
    for gcols, scols, dim in ((cam_g, np.asarray(cam_col), 6), (cub_g, np.asarray(cub_col), 9)):
        assert np.array_equal(gcols < 0, scols < 0), "fixed vertices differ between the handle and the problem"
        for g, s in zip(gcols, scols):
            if s < 0:
                continue
            if s >= n_red:
                elim.extend(range(g, g + dim))
            else:
                perm[s:s + dim] = np.arange(g, g + dim)
    assert (perm >= 0).all() and len(np.unique(perm)) == n_red, "solver columns do not cover the reduced system"
    return perm, np.array(elim, int)


def _cho(A):
    """Upper Cholesky factor, or None if A is not positive definite."""
    try:
        return scipy.linalg.cho_factor(A, lower=False, check_finite=False)
    except np.linalg.LinAlgError:
        return None


class Reference:
    def __init__(self, system, pr, cuboids_first=False):
        Hpp, Hll, Hpl, b = system
        self.Hpp = np.asarray(Hpp, float)
        self.n = n = self.Hpp.shape[0]
        self.Hll = np.asarray(Hll, float).reshape(-1, 3, 3)
        self.n_lm = len(self.Hll)
        self.b = np.asarray(b, float)
        assert len(self.b) == n + 3 * self.n_lm
        cam_g, _ = pose_columns(pr, cuboids_first)
        pf = np.asarray(pr["pt_fixed"]).astype(bool)
        lm = np.full(len(pf), -1)
        lm[~pf] = np.arange(int((~pf).sum()))
        assert int((~pf).sum()) == self.n_lm
        e_pt, e_cam = np.asarray(pr["e_pt"]), np.asarray(pr["e_cam"])
        li, cc = lm[e_pt], cam_g[e_cam]
        ok = (li >= 0) & (cc >= 0)
        B = np.asarray(Hpl, float).reshape(-1, 6, 3)[ok]
        li, cc = li[ok], cc[ok]
        # W (n x 3 n_lm): the 6x3 blocks at (camera column, 3 * landmark); coo sums repeated (camera, landmark) pairs
        rows = (cc[:, None, None] + np.arange(6)[None, :, None]).repeat(3, 2)
        cols = (3 * li[:, None, None] + np.arange(3)[None, None, :]).repeat(6, 1)
        self.W = sp.csr_matrix((B.ravel(), (rows.ravel(), cols.ravel())), shape=(n, 3 * self.n_lm))
        self.WT = self.W.T.tocsr()
        bi = (3 * np.arange(self.n_lm)[:, None, None] + np.arange(3)[None, :, None]).repeat(3, 2)
        self._bd_rows, self._bd_cols = bi.ravel(), bi.transpose(0, 2, 1).ravel()

    def _dinv(self, lam):
        D = self.Hll + lam * np.eye(3)
        return np.linalg.inv(D)

    def _blockdiag(self, blocks):
        return sp.csr_matrix((blocks.ravel(), (self._bd_rows, self._bd_cols)), shape=(3 * self.n_lm, 3 * self.n_lm))

    def landmarks_pd(self, lam):
        return bool((np.linalg.eigvalsh(self.Hll + lam * np.eye(3))[:, 0] > 0).all()) if self.n_lm else True

    def schur(self, lam):
        """(S, r) with every landmark eliminated: all pose columns, g2o order."""
        Dinv = self._dinv(lam)
        bl = self.b[self.n:]
        S = self.Hpp + lam * np.eye(self.n)
        if self.n_lm == 0:
            return S, self.b[:self.n].copy()
        WD = self.W @ self._blockdiag(Dinv)
        S -= (WD @ self.WT).toarray()
        r = self.b[:self.n] - WD @ bl
        return 0.5 * (S + S.T), r

    def reduced(self, lam, keep):
        """The damped reduced system on the g2o pose columns `keep` (in that order): landmarks and every other pose column eliminated."""
        S, r = self.schur(lam)
        keep = np.asarray(keep)
        rest = np.setdiff1d(np.arange(self.n), keep)
        if len(rest) == 0:
            return S[np.ix_(keep, keep)], r[keep]
        F = _cho(S[np.ix_(rest, rest)])
        assert F is not None, "eliminated pose block not positive definite"
        X = scipy.linalg.cho_solve(F, np.column_stack([S[np.ix_(rest, keep)], r[rest]]), check_finite=False)
        Sk = S[np.ix_(keep, keep)] - S[np.ix_(keep, rest)] @ X[:, :-1]
        rk = r[keep] - S[np.ix_(keep, rest)] @ X[:, -1]
        return 0.5 * (Sk + Sk.T), rk

    def positive_definite(self, lam):
        """Is the whole damped system (poses and landmarks) positive definite?  Every D_i and the Schur complement (Haynsworth)."""
        if not self.landmarks_pd(lam):
            return False
        return _cho(self.schur(lam)[0]) is not None

    def solve(self, lam):
        """(positive definite?, full increment x in g2o order [poses, landmarks]) by Cholesky."""
        if not self.landmarks_pd(lam):
            return False, None
        S, r = self.schur(lam)
        F = _cho(S)
        if F is None:
            return False, None
        xp = scipy.linalg.cho_solve(F, r, check_finite=False)
        return True, self.backsub(lam, xp)

    def backsub(self, lam, xp):
        x = np.zeros(len(self.b))
        x[:self.n] = xp
        if self.n_lm:
            rl = self.b[self.n:] - self.WT @ xp
            x[self.n:] = np.einsum("kij,kj->ki", self._dinv(lam), rl.reshape(-1, 3)).ravel()
        return x

    def lambda_star(self, rel=1e-3):
        """The most negative damping at which the whole damped system is still positive definite (-lambda_min of H), by bisection:
        a geometric bracket first, then halving to `rel` of its size.  (lambda_star, landmark-only bound: -min eig of the H_ll)."""
        lam_lm = -float(np.linalg.eigvalsh(self.Hll)[:, 0].min()) if self.n_lm else -np.inf
        hi = 0.0
        if not self.positive_definite(hi):        # (an undamped system that is already indefinite: bracket upwards)
            lo, hi = 0.0, 1e-8 * float(np.abs(np.diag(self.Hpp)).max() + 1.0)
            while not self.positive_definite(hi):
                lo, hi = hi, 4 * hi
        else:
            step = 1e-12 * float(np.abs(np.diag(self.Hpp)).max() + 1.0)
            lo = -step
            while self.positive_definite(lo):
                hi, lo = lo, 4 * lo
        while hi - lo > rel * max(abs(lo), abs(hi)):
            mid = 0.5 * (lo + hi)
            if self.positive_definite(mid):
                hi = mid
            else:
                lo = mid
        return hi, lam_lm
