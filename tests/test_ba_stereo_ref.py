"""The numpy reference behind the stereo bundle-adjustment GPU tests (tests/ba_stereo_ref.py) pinned on the CPU: restricted to mono edges it
reproduces the committed independent fixture, its stereo Jacobians are the derivative of its own error, the error carries the reference's
single-precision disparity, and the LM runs the GPU tests compare against take no decision that rounding could flip."""
import numpy as np
import pytest

import ba_stereo_ref as ref
from test_ba_oracle import check_against_independent_fixture


def test_mono_restriction_reproduces_the_independent_fixture():
    """tests/golden/ba_proj_schur_30.npz to the tolerances the CPU oracle is held to (test_ba_oracle.py: 1e-11 on the system, 1e-8 on the state)."""
    def make(g):
        return ref.Graph(g["cams"], g["cam_fixed"], g["points"], g["pt_fixed"], mono=(g["e_pt"], g["e_cam"], g["e_uv"], g["e_info"], g["e_intr"], g["e_huber"]))
    check_against_independent_fixture(make, 1e-11, 1e-8)


def test_stereo_jacobians_are_the_derivative_of_the_error():
    """Central differences (step 1e-6) of the reference's own error with a double invz -- the smooth function linearizeOplus differentiates; the
    float-rounded invz moves in steps of 6e-8 relative and has no derivative -- against both analytic Jacobians, 1e-6 of each Jacobian's largest entry."""
    f = ref.make_family(seed=1, stereo_share=1.0)
    G = ref.graph_of(f)
    Ji, Jj = G.jacobians()
    h = 1e-6
    worst = 0.0
    X0, R0, t0 = G.X.copy(), G.R.copy(), G.t.copy()
    for j in range(3):
        G.X = X0.copy(); G.X[:, j] += h; ep, _ = G.errors(double_invz=True)
        G.X = X0.copy(); G.X[:, j] -= h; em, _ = G.errors(double_invz=True)
        num = (ep - em) / (2 * h)
        worst = max(worst, (np.abs(num - Ji[:, :, j]).max(1) / np.abs(Ji).max((1, 2))).max())
    G.X = X0
    for j in range(6):
        d = np.zeros(6); d[j] = h
        out = []
        for sgn in (1.0, -1.0):
            dR, dt = ref.se3_exp(sgn * d)
            G.R = np.einsum("ij,cjk->cik", dR, R0); G.t = dt + np.einsum("ij,cj->ci", dR, t0)
            out.append(G.errors(double_invz=True)[0])
        num = (out[0] - out[1]) / (2 * h)
        worst = max(worst, (np.abs(num - Jj[:, :, j]).max(1) / np.abs(Jj).max((1, 2))).max())
    print("worst relative difference analytic vs central:", worst)
    assert worst <= 1e-6


def test_disparity_is_the_single_precision_product():
    """u_left - u_right of the error function equals float(bf) * float(1 / z), bit for bit, over depths 2 .. 60 m (disparities 190 .. 6 px)."""
    rng = np.random.default_rng(5)
    n = 4000
    Xc = np.stack([rng.uniform(-3, 3, n), rng.uniform(-1, 1, n), rng.uniform(2, 60, n)], 1)
    intr = np.tile([ref.FX, ref.FY, ref.CX, ref.CY], (n, 1))
    G = ref.Graph(np.array([[0, 0, 0, 0, 0, 0, 1.0]]), [1], Xc, np.zeros(n, int),
                  stereo=(np.arange(n), np.zeros(n, int), np.zeros((n, 3)), np.tile(np.eye(3).ravel(), (n, 1)), np.concatenate([intr, np.full((n, 1), ref.BF)], 1), np.zeros(n)))
    e, _ = G.errors()
    proj = -e                                  # measurement zero: error = -projection
    want = (np.float32(ref.BF) * (1.0 / Xc[:, 2]).astype(np.float32)).astype(np.float64)
    assert np.array_equal(proj[:, 0] - proj[:, 2], want)
    assert not np.array_equal(want, ref.BF / Xc[:, 2])       # (and that is not the double quotient)


# the graphs and iteration counts of tests/test_ba_stereo_gpu.py
@pytest.mark.parametrize("kw", [dict(seed=1), dict(seed=1, stereo_share=1.0), dict(seed=2, long_track=False, n_cams=60)], ids=["mixed", "all_stereo", "banded_60_cameras"])
def test_no_lm_decision_of_the_reference_runs_is_within_rounding(kw):
    G = ref.graph_of(ref.make_family(**kw))
    assert G.optimize(3) == 3
    print("rho of every trial:", G.rho_log)
    assert all(abs(r) > 1e-6 for r in G.rho_log)
