"""tests/pgo_ref.py on its own (no GPU): what the comparisons of tests/test_pgo_gpu.py rest on, asserted for every graph they use.

  (a) the float64 and the long-double run take the same trials, and their states agree to 1e-6 -- ten times inside the 1e-5 contract;
  (b) no trial's |rho| is below 1e-6 (the rule of test_pose_only_gpu.py: a decision that close is taken by rounding);
  (c) the graphs that are not the rejected-trial case never evaluate log in sim3.h:192's branch, and the rejected-trial case does;
  (d) chi2 and lambda histories of the two precisions agree to 5e-6, half the contract: they are more sensitive than the states (lambda's
      update 1 - (2 rho - 1)^3; the chi2 after a step from a far start), and the device differs from the float64 reference by errors of
      the kind and size float64 differs from long double by, so the reference's own share must leave the other half.  With seed 1 the
      far graph's lambda differed by 1.1e-5 between the two precisions; pgo_cases.SEED = 2 is a seed where it does not.
Measured (float64 against long double): state deviations 4e-8 .. 2.5e-7, chi2 1.2e-7 .. 1.8e-6 (the far graph), lambda <= 1.2e-7; the
rejected-trial graph: trials [1, 6], states 1.1e-7, chi2 3.2e-6."""
import numpy as np
import pytest

import pgo_cases as pc
import pgo_ref


def _rel(a, b):
    return max(abs(float(x - y)) / abs(float(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("name,lam,iterations", pc.all_runs(), ids=lambda v: str(v))
def test_conditions_of_the_gpu_comparisons(name, lam, iterations):
    a, b = pc.ref_run(name, lam, iterations), pc.ref_run(name, lam, iterations, True)
    assert a.done == b.done == iterations
    assert a.trials_hist == b.trials_hist                                                          # (a)
    dev = pgo_ref.state_deviation(a.est, b.est)
    rho = min(abs(r) for rr in a.rho_log for r in rr)
    print("%s lambda %g: trials %s, state deviation %.3g, chi2 %.3g, lambda %.3g, min |rho| %.3g, sim3.h:192 evaluations %s"
          % (name, lam, a.trials_hist, dev, _rel(a.chi2_hist, b.chi2_hist), _rel(a.lambda_hist, b.lambda_hist), rho, a.quirk_per_linearisation))
    assert dev < 1e-6                                                                              # (a)
    assert rho > 1e-6                                                                              # (b)
    if name == "rejected":
        assert a.quirk_per_linearisation[0] == 0 and a.quirk_per_linearisation[1] > 0              # (c)
        assert a.trials_hist[1] > 1 and min(r for r in a.rho_log[1]) < 0
    else:
        assert a.stats.get("quirk", 0) == 0 and b.stats.get("quirk", 0) == 0                       # (c)
        assert _rel(a.chi2_hist, b.chi2_hist) < 5e-6 and _rel(a.lambda_hist, b.lambda_hist) < 5e-6  # (d)


def test_big_rotation_update_reaches_every_quaternion_branch():
    """pgo_cases.bigrot_graph: the first step's exp(update) takes Quaterniond(R)'s trace branch and its three diagonal branches.  After one
    iteration the two precisions differ by 4.8e-6 (a 2.6 rad step carries the numeric Jacobian's noise), after two by 1.5e-12 -- so the
    GPU comparison runs two.  The second trial's rho is 1.8e-7, under rule (b)'s 1e-6, but not by rounding: chi2 falls from 1.8e-10 to
    7.6e-22 and rho is small only because its denominator carries the + 1e-3; asserted below as a drop of six orders of magnitude."""
    name, lam, iterations = pc.BIGROT
    a, b = pc.ref_run(name, lam, iterations), pc.ref_run(name, lam, iterations, True)
    assert a.trials_hist == b.trials_hist == [1, 1] and pgo_ref.state_deviation(a.est, b.est) < 1e-6
    assert a.rho_log[0][0] > 0.9 and float(a.chi2_hist[1]) < 1e-6 * float(a.chi2_hist[0])
    G = pc.make_ref(pc.graph(name), lam=lam)
    H, rhs, _ = G.build_system()
    x = pgo_ref.cholesky_solve(H + lam * np.eye(G.n), rhs).reshape(-1, 7)
    branches = []
    pgo_ref.quat_from_rotmat(pgo_ref.rotmat(pgo_ref.sim3_exp(x)[:, :4]), branches)
    assert set(branches[0].tolist()) == {0, 1, 2, 3}


def test_layout_graph_is_what_it_claims():
    g = pc.layout_graph()
    pairs = list(zip(g["vi"].tolist(), g["vj"].tolist()))
    deg = np.bincount(np.concatenate([g["vi"], g["vj"]]), minlength=70)
    assert len(g["sim8"]) == 70 and len(pairs) % 2 == 1 and deg.max() == 40 and deg[20] == 0
    assert g["fixed"].sum() == 3 and g["fixed"][33] and any(g["fixed"][i] and g["fixed"][j] for i, j in pairs)
    assert 0 < g["fix_scale"].sum() < 70


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble], ids=["f64", "ld"])
def test_exp_log_round_trip_in_the_consistent_branches(dtype):
    rng = np.random.default_rng(0)
    tol = 1e-9 if dtype is np.float64 else 1e-12
    for th, sg in ((3e-6, 2e-6), (0.7, 3e-6), (0.7, 0.3), (2.9, -0.4)):      # small/small (first order), rotation only, both
        w = rng.standard_normal((50, 3))
        u = np.concatenate([th * w / np.linalg.norm(w, axis=1, keepdims=True), rng.uniform(-2, 2, (50, 3)), np.full((50, 1), sg)], 1).astype(dtype)
        stats = {}
        back = pgo_ref.sim3_log(pgo_ref.sim3_exp(u), stats)
        assert stats["quirk"] == 0
        # (the small-angle branch is first order by construction: I + Omega + Omega^2 and omega = deltaR / 2)
        assert np.abs(back - u).max() < (tol if th > 1e-5 else 1e-10), (th, sg, np.abs(back - u).max())


def test_matrix_to_quaternion_takes_all_four_branches():
    ax = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1.0]])
    u = np.zeros((8, 7))
    u[:4, :3] = 2.6 * ax / np.linalg.norm(ax, axis=1, keepdims=True)
    u[4:, :3] = 0.5 * ax / np.linalg.norm(ax, axis=1, keepdims=True)
    R = pgo_ref.rotmat(pgo_ref.sim3_exp(u)[:, :4])
    branches = []
    q = pgo_ref.quat_from_rotmat(R, branches)
    assert set(branches[0].tolist()) == {0, 1, 2, 3}
    assert np.abs(pgo_ref.rotmat(q) - R).max() < 1e-14


def test_kept_branch_is_the_formula_as_written():
    """|sigma| >= eps with a small rotation: B = ((0.5 sigma^2 - sigma + 1) s) / sigma^3, in exp and in log."""
    for sigma, theta in ((2e-5, 0.0), (-1e-3, 3e-6), (0.05, 9e-6)):
        s = np.exp(sigma)
        A, B, C, quirk = pgo_ref._abc(np.array([sigma]), np.array([s]), np.array([theta]), np.array([True]))
        assert quirk[0]
        assert B[0] == ((0.5 * sigma * sigma - sigma + 1) * s) / (sigma * sigma * sigma)
        assert A[0] == ((sigma - 1) * s + 1) / (sigma * sigma) and C[0] == (s - 1) / sigma
        assert abs(B[0]) > 1e3                      # ~ 1 / sigma^3, nowhere near 1/6
    # log of a state in that branch: W = A Omega + B Omega^2 + C I with that B, solved by LU
    S = np.array([[1e-3, -5e-4, 2e-4, 1.0, 0.3, -0.2, 0.5, np.exp(0.01)]])
    stats = {}
    e = pgo_ref.sim3_log(S, stats)[0]
    assert stats["quirk"] == 1
    R = pgo_ref.rotmat(S[:, :4])[0]
    om = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    Om = np.array([[0, -om[2], om[1]], [om[2], 0, -om[0]], [-om[1], om[0], 0]])
    sg, s = np.log(S[0, 7]), S[0, 7]
    W = ((sg - 1) * s + 1) / sg ** 2 * Om + ((0.5 * sg * sg - sg + 1) * s) / (sg * sg * sg) * (Om @ Om) + (s - 1) / sg * np.eye(3)
    assert np.allclose(e[:3], om, rtol=0, atol=1e-18) and np.allclose(W @ e[3:6], S[0, 4:7], rtol=1e-9)


def test_cholesky_and_lu_against_numpy():
    rng = np.random.default_rng(1)
    M = rng.standard_normal((30, 30))
    A, b = M @ M.T + 30 * np.eye(30), rng.standard_normal(30)
    assert np.allclose(pgo_ref.cholesky_solve(A, b), np.linalg.solve(A, b), rtol=1e-10)
    assert pgo_ref.cholesky_solve(A - 100 * np.eye(30), b) is None
    W, r = rng.standard_normal((20, 3, 3)), rng.standard_normal((20, 3))
    W[3, 0, 0] = 0     # a zero in the first pivot's place: the rows must be exchanged
    assert np.allclose(pgo_ref.lu3_solve(W, r), np.linalg.solve(W, r[..., None])[..., 0], rtol=1e-9)


def test_fix_scale_column_is_exactly_zero_and_fixed_block_is_zero():
    g, _ = pc.edge_block_case()
    (e, Ji, Jj), _ = pc.edge_block_refs()
    fs_i, fs_j = g["fix_scale"][g["vi"]].astype(bool), g["fix_scale"][g["vj"]].astype(bool)
    fx_i, fx_j = g["fixed"][g["vi"]].astype(bool), g["fixed"][g["vj"]].astype(bool)
    assert fs_i.any() and fs_j.any() and fx_i.any() and fx_j.any() and (fx_i & fx_j).any()
    assert np.all(Ji[fs_i][:, :, 6] == 0) and np.all(Jj[fs_j][:, :, 6] == 0)
    assert np.all(Ji[fx_i] == 0) and np.all(Jj[fx_j] == 0)
    assert np.all(np.abs(Ji[~fs_i & ~fx_i][:, :, 6]).max(-1) > 0)
    assert np.all(e[0] == 0)                        # the exactly zero error
