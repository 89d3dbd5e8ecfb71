"""tests/pgo_ref.py on its own (no GPU): what the comparisons of tests/test_pgo_gpu.py rest on, asserted for every graph they use.

  (a) the float64 and the long-double run take the same trials, and their states agree to 1e-6 -- ten times inside the 1e-5 contract;
  (b) no trial's |rho| is below 1e-6 (the rule of test_pose_only_gpu.py: a decision that close is taken by rounding);
  (c) the graphs that are not the rejected-trial case never evaluate log in sim3.h:192's branch, and the rejected-trial case does;
  (d) chi2 and lambda histories of the two precisions agree to 5e-6, half the contract: they are more sensitive than the states (lambda's
      update 1 - (2 rho - 1)^3; the chi2 after a step from a far start), and the device differs from the float64 reference by errors of
      the kind and size float64 differs from long double by, so the reference's own share must leave the other half.  With seed 1 the
      far graph's lambda differed by 1.1e-5 between the two precisions; pgo_cases.SEED = 2 is a seed where it does not.
Measured (float64 against long double): state deviations 4e-8 .. 2.5e-7, chi2 1.2e-7 .. 1.8e-6 (the far graph), lambda <= 1.2e-7; the
rejected-trial graph: trials [1, 6], states 1.1e-7, chi2 3.2e-6.

The graphs with dense edge information (pgo_cases: fixscale_w, free_w, layout_w) and the 11 x 11 mesh go through the same four rules:
states 4.2e-8 .. 9.9e-8 (mesh 2.6e-7, 4.4e-7), chi2 1.2e-7 .. 2.8e-6 (fixscale_w; mesh 5e-8), lambda <= 2.2e-7, min |rho| 1.9e-5 (free_w,
lambda 1e-16).  Besides: the weighted optima lie more than 1e-3 from the unweighted ones (8e-3 .. 9e-2), so ignoring Omega cannot pass the
1e-5 contract; the information generator and the mesh are what they claim; the rounding bound of test_pgo_gpu.py's test_edge_terms
holds for float64 products and tells another edge's Omega, the identity and a transposed Omega; and the mesh's state after one step
differs by 4.9e-15 between three float64 factorisations, the yardstick of the back ends' comparison there.  That the mesh keeps a
dense tail in the sparse plan is tests/test_pgo_plan_cpu.py's."""
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


@pytest.mark.parametrize("name,lam,iterations", pc.weighted_runs(), ids=lambda v: str(v))
def test_weighted_optimum_is_not_the_unweighted_one(name, lam, iterations):
    """What makes the weighted runs a test of Omega: the same graph without information ends somewhere else -- 8e-3 (fixscale) to 9e-2
    (layout) in state, against the 1e-5 contract.  A generator that drifts toward the identity is noticed here."""
    a, b = pc.ref_run(name, lam, iterations), pc.ref_run(name[:-2], lam, iterations)
    sep = pgo_ref.state_deviation(a.est, b.est)
    print("%s lambda %g: weighted against unweighted %.3g" % (name, lam, sep))
    assert sep > 1e-3


def test_edge_information_is_what_it_claims():
    W = pc.edge_information(40, pc.INFO_SEED).reshape(-1, 7, 7)
    assert np.array_equal(W, W.transpose(0, 2, 1))                                                 # symmetric exactly
    ev = np.linalg.eigvalsh(W)
    assert ev.min() > 0.099 and ev.max() < 31.7 and (ev.max(-1) / ev.min(-1)).min() > 3            # 10 ** U(-1, 1.5) per axis, far from a multiple of I
    off = W * (1 - np.eye(7))
    assert np.abs(off).max(axis=(1, 2)).min() > 0.1                                                # every matrix has off-diagonal weight
    assert min(np.abs(W[a] - W[b]).max() for a in range(40) for b in range(a)) > 0.1               # another matrix for every edge
    for name in ("layout_w", "mesh"):
        g = pc.graph(name)
        assert g["info49"].shape == (len(g["vi"]), 49)
    # the per-edge products' matrices: every second one asymmetric, the others not
    T = pc.edge_terms_case()["info49"].reshape(-1, 7, 7)
    asym = np.abs(T - T.transpose(0, 2, 1)).max(axis=(1, 2))
    assert len(T) == 46 and np.all(asym[1::2] > 0.1) and np.all(asym[0::2] == 0)


def test_edge_terms_bound_holds_for_float64_products_and_tells_a_wrong_omega():
    """pgo_cases.edge_terms_expected, the yardstick of test_pgo_gpu.py's test_edge_terms, on the reference's own e, J_i, J_j: plain float64
    products (numpy's order, not the kernel's) stay inside the rounding bound; the same products with the NEXT edge's Omega, with the
    identity, or with Omega transposed do not -- the transposed one on the asymmetric matrices only."""
    g = pc.edge_terms_case()
    (e, Ji, Jj), _ = pc.edge_block_refs()
    W = g["info49"].reshape(-1, 7, 7)
    want = pc.edge_terms_expected(g["info49"], e, Ji, Jj)

    def worst(Wk):
        """Per edge: the largest error / bound over the six products formed in float64 with Wk (0 where both vanish)."""
        got = dict(Hii=np.einsum("kra,krc,kcb->kab", Ji, Wk, Ji), Hij=np.einsum("kra,krc,kcb->kab", Ji, Wk, Jj), Hjj=np.einsum("kra,krc,kcb->kab", Jj, Wk, Jj),
                   bi=-np.einsum("kra,krc,kc->ka", Ji, Wk, e), bj=-np.einsum("kra,krc,kc->ka", Jj, Wk, e), chi2=np.einsum("kr,krc,kc->k", e, Wk, e))
        out = np.zeros(len(Wk))
        for nm, (val, bound) in want.items():
            err = np.abs(got[nm].astype(np.longdouble) - val).reshape(len(Wk), -1)
            b = bound.reshape(len(Wk), -1)
            assert np.all(err[b == 0] == 0)
            out = np.maximum(out, (err / np.where(b > 0, b, 1)).max(-1).astype(float))
        return out

    assert worst(W).max() <= 1.0
    live = np.abs(e).max(-1) > 0                   # (the exactly zero error between two identities has J != 0 and still tells)
    assert worst(np.roll(W, -1, axis=0)).min() > 1e6 and worst(np.broadcast_to(np.eye(7), W.shape))[live].min() > 1e6
    t = worst(W.transpose(0, 2, 1))
    both_fixed = (g["fixed"][g["vi"]] & g["fixed"][g["vj"]]).astype(bool)      # (no Jacobian at all: e^T Omega e alone, which a transpose keeps)
    asym = np.arange(len(W)) % 2 == 1
    assert both_fixed.sum() == 1 and t[asym & ~both_fixed].min() > 1e6 and t[~asym | both_fixed].max() <= 1.0


def test_mesh_graph_is_what_it_claims():
    g = pc.mesh_graph()
    w = pc.MESH_SIDE
    pairs = list(zip(g["vi"].tolist(), g["vj"].tolist()))
    assert len(g["sim8"]) == 121 and len(pairs) == 320 and len({(min(p), max(p)) for p in pairs}) == 320
    assert sorted(np.flatnonzero(g["fixed"]).tolist()) == [0, 10, 60, 110, 120]
    assert np.array_equal(np.flatnonzero(g["fix_scale"]), np.arange(2, 121, 5))
    step = sorted({abs(i - j) for i, j in pairs})
    assert step == [1, w, w + 1]                                                                   # right, down, one diagonal
    straight = [(i, j) for i, j in pairs if abs(i - j) in (1, w)]
    assert all(((i % w) + (i // w)) % 2 == 0 for i, j in straight) and any(i > j for i, j in straight) and any(i < j for i, j in straight)
    G = pc.make_ref(g)
    assert len(pairs) > 256 and G.n == 7 * 116 > 256                                               # PGO_REDUCE_T


def test_mesh_factorisation_yardstick():
    """The mesh's states after one step from three float64 factorisations of the reference's system (pgo_cases.mesh_factorisation_deviation;
    measured 4.9e-15): 100 x this is the tolerance of test_pgo_gpu.py's test_back_ends_mesh.  After more iterations the deviation is
    carried through the numeric Jacobians and no longer a factorisation's (a similar mesh: 5e-6 after three), hence one iteration there."""
    dev = pc.mesh_factorisation_deviation()
    print("mesh, one step, three float64 factorisations: state deviation %.3g" % dev)
    assert 0 < dev < 1e-10


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
