"""What a cs_ba handle holds once cs_ba_optimize has returned, and the one-level estimate backup (cs_ba_push / cs_ba_pop).

The contract (include/cubeslam_hip.h at cs_ba_optimize and cs_ba_push / cs_ba_pop):
  * an optimize call that ran at least one iteration leaves NO linear system on the handle: cs_ba_solve, cs_ba_update, cs_ba_get_system,
    cs_ba_get_reduced_system, cs_ba_get_vertex_hessians and cs_ba_pose_marginals return CS_ERR_NOT_RUN until cs_ba_compute_errors +
    cs_ba_build_system have run again; cs_ba_check_finite scans estimates and edge errors only;
  * cs_ba_pop needs a backup that cs_ba_push made and nothing has spent since (the structure phase, cs_ba_set_estimates, an optimize call
    that ran an iteration, an earlier pop).
Why: from its second iteration on cs_ba_optimize forms H_pl inside the Schur and back-substitution kernels and never writes it; behind an
accepted trial it linearises the next state before the verdict is in; its update kernel saves the estimates it replaces in the backup
buffers.  What is left in device memory is blocks of up to three states.

Cases (the smallest graphs that reach each path; `switches` are environment variables set around the case's handles):
  fused     make_problem(40, 2500, 8, seed=3)               stream flow + fused linearisation + cuboid elimination
  classic   the same, CS_BA_FUSE_LIN=0                       the control: the classic pair of kernels throughout
  pairs     the same, CS_BA_SCHUR_PAIRS=1                    pair-major Schur build, not fused
  bcr132    make_problem(23, 920, 0, seed=23)                no cuboid, the smallest banded system (132 unknowns)
  dense     make_problem(12, 400, 2, seed=5)                 under 128 unknowns: no stream flow, cs_ba_optimize pushes and pops on the host
  stereo    make_stereo_problem(0.5, 30, 1500, 0, seed=9)    stereo projection edges in the fused kernels
  stopped   the fused graph, optimize(64)                    leaves by a stopping rule behind an accepted, speculated trial
  rejected  the fused graph, user lambda 1e-8                rejected trials: pop + re-linearisation inside optimize (the oracle rejects two
                                                             trials in the second iteration; at 1e-6 this graph accepts every first trial)
Every graph carries odometry edges (synth_ba.make_problem), whose Jacobians are 1e-9-step differences.

Per case, after optimize(4) (64 for `stopped`):
  (a) the six calls are refused with CS_ERR_NOT_RUN and a text that names cs_ba_compute_errors + cs_ba_build_system; state() and
      check_finite() succeed, check_finite is clean; the estimates are bit-identical before and after the refused calls;
  (b) compute_errors() equals the last chi2 of history() at rtol 1e-9 (the bound test_stepwise_abi_driven_like_g2o_levenberg holds its chi2 to);
  (c) compute_errors + build_system against an independent reference at the handle's state: oracle/ba_oracle_py (ba_stereo_ref.Graph for the
      projection edges of `stereo`, plus the oracle's odometry terms).  Bounds of test_ba_gpu.py's test_system_parity_*: H_ll and H_pl (analytic)
      1e-11 of the matrix scale, H_pp and b (numeric Jacobians inside) 1e-5; vertex_hessians() equals the diagonal blocks of the H_pp and H_ll
      handed out, bit for bit;
  (d) solve(1e-3) and solve(30) against ba_numpy_ref.Reference on the system of (c): 1e-9 of max |x| (test_ba_solver_paths_gpu.py's (c));
  (e) pose_marginals of a camera diagonal, a camera-camera pair and a cuboid diagonal against numpy's inverse of the device's H_pp (1e-9) and
      of the reference's H_pp (1e-4): the bounds of test_pose_marginals_are_blocks_of_the_inverse_pose_hessian;
  (f) s = state(); the optimised handle and a fresh one both get set_estimates(*s), compute_errors, build_system, reduced_system(1e-3),
      solve(1e-3): every array bit-identical.  Control: the fresh handle against a second fresh one through the same calls.
Conditions asserted so that no case passes beside its path: the Schur layout, band_ld, >= 2 iterations, `stopped` done < 64, `rejected` a
trial count > 1, and H_pl of the reference at the start state and at the returned state differ by more than 1000 x the H_pl bound of (c), so a
stale H_pl cannot hide inside the tolerance.
Once, on the fused graph: (g) optimize(3); optimize(3) equals optimize(3) + three step-wise iterations (tests/ba_stepwise.py) from the state it
left; (h) the backup rules.
"""
import os
import re

import numpy as np
import pytest

import ba_numpy_ref
import ba_stepwise
import ba_stereo_ref
from cube_slam_wu_amd import capi, synth_ba
from oracle import ba_oracle_py as O

pytestmark = pytest.mark.gpu
NOT_RUN = r"\(-5\)"
WAY_FORWARD = r"\(-5\).*cs_ba_compute_errors \+ cs_ba_build_system"
LAMS = (1e-3, 30.0)
TOL_ANALYTIC, TOL_NUMERIC = 1e-11, 1e-5

CASES = {
    "fused": dict(graph="g40", fused=True),
    "classic": dict(graph="g40", env={"CS_BA_FUSE_LIN": "0"}, fused=True),
    "pairs": dict(graph="g40", env={"CS_BA_SCHUR_PAIRS": "1"}, fused=False),
    "bcr132": dict(graph="g23"),
    "dense": dict(graph="g12", band=False),
    "stereo": dict(graph="stereo30", fused=True),
    "stopped": dict(graph="g40", fused=True, iters=64),
    "rejected": dict(graph="g40", fused=True, lm=(1e-8, 10)),
}

_graphs, _runs = {}, {}


def _graph(name):
    if name not in _graphs:
        _graphs[name] = {
            "g40": lambda: synth_ba.make_problem(40, 2500, 8, seed=3),
            "g23": lambda: synth_ba.make_problem(23, 920, 0, seed=23),
            "g12": lambda: synth_ba.make_problem(12, 400, 2, seed=5),
            "stereo30": lambda: synth_ba.make_stereo_problem(0.5, n_cams=30, n_points=1500, n_cuboids=0, seed=9),
        }[name]()
    return _graphs[name]


def _rel(a, b):
    return np.abs(a - b).max() / max(1e-300, np.abs(b).max())


def reference_system(pr, state):
    """(chi2, H_pp, H_ll, H_pl, b) of the graph at `state`, by code that shares nothing with the device library."""
    cams, cubs, pts = state
    if len(pr.get("se_pt", [])) == 0:
        R = O.Problem(cams, pr["cam_fixed"], cubs, pr["cub_fixed"], pts, pr["pt_fixed"])
        R.set_edges_proj(pr["e_pt"], pr["e_cam"], pr["e_uv"], pr["e_info"], pr["e_intr"], pr["e_huber"])
        if len(pr["ce_cam"]):
            R.set_edges_cuboid(pr["ce_cam"], pr["ce_cub"], pr["ce_meas"], pr["ce_info"])
        R.set_edges_odom(pr["oe_i"], pr["oe_j"], pr["oe_meas"], pr["oe_info"])
        chi = R.compute_errors()[0]
        out = (chi,) + tuple(R.build_system())
        R.close()
        return out
    # mono + stereo projection edges: the numpy restatement; the odometry edges' share of H_pp and b_p from the oracle (cameras only: the
    # same pose columns)
    assert len(pr["cuboids"]) == 0
    G = ba_stereo_ref.Graph(cams, pr["cam_fixed"], pts, pr["pt_fixed"],
                            (pr["e_pt"], pr["e_cam"], pr["e_uv"], pr["e_info"], pr["e_intr"], pr["e_huber"]),
                            (pr["se_pt"], pr["se_cam"], pr["se_uvr"], pr["se_info"], pr["se_intr"], pr["se_huber"]))
    Hpp, Hll, Hpl, b = G.build_system()
    R = O.Problem(cams, pr["cam_fixed"], None, None, pts[:0], np.zeros(0, np.int32))
    R.set_edges_odom(pr["oe_i"], pr["oe_j"], pr["oe_meas"], pr["oe_info"])
    chi_o = R.compute_errors()[0]
    Hpp_o, _, _, b_o = R.build_system()
    R.close()
    assert Hpp_o.shape == Hpp.shape
    b = b.copy()
    b[:len(b_o)] += b_o
    return G.chi2() + chi_o, Hpp + Hpp_o, Hll, Hpl, b


def _edges_dict(pr):
    """The problem dict as ba_numpy_ref.Reference reads it: one projection-edge list, mono rows first (cs_ba_get_system's H_pl order)."""
    if len(pr.get("se_pt", [])) == 0:
        return pr
    d = dict(pr)
    d["e_pt"] = np.concatenate([pr["e_pt"], pr["se_pt"]]); d["e_cam"] = np.concatenate([pr["e_cam"], pr["se_cam"]])
    return d


def _refused(fn):
    """The exception text of a refused call; None if the call went through."""
    try:
        fn()
    except RuntimeError as e:
        return str(e)
    return None


def _linear_algebra(H, s):
    """(f)'s sequence on a handle: every array the calls return, by name."""
    H.set_estimates(*s)
    out = {"chi2": np.array(H.compute_errors())}
    for k, v in zip(("Hpp", "Hll", "Hpl", "b"), H.build_system()):
        out[k] = v
    S, r, cc, oc = H.reduced_system(1e-3)
    out.update(S=S, r=r, cam_col=cc, cub_col=oc)
    ok, x = H.solve(1e-3)
    out.update(ok=np.array(ok), x=x)
    return out


def _pairs(pr):
    """(e)'s vertex pairs: a camera diagonal, a camera-camera pair, a cuboid diagonal where the graph has cuboids."""
    nc = len(pr["cams"])
    pairs = [((0, 1), (0, 1)), ((0, nc // 2), (0, nc // 2 + 2))]
    if len(pr["cuboids"]):
        pairs.append(((1, len(pr["cuboids"]) - 1), (1, len(pr["cuboids"]) - 1)))
    return pairs


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _record(name):
    """Everything the device does for one case, in the order of the module docstring; nothing is asserted here."""
    c = CASES[name]
    pr = _graph(c["graph"])
    r = {"pr": pr}
    A = capi.ba_from_dict(pr)
    if "lm" in c:
        A.set_lm_params(*c["lm"])
    r["start"] = A.state()
    r["schur_layout"], r["solver_layout"] = A.schur_layout(), A.solver_layout()
    r["done"] = A.optimize(c.get("iters", 4))
    r["history"] = tuple(np.array(h) for h in A.history())
    # (a)
    s0 = A.state()
    pairs = _pairs(pr)
    r["refusals"] = {
        "cs_ba_solve": _refused(lambda: A.solve(1e-3)),
        "cs_ba_update": _refused(A.update),
        "cs_ba_get_system": _refused(A.system_vectors),
        "cs_ba_get_reduced_system": _refused(lambda: A.reduced_system(1e-3)),
        "cs_ba_get_vertex_hessians": _refused(A.vertex_hessians),
        "cs_ba_pose_marginals": _refused(lambda: A.pose_marginals(pairs)),
    }
    r["finite"] = A.check_finite()
    r["state_before"], r["state_after"] = s0, A.state()
    # (b)
    r["chi2"] = A.compute_errors()
    # (c)
    r["system"] = A.build_system()
    r["vertex_hessians"] = A.vertex_hessians()
    r["state"] = A.state()
    # (d)
    r["solves"] = [A.solve(lam) for lam in LAMS]
    # (e)
    r["pairs"] = pairs
    r["marginals"] = A.pose_marginals(pairs)
    # (f)
    s = A.state()
    B, C2 = capi.ba_from_dict(pr), capi.ba_from_dict(pr)
    r["f_A"], r["f_B"], r["f_C"] = _linear_algebra(A, s), _linear_algebra(B, s), _linear_algebra(C2, s)
    A.close(); B.close(); C2.close()
    return r


def _run(name):
    if name not in _runs:
        try:
            _runs[name] = _with_env(CASES[name].get("env", {}), lambda: _record(name))
        except Exception as e:      # (recorded once: every check of the case reports it)
            _runs[name] = e
    if isinstance(_runs[name], Exception):
        raise _runs[name]
    return _runs[name]


def _reference(r):
    """The independent reference at the state (c) rebuilt at, and H_pl at the start state (computed once per case)."""
    if "ref" not in r:
        r["ref"] = reference_system(r["pr"], r["state"])
        r["ref_Hpl_start"] = reference_system(r["pr"], r["start"])[3]
    return r["ref"]


case = pytest.mark.parametrize("name", list(CASES))


@case
def test_the_case_took_its_path(name):
    c, r = CASES[name], _run(name)
    if "fused" in c:
        assert r["schur_layout"][0] == c["fused"], r["schur_layout"]
    band_ld = r["solver_layout"][0]
    assert (band_ld > 0) if c.get("band", True) else (band_ld == 0), r["solver_layout"]
    assert r["done"] >= 2
    if name == "stopped":
        assert r["done"] < 64
    if name == "rejected":
        assert r["history"][2].max() > 1, r["history"][2]
    _reference(r)
    moved = _rel(r["ref_Hpl_start"], r["ref"][3])
    print(name, "iterations", r["done"], "trials", r["history"][2], "H_pl start vs returned state (reference):", moved)
    assert moved > 1000 * TOL_ANALYTIC


@case
def test_a_linear_system_calls_are_refused_after_optimize(name):
    r = _run(name)
    print(name, {k: (v if v is None else v[:60]) for k, v in r["refusals"].items()})
    for call, text in r["refusals"].items():
        assert text is not None, "%s went through after cs_ba_optimize" % call
        assert re.search(WAY_FORWARD, text), (call, text)
    n_bad, report = r["finite"]
    assert n_bad == 0 and report == "", report
    for a, b in zip(r["state_before"], r["state_after"]):
        assert np.array_equal(a, b)


@case
def test_b_chi2_of_the_returned_state_is_the_last_of_the_history(name):
    r = _run(name)
    last = r["history"][0][-1]
    print(name, "compute_errors", r["chi2"], "history", last, "relative", abs(r["chi2"] - last) / last)
    assert np.allclose(r["chi2"], last, rtol=1e-9, atol=0)


@case
def test_c_rebuilt_system_equals_the_reference(name):
    r = _run(name)
    pr = r["pr"]
    Hpp, Hll, Hpl, b = r["system"]
    chi_r, Hpp_r, Hll_r, Hpl_r, b_r = _reference(r)
    d = {"Hpp": _rel(Hpp, Hpp_r), "Hll": _rel(Hll, Hll_r), "Hpl": _rel(Hpl, Hpl_r), "b": _rel(b, b_r), "chi2": abs(r["chi2"] - chi_r) / chi_r}
    print(name, "relative to the reference:", d)
    assert d["Hll"] < TOL_ANALYTIC and d["Hpl"] < TOL_ANALYTIC
    assert d["Hpp"] < TOL_NUMERIC and d["b"] < TOL_NUMERIC
    for a, bb in zip(r["state"], r["state_after"]):      # (neither call moved the estimates)
        assert np.array_equal(a, bb)
    hc, ho, hp = r["vertex_hessians"]
    cam_g, cub_g = ba_numpy_ref.pose_columns(pr)
    for blocks, cols, dim in ((hc, cam_g, 6), (ho, cub_g, 9)):
        for i, k in enumerate(cols):
            assert np.array_equal(blocks[i], Hpp[k:k + dim, k:k + dim] if k >= 0 else np.zeros((dim, dim))), (dim, i)
    free = np.asarray(pr["pt_fixed"]) == 0
    assert np.array_equal(hp[free].reshape(-1, 9), Hll) and not hp[~free].any()


@case
def test_d_solves_on_the_rebuilt_system(name):
    r = _run(name)
    F = ba_numpy_ref.Reference(r["system"], _edges_dict(r["pr"]))
    for lam, (ok, x) in zip(LAMS, r["solves"]):
        ok_r, x_r = F.solve(lam)
        assert ok and ok_r, (lam, ok, ok_r)
        fe = np.abs(x - x_r).max() / np.abs(x_r).max()
        print(name, "lambda", lam, "forward error", fe)
        assert fe <= 1e-9, (lam, fe)


@case
def test_e_pose_marginals_on_the_rebuilt_system(name):
    r = _run(name)
    blocks, pd = r["marginals"]
    assert pd
    cam_g, cub_g = ba_numpy_ref.pose_columns(r["pr"])
    inv_g, inv_r = np.linalg.inv(r["system"][0]), np.linalg.inv(_reference(r)[1])
    for ((ca, ia), (cb, ib)), blk in zip(r["pairs"], blocks):
        r0, c0 = (cam_g, cub_g)[ca][ia], (cam_g, cub_g)[cb][ib]
        da, db = (6, 9)[ca], (6, 9)[cb]
        assert r0 >= 0 and c0 >= 0 and blk.shape == (da, db)
        dg, dr = _rel(blk, inv_g[r0:r0 + da, c0:c0 + db]), _rel(blk, inv_r[r0:r0 + da, c0:c0 + db])
        print(name, (ca, ia), (cb, ib), "against the device's H_pp", dg, "the reference's", dr)
        assert dg < 1e-9 and dr < 1e-4, ((ca, ia), (cb, ib), dg, dr)


@case
def test_f_nothing_of_optimize_leaks_into_the_next_linearisation(name):
    r = _run(name)
    differ = lambda p, q: [k for k in p if not np.array_equal(p[k], q[k])]
    control, leak = differ(r["f_B"], r["f_C"]), differ(r["f_A"], r["f_B"])
    print(name, "arrays that differ between two fresh handles:", control, "between the optimised and a fresh handle:", leak)
    assert control == [], "two fresh handles through the same calls are not bit-identical: %s" % control
    assert leak == [], leak


def test_g_a_second_optimize_continues_like_the_stepwise_calls():
    pr = _graph("g40")
    A, B = capi.ba_from_dict(pr), capi.ba_from_dict(pr)
    assert A.optimize(3) == 3 and B.optimize(3) == 3
    for a, b in zip(A.state(), B.state()):
        assert np.array_equal(a, b)
    n_a = A.optimize(3)
    chi_a, lam_a, tr_a = A.history()
    s = ba_stepwise.run(B, 3, B.state())
    assert len(s["chi2"]) == n_a == 3 and s["trials"] == list(tr_a)
    assert np.allclose(s["chi2"], chi_a, rtol=1e-9) and np.allclose(s["lam"], lam_a, rtol=1e-9)
    for a, b in zip(B.state(), A.state()):
        assert np.abs(a - b).max() < 1e-7 * max(1.0, np.abs(b).max())
    A.close(); B.close()


def test_h_pop_needs_a_live_backup():
    pr = _graph("g40")
    H = capi.ba_from_dict(pr)
    H.sizes()                                   # the structure phase has run; nothing was pushed
    s0 = H.state()
    with pytest.raises(RuntimeError, match=NOT_RUN):
        H.pop()
    for a, b in zip(H.state(), s0):
        assert np.array_equal(a, b)
    H.push()
    assert H.optimize(3) == 3                   # (its update kernel saves every trial's estimates in the backup buffers)
    s1 = H.state()
    assert not np.array_equal(s1[2], s0[2])
    with pytest.raises(RuntimeError, match=NOT_RUN):
        H.pop()
    for a, b in zip(H.state(), s1):
        assert np.array_equal(a, b)
    H.compute_errors(); H.build_system()
    H.push()
    ok, _ = H.solve(1.0)
    assert ok
    H.update()
    assert not np.array_equal(H.state()[2], s1[2])
    H.pop()
    for a, b in zip(H.state(), s1):
        assert np.array_equal(a, b)
    with pytest.raises(RuntimeError, match=NOT_RUN):
        H.pop()                                 # the backup is spent
    for a, b in zip(H.state(), s1):
        assert np.array_equal(a, b)
    H.push()
    H.set_estimates(*s0)                        # new estimates from the host: the backup is of another trajectory
    with pytest.raises(RuntimeError, match=NOT_RUN):
        H.pop()
    H.close()
