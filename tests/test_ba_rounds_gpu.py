"""Edge levels, kernels switched in place, the classification kernel and cs_ba_optimize_rounds (ORB-SLAM2's LocalBundleAdjustment on the device)
against tests/ba_rounds_ref.py -- ba_stereo_ref.Graph with "level 1" restated as "the edge left out" -- and, for cuboid / odometry edges,
oracle/ba_oracle_py.Problem on the sub-graph.  Neither shares code with the product; tests/test_ba_rounds_ref.py pins the reference on the CPU.

Cases (ba_rounds_ref.CASES): 24 cameras (dense reduced system, the long-track kernel), 60 cameras without the long track (banded solve, the
linearisation fused into the Schur kernels from the second iteration on), 24 cameras all mono.  5 % of the measurements carry N(0, 12) pixels;
Huber deltas sqrt(5.991) / sqrt(7.815).  The reference's own margins (no edge within 1e-3 relative of its threshold at either classification,
every |rho| > 1e-6) are asserted before the device is held to its decisions.

Tolerances are those the same references are held to elsewhere: tests/test_ba_stereo_gpu.py (blocks 1e-9 of the block's largest entry, chi2 and b
1e-5 -- the stereo error's float invz --, trajectory: equal iterations and trials, chi2 history rtol 1e-5, lambda rtol 1e-4, state 1e-5 of the
scale, quaternions 1e-5) and tests/test_ba_after_optimize_gpu.py (numeric-Jacobian blocks H_pp and b: 1e-5 of the matrix scale).
"""
import numpy as np
import pytest

import ba_rounds_ref as rr
import ba_stereo_ref as ref
from cube_slam_wu_amd import capi, synth_ba

pytestmark = pytest.mark.gpu
HUB, TH = rr.HUB, rr.TH
P_, S_ = capi.EDGE_PROJ, capi.EDGE_PROJ_STEREO


def _device(f, huber=HUB, cams=None, points=None):
    P = capi.BaProblem(f["cams"] if cams is None else cams, f["cam_fixed"], None, None, f["points"] if points is None else points, f["pt_fixed"])
    m, s = f["mono"], f["stereo"]
    if len(m[0]):
        P.set_edges_proj(*m[:5], np.full(len(m[0]), huber[0]) if huber else None)
    if len(s[0]):
        P.set_edges_proj_stereo(*s[:5], np.full(len(s[0]), huber[1]) if huber else None)
    return P


def _levels(P, f):
    return np.concatenate([P.edge_levels(P_, len(f["mono"][0])), P.edge_levels(S_, len(f["stereo"][0]))]).astype(bool)


def _set_levels(P, f, lv):
    nm = len(f["mono"][0])
    if nm:
        P.set_edge_levels(P_, lv[:nm].astype(np.uint8))
    if len(f["stereo"][0]):
        P.set_edge_levels(S_, lv[nm:].astype(np.uint8))


def _rel(a, b, scale=None):
    return float(np.abs(a - b).max() / (np.abs(b).max() if scale is None else scale))


def _state_close(cams_d, pts_d, cams_r, pts_r):
    scale = np.abs(pts_r).max()
    print("state: points", np.abs(pts_d - pts_r).max() / scale, "translations", np.abs(cams_d[:, :3] - cams_r[:, :3]).max() / scale)
    assert np.abs(pts_d - pts_r).max() <= 1e-5 * scale and np.abs(cams_d[:, :3] - cams_r[:, :3]).max() <= 1e-5 * scale
    assert np.abs(np.abs(np.sum(cams_d[:, 3:] * cams_r[:, 3:], axis=1)) - 1).max() <= 1e-5


_runs = {}


def _run(name, case=None, huber=HUB):
    """Per case, once: handle A through cs_ba_optimize_rounds; handle B through the calls it is made of, with the state and the levels between the
    rounds read out.  case = (graph, local_ba() of it) other than ba_rounds_ref.case(name), huber = its first round's deltas."""
    if name in _runs:
        return _runs[name]
    f, r = rr.case(name) if case is None else case
    rr.assert_comparable(r)
    out = {}
    A = _device(f, huber)
    A.compute_errors()                              # the structure phase, once
    out["digest0"], out["structure_ms0"] = A.structure_digest(), A.timing()["structure_ms"]
    out["done"], out["n_out"] = A.optimize_rounds(list(rr.LOCAL_BA))
    out["digest1"], out["structure_ms1"] = A.structure_digest(), A.timing()["structure_ms"]
    out["hist"], out["state"], out["levels"] = A.rounds_history(), A.state(), _levels(A, f)
    A.close()
    B = _device(f, huber)
    d1 = B.optimize(5); h1 = tuple(a.copy() for a in B.history())
    c1 = B.classify_edges(TH[0], TH[1], depth_positive=True, sticky=True)
    out["levels1"], out["state1"] = _levels(B, f), B.state()
    B.set_kernels_enabled(P_, False); B.set_kernels_enabled(S_, False)
    d2 = B.optimize(10); h2 = tuple(a.copy() for a in B.history())
    c2 = B.classify_edges(TH[0], TH[1], depth_positive=True, sticky=False)
    out["B"] = dict(done=(d1, d2), n_out=(c1, c2), hist=(h1, h2), state=B.state(), levels=_levels(B, f))
    B.close()
    _runs[name] = out
    return out


def _check_rounds(name, r, d):
    """The device's rounds d = _run() against the reference's r = local_ba(): levels, counts, histories, final state and classification."""
    nm = r["n_mono"]
    # after round 1: the reference's levels exactly, its counts per class
    assert np.array_equal(d["levels1"], r["out1"])
    assert tuple(d["n_out"][0]) == (int(r["out1"][:nm].sum()), int(r["out1"][nm:].sum()))
    # per round: iterations, trials, chi2 and lambda histories
    assert tuple(d["done"]) == r["done"]
    for k in range(2):
        chi_d, lam_d, tr_d = d["hist"][k]
        chi_r, lam_r, tr_r = r["hist"][k]
        print(name, "round", k, "chi2 device", chi_d, "reference", chi_r)
        assert np.array_equal(tr_d, tr_r)
        assert np.allclose(chi_d, chi_r, rtol=1e-5) and np.allclose(lam_d, lam_r, rtol=1e-4)
    # the final state and the final classification (every edge tested again)
    _state_close(d["state"][0], d["state"][2], *r["state2"])
    assert np.array_equal(d["levels"], r["out2"])
    assert tuple(d["n_out"][1]) == (int(r["out2"][:nm].sum()), int(r["out2"][nm:].sum()))


@pytest.mark.parametrize("name", list(rr.CASES))
def test_rounds_equal_the_reference(name):
    f, r = rr.case(name)
    d = _run(name)
    _check_rounds(name, r, d)
    # landmarks without an active edge in round 2 do not move by a bit (lambda I on their diagonal, a zero right-hand side)
    dead = (r["active1"][0] == 0) & (np.bincount(r["e_pt"], minlength=len(r["active1"][0])) > 0)
    assert dead.sum() >= 2
    assert np.array_equal(d["B"]["state"][2][dead], d["state1"][2][dead])
    assert not np.array_equal(d["B"]["state"][2][~dead][1:], d["state1"][2][~dead][1:])


@pytest.mark.parametrize("name", list(rr.CASES))
def test_rounds_run_no_structure_phase(name):
    d = _run(name)
    assert d["digest0"] == d["digest1"]
    assert d["structure_ms0"] > 0 and d["structure_ms1"] == d["structure_ms0"]


@pytest.mark.parametrize("name", list(rr.CASES))
def test_rounds_are_the_composition_of_the_single_calls(name):
    _check_composition(_run(name))


def _check_composition(d):
    b = d["B"]
    assert tuple(d["done"]) == b["done"]
    assert [tuple(x) for x in d["n_out"]] == [tuple(x) for x in b["n_out"]]
    for k in range(2):
        for x, y in zip(d["hist"][k], b["hist"][k]):
            assert np.array_equal(x, y)
    for x, y in zip(d["state"], b["state"]):
        assert np.array_equal(x, y)
    assert np.array_equal(d["levels"], b["levels"])


def _check_system(P, G, kept, what):
    """test_ba_stereo_gpu._check_system on a sub-graph: G holds the kept edges only (kept = their indices among all, mono first)."""
    chi_d, chi_r = P.compute_errors(), G.chi2()
    Hpp, Hll, Hpl, b = P.build_system()
    hc, _, hp = P.vertex_hessians()
    Hcam, bcam, Hpt, bpt, Hpl_r = G.build()
    _, _, _, b_r = G.build_system()
    worst = {"Hcc": 0.0, "Hll": 0.0, "Hpl": 0.0}
    for c in np.nonzero(G.cam_col >= 0)[0]:
        worst["Hcc"] = max(worst["Hcc"], _rel(hc[c], Hcam[c]))
        k = G.cam_col[c]
        assert np.array_equal(Hpp[k:k + 6, k:k + 6], hc[c])
    for p in np.nonzero(G.lm >= 0)[0]:
        if np.abs(Hpt[p]).max() == 0:
            assert np.abs(hp[p]).max() == 0          # a landmark without an active edge: an exact zero block
        else:
            worst["Hll"] = max(worst["Hll"], _rel(hp[p], Hpt[p]))
        assert np.array_equal(Hll[G.lm[p]].reshape(3, 3), hp[p])
    excluded = np.ones(len(Hpl), bool); excluded[kept] = False
    assert np.all(Hpl[excluded] == 0)                 # rows of level-1 edges: exactly zero
    Hk = Hpl[kept]
    nz = np.abs(Hpl_r).max((1, 2)) > 0
    assert np.array_equal(np.abs(Hk).max(1) > 0, nz)
    dd = np.abs(Hk.reshape(-1, 6, 3) - Hpl_r).max((1, 2))[nz] / np.abs(Hpl_r).max((1, 2))[nz]
    worst["Hpl"] = float(dd.max())
    worst["chi2"], worst["b"] = abs(chi_d - chi_r) / chi_r, _rel(b, b_r)
    print(what, "worst relative differences:", worst)
    assert max(worst["Hcc"], worst["Hll"], worst["Hpl"]) <= 1e-9
    assert worst["chi2"] <= 1e-5 and worst["b"] <= 1e-5
    return chi_d, Hpp, Hll, Hpl, b


def test_stepwise_calls_honour_levels():
    """A hand-set pattern on the 24-camera graph: every 7th mono edge, every 5th stereo edge, every edge of the landmark behind one stereo edge."""
    f, _ = rr.case("dense24")
    nm, ns = len(f["mono"][0]), len(f["stereo"][0])
    lv = np.zeros(nm + ns, bool)
    lv[:nm][::7] = True
    lv[nm:][::5] = True
    lv[nm:][f["stereo"][0] == f["single_stereo"]] = True
    lv[:nm][f["mono"][0] == f["single_stereo"]] = True
    P = _device(f)
    chi0 = P.compute_errors()
    sys0 = P.build_system()
    dig = P.structure_digest()
    _set_levels(P, f, lv)
    with pytest.raises(RuntimeError, match=r"\(-5\)"):          # CS_ERR_NOT_RUN: a level change leaves no linear system
        P.system_vectors()
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        P.solve(1e-3)
    G = rr.subgraph(f, f["cams"], f["points"], ~lv[:nm], ~lv[nm:], huber=HUB)
    _check_system(P, G, np.nonzero(~lv)[0], "levels set:")
    assert np.abs(P.vertex_hessians()[2][f["single_stereo"]]).max() == 0
    assert np.array_equal(_levels(P, f), lv) and P.structure_digest() == dig and P.check_finite()[0] == 0
    # the kernels switched off in place = the sub-graph without deltas; and back on
    P.set_kernels_enabled(P_, False); P.set_kernels_enabled(S_, False)
    _check_system(P, rr.subgraph(f, f["cams"], f["points"], ~lv[:nm], ~lv[nm:]), np.nonzero(~lv)[0], "levels set, kernels off:")
    P.set_kernels_enabled(P_, True); P.set_kernels_enabled(S_, True)
    # all levels cleared: the system the handle built before any was set, bit for bit
    P.set_edge_levels(P_, None); P.set_edge_levels(S_, None)
    assert P.compute_errors() == chi0
    for a, b in zip(P.build_system(), sys0):
        assert np.array_equal(a, b)
    assert P.structure_digest() == dig
    P.close()


def _tiny(bad_stereo):
    """Identity rotations, binary-exact coordinates: four cameras, twelve landmarks at depth 6 .. 10 seen by all of them, a thirteenth exactly at
    camera 1's centre seen by all four -- its edge to camera 1 projects a point at depth 0."""
    C_ = np.array([[0, 0, 0], [0.5, 0, 2], [1, 0, 0], [0, 0.5, 0]], float)
    cams = np.concatenate([-C_, np.tile([0, 0, 0, 1.0], (4, 1))], 1)
    X = np.array([[-1.5 + 0.25 * i + 0.125 * (i % 3), -0.75 + 0.125 * ((5 * i) % 11), 6 + 0.375 * ((7 * i) % 11)] for i in range(12)] + [list(C_[1])])
    cam_fixed, pt_fixed = np.array([1, 0, 0, 0], np.int32), np.zeros(13, np.int32)
    fx = fy = 512.0; cx, cy, bf = 320.0, 240.0, 256.0
    e_pt, e_cam = np.repeat(np.arange(13), 4), np.tile(np.arange(4), 13)
    bad = (e_pt == 12) & (e_cam == 1)
    Xc = X[e_pt] - C_[e_cam]
    Xc[bad] = [0.25, 0.125, 1.0]                           # (any finite measurement for the edge that is never evaluated)
    k = np.arange(len(e_pt))
    du, dv = 0.25 * ((k % 5) - 2), 0.125 * ((k % 7) - 3)   # the "noise": binary-exact offsets
    u, v = fx * Xc[:, 0] / Xc[:, 2] + cx + du, fy * Xc[:, 1] / Xc[:, 2] + cy + dv
    ur = u - bf / Xc[:, 2] + 0.125 * ((k % 3) - 1)
    st = (e_pt % 2 == 1)
    st[bad] = bad_stereo
    st[(e_pt == 12) & ~bad] = not bad_stereo
    m, s = ~st, st
    intr = np.tile([fx, fy, cx, cy], (len(e_pt), 1))
    mono = (e_pt[m].astype(np.int32), e_cam[m].astype(np.int32), np.stack([u, v], 1)[m], np.tile(np.eye(2).ravel(), (m.sum(), 1)), intr[m], np.zeros(m.sum()))
    stereo = (e_pt[s].astype(np.int32), e_cam[s].astype(np.int32), np.stack([u, v, ur], 1)[s], np.tile(np.eye(3).ravel(), (s.sum(), 1)),
              np.concatenate([intr[s], np.full((s.sum(), 1), bf)], 1), np.zeros(s.sum()))
    pts = X.copy()
    pts[:12] += 0.015625 * np.array([[(i % 3) - 1, ((i + 1) % 3) - 1, ((i + 2) % 3) - 1] for i in range(12)])      # start off the optimum; landmark 12 stays at the centre
    f = dict(cams=cams, cam_fixed=cam_fixed, points=pts, pt_fixed=pt_fixed, mono=mono, stereo=stereo)
    lv = np.concatenate([bad[m], bad[s]])
    return f, lv


@pytest.mark.parametrize("bad_stereo", [False, True])
def test_excluded_edge_at_depth_zero_never_reaches_a_sum(bad_stereo):
    f, lv = _tiny(bad_stereo)
    nm = len(f["mono"][0])
    assert lv.sum() == 1 and bool(lv[nm:].any()) == bad_stereo
    # (with the level cleared the reference itself is non-finite: that graph is never given to the device)
    with np.errstate(all="ignore"):
        assert not np.isfinite(rr.subgraph(f, f["cams"], f["points"], huber=HUB).chi2())
    P = _device(f)
    _set_levels(P, f, lv)
    n_bad, report = P.check_finite()
    assert n_bad == 0, report
    G = rr.subgraph(f, f["cams"], f["points"], ~lv[:nm], ~lv[nm:], huber=HUB)
    _check_system(P, G, np.nonzero(~lv)[0], "depth-0 edge excluded:")
    assert P.check_finite()[0] == 0                      # with the linear system on the handle
    n_d, n_r = P.optimize(3), G.optimize(3)
    assert all(abs(x) > 1e-6 for x in G.rho_log)
    chi_d, lam_d, tr_d = P.history()
    chi_r, lam_r, tr_r = G.history()
    print("chi2 device", chi_d, "reference", chi_r)
    assert n_d == n_r and np.array_equal(tr_d, tr_r) and np.all(np.isfinite(chi_d))
    assert np.allclose(chi_d, chi_r, rtol=1e-5) and np.allclose(lam_d, lam_r, rtol=1e-4)
    cams_d, _, pts_d = P.state()
    _state_close(cams_d, pts_d, G.cams7(), G.X)
    assert P.check_finite()[0] == 0
    P.close()


def test_depth_test_sticky_and_chi2_arrays():
    f, _ = rr.case("dense24")
    nm = len(f["mono"][0])
    G = ref.graph_of(f, huber=HUB)
    out_r, chi_r, _ = rr.classify(G)
    # (at the start state one edge of 4088 lies within 5e-4 of its threshold: the device is held to the reference's decision on every edge that is
    # clear of its threshold by ba_rounds_ref.MARGIN, and to its chi2 -- 1e-9 -- on all of them)
    th = np.where(G.stereo, TH[1], TH[0])
    clear = np.abs(chi_r / th - 1) > rr.MARGIN
    assert (~clear).sum() <= 4
    same = lambda lv, out, ok=clear: np.array_equal(lv[ok], out[ok])
    P = _device(f)
    (n_m, n_s), chi_m, chi_s = P.classify_edges(TH[0], TH[1], depth_positive=True, sticky=False, want_chi2=True)
    chi_d = np.concatenate([chi_m, chi_s])
    print("plain chi2 per edge, worst relative difference", np.abs(chi_d / chi_r - 1).max())
    assert np.abs(chi_d - chi_r).max() <= 1e-9 * np.abs(chi_r).max() and np.all(np.abs(chi_d / chi_r - 1) <= 1e-9)
    lv0 = _levels(P, f)
    assert same(lv0, out_r) and (n_m, n_s) == (int(lv0[:nm].sum()), int(lv0[nm:].sum())) and abs(n_m + n_s - int(out_r.sum())) <= int((~clear).sum())
    # a landmark of a two-camera track with a mono edge that is an inlier: reflected through that camera's centre it projects to the same pixel
    # at negative depth
    pick = None
    for p, tr in enumerate(f["tracks"]):
        if len(tr) == 2 and p != 0:
            e = np.nonzero(f["mono"][0] == p)[0]
            e = [k for k in e if not out_r[k] and chi_r[k] < 0.5 * TH[0]]
            if e:
                pick = (p, e[0]); break
    assert pick is not None
    p, e = pick
    c = f["mono"][1][e]
    R, t = ref.quat_to_R(f["cams"][c, 3:]), f["cams"][c, :3]
    centre = -R.T @ t
    pts = f["points"].copy()
    pts[p] = 2 * centre - pts[p]
    P.set_estimates(points=pts)
    Gm = rr.subgraph(f, f["cams"], pts, huber=HUB)
    out_m, chi_mr, _ = rr.classify(Gm, depth_positive=False)
    clear_m = np.abs(chi_mr / th - 1) > rr.MARGIN
    assert (~clear_m).sum() <= 4 and clear_m[e] and not out_m[e] and Gm.errors()[1][e, 2] < 0
    P.classify_edges(TH[0], TH[1], depth_positive=False, sticky=False)
    assert not _levels(P, f)[e] and same(_levels(P, f), out_m, clear_m)
    P.classify_edges(TH[0], TH[1], depth_positive=True, sticky=False)
    lv = _levels(P, f)
    assert lv[e] and same(lv, rr.classify(Gm)[0], clear_m)
    # the point back where it was: the edge's chi2 is small again.  sticky keeps it out, not sticky lets it return
    P.set_estimates(points=f["points"])
    P.classify_edges(TH[0], TH[1], depth_positive=True, sticky=True)
    lv_s = _levels(P, f)
    assert lv_s[e] and same(lv_s, lv | out_r, clear & clear_m) and np.array_equal(lv_s[lv], lv[lv])      # (nothing that was out came back)
    # a threshold <= 0 leaves the class alone
    P.classify_edges(0.0, TH[1], depth_positive=True, sticky=False)
    assert _levels(P, f)[e]
    P.classify_edges(TH[0], TH[1], depth_positive=True, sticky=False)
    assert not _levels(P, f)[e] and np.array_equal(_levels(P, f), lv0)
    P.close()


def test_cuboid_and_odometry_levels_against_the_oracle():
    from oracle import ba_oracle_py as O
    pr = synth_ba.make_problem(n_cams=12, n_points=300, n_cuboids=4, bbox_edges=True)
    n3, n4, n6 = len(pr["ce_cam"]), len(pr["pe_cam"]), len(pr["oe_i"])
    l3, l4, l6 = np.zeros(n3, bool), np.zeros(n4, bool), np.zeros(n6, bool)
    l3[::3] = True; l4[1::3] = True; l6[2::3] = True
    l3[pr["ce_cub"] == 1] = True; l4[pr["pe_cub"] == 1] = True          # cuboid 1 keeps no edge at all
    assert l3.sum() >= n3 // 3 and l4.sum() >= n4 // 3 and l6.sum() >= n6 // 3 and not l3.all() and not l6.all()
    P = capi.ba_from_dict(pr)
    chi0 = P.compute_errors(); sys0 = P.build_system(); dig = P.structure_digest()
    P.set_edge_levels(capi.EDGE_CUBOID, l3.astype(np.uint8)); P.set_edge_levels(capi.EDGE_CUBOID_PROJ, l4.astype(np.uint8)); P.set_edge_levels(capi.EDGE_ODOM, l6.astype(np.uint8))
    assert P.structure_digest() == dig
    R = O.Problem(pr["cams"], pr["cam_fixed"], pr["cuboids"], pr["cub_fixed"], pr["points"], pr["pt_fixed"])
    R.set_edges_proj(pr["e_pt"], pr["e_cam"], pr["e_uv"], pr["e_info"], pr["e_intr"], pr["e_huber"])
    R.set_edges_cuboid(pr["ce_cam"][~l3], pr["ce_cub"][~l3], pr["ce_meas"][~l3], pr["ce_info"][~l3])
    R.set_edges_cuboid_proj(pr["pe_cam"][~l4], pr["pe_cub"][~l4], pr["pe_meas"][~l4], pr["pe_info"][~l4], pr["pe_K"][~l4])
    R.set_edges_odom(pr["oe_i"][~l6], pr["oe_j"][~l6], pr["oe_meas"][~l6], pr["oe_info"][~l6])
    chi_d, chi_r = P.compute_errors(), R.compute_errors()[0]
    Hpp, Hll, Hpl, b = P.build_system()
    Hpp_r, Hll_r, Hpl_r, b_r = R.build_system()
    d = dict(chi2=abs(chi_d - chi_r) / chi_r, Hpp=_rel(Hpp, Hpp_r), Hll=_rel(Hll, Hll_r), Hpl=_rel(Hpl, Hpl_r), b=_rel(b, b_r))
    print("cuboid / odometry levels, relative to each matrix's scale:", d)
    assert d["Hpp"] <= 1e-5 and d["b"] <= 1e-5 and d["chi2"] <= 1e-5 and d["Hll"] <= 1e-11 and d["Hpl"] <= 1e-11
    assert P.check_finite()[0] == 0
    assert P.optimize(3) == R.optimize(3)
    assert np.array_equal(P.history()[2], R.history()[2]) and np.allclose(P.history()[0], R.history()[0], rtol=1e-5)
    scale = np.abs(R.state()[2]).max()
    for a, b_ in zip(P.state(), R.state()):
        assert np.abs(a - b_).max() <= 1e-5 * scale
    assert np.array_equal(P.edge_levels(capi.EDGE_CUBOID), l3) and np.array_equal(P.edge_levels(capi.EDGE_ODOM), l6)
    # levels cleared at the start estimates: the first system again, bit for bit
    P.set_estimates(pr["cams"], pr["cuboids"], pr["points"])
    for cls in (capi.EDGE_CUBOID, capi.EDGE_CUBOID_PROJ, capi.EDGE_ODOM):
        P.set_edge_levels(cls, None)
    assert P.compute_errors() == chi0
    for a, b_ in zip(P.build_system(), sys0):
        assert np.array_equal(a, b_)
    P.close(); R.close()


def test_append_dump_load_keep_levels_and_refusals(tmp_path):
    f, _ = rr.case("dense24")
    m, s = f["mono"], f["stereo"]
    nm, ns = len(m[0]), len(s[0])
    late_m, late_s = m[1] == 23, s[1] == 23                       # the last camera's edges arrive later
    assert late_m.sum() > 0 and late_s.sum() > 0
    order = lambda late: np.concatenate([np.nonzero(~late)[0], np.nonzero(late)[0]])
    om, os_ = order(late_m), order(late_s)
    f2 = dict(f, mono=tuple(a[om] for a in m), stereo=tuple(a[os_] for a in s))      # the same graph in the appended handle's edge order
    A = capi.BaProblem(f["cams"], f["cam_fixed"], None, None, f["points"], f["pt_fixed"])
    A.set_edges_proj(*(a[~late_m] for a in m[:5]), np.full(int((~late_m).sum()), HUB[0]))
    A.set_edges_proj_stereo(*(a[~late_s] for a in s[:5]), np.full(int((~late_s).sum()), HUB[1]))
    A.optimize(2)
    A.classify_edges(TH[0], TH[1], depth_positive=True, sticky=False)               # levels that exist on the device only
    lv_m, lv_s = A.edge_levels(P_).astype(bool), A.edge_levels(S_).astype(bool)
    assert lv_m.sum() > 20 and lv_s.sum() > 20
    A.append_edges_proj(*(a[late_m] for a in m[:5]), np.full(int(late_m.sum()), HUB[0]))
    A.append_edges_proj_stereo(*(a[late_s] for a in s[:5]), np.full(int(late_s.sum()), HUB[1]))
    want = np.concatenate([lv_m, np.zeros(late_m.sum(), bool), lv_s, np.zeros(late_s.sum(), bool)])
    assert np.array_equal(_levels(A, f2), want)                   # before the structure phase ...
    cams, _, pts = A.state()
    chi_a = A.compute_errors()
    assert np.array_equal(_levels(A, f2), want)                   # ... and after it
    # the same graph set up in one go at the same estimates, the levels set by hand (1e-9: cs_ba_set_vertices normalises the quaternions again,
    # the bound tests/test_ba_stereo_gpu.py's append test holds the same comparison to)
    B = _device(f2, cams=cams, points=pts)
    _set_levels(B, f2, want)
    assert abs(B.compute_errors() - chi_a) <= 1e-9 * chi_a
    for x, y in zip(A.build_system(), B.build_system()):
        assert np.abs(x - y).max() <= 1e-9 * np.abs(y).max()
    B.close()
    # dump / load: levels and the kernel switch come back; a handle without either dumps the bytes it always did
    A.set_kernels_enabled(S_, False)
    path = str(tmp_path / "levels.csba")
    A.dump(path)
    L2 = capi.BaProblem.load(path, (len(f["cams"]), 0, len(f["points"]), nm))
    L2.n_stereo = ns
    assert np.array_equal(_levels(L2, f2), want)
    A.optimize(3); L2.optimize(3)
    for x, y in zip(A.history(), L2.history()):
        assert np.array_equal(x, y)
    for x, y in zip(A.state(), L2.state()):
        assert np.array_equal(x, y)
    L2.close()
    C1, C2 = _device(f), _device(f)
    C2.set_edge_levels(P_, np.ones(nm, np.uint8)); C2.set_edge_levels(P_, None); C2.set_kernels_enabled(P_, False); C2.set_kernels_enabled(P_, True)
    p1, p2 = str(tmp_path / "a.csba"), str(tmp_path / "b.csba")
    C1.dump(p1); C2.dump(p2)
    assert open(p1, "rb").read() == open(p2, "rb").read()
    C1.close(); C2.close()
    # refusals: a wrong count, a level that is neither 0 nor 1, a sharded handle; the linear-system calls after a level change
    Lb = capi.lib()
    up = lambda a: a.ctypes.data_as(capi.C.POINTER(capi.C.c_ubyte))
    one = np.zeros(nm + 1, np.uint8)
    assert Lb.cs_ba_set_edge_levels(A.h, P_, nm - 1, up(one)) == -1 and "number of edges" in capi.last_error()
    assert Lb.cs_ba_set_edge_levels(A.h, P_, nm + 1, None) == -1
    assert Lb.cs_ba_get_edge_levels(A.h, S_, ns + 1, up(one)) == -1
    assert Lb.cs_ba_set_edge_levels(A.h, 7, 0, None) == -1
    two = np.full(nm, 2, np.uint8)
    assert Lb.cs_ba_set_edge_levels(A.h, P_, nm, up(two)) == -1
    A.compute_errors(); A.build_system()
    A.set_edge_levels(P_, None)
    for call in (lambda: A.solve(1e-3), A.update, A.system_vectors, A.vertex_hessians, lambda: A.reduced_system(1e-3)):
        with pytest.raises(RuntimeError, match=r"\(-5\)"):
            call()
    A.compute_errors(); A.build_system()
    A.classify_edges(TH[0], TH[1])
    with pytest.raises(RuntimeError, match=r"\(-5\)"):
        A.system_vectors()
    A.close()
    S = capi.BaProblem(f["cams"], f["cam_fixed"], None, None, f["points"], f["pt_fixed"])
    S.set_edges_proj(*m[:5])
    S.set_edge_levels(P_, (np.arange(nm) % 9 == 0).astype(np.uint8))
    assert Lb.cs_ba_set_shard(S.h, 0, 2) == -1 and "levels" in capi.last_error()      # a handle that holds levels is not sharded ...
    S.set_edge_levels(P_, None)
    S.set_shard(0, 2)                                                                  # ... and a sharded one takes none
    assert Lb.cs_ba_set_edge_levels(S.h, P_, nm, up(one)) == -1 and "sharded" in capi.last_error()
    cl = capi.CsBaClassify(TH[0], TH[1], 1, 0)
    assert Lb.cs_ba_classify_edges(S.h, capi.C.byref(cl), None, None, None) == -1
    rd = (capi.CsBaRound * 1)(capi.CsBaRound(1, 1, cl))
    assert Lb.cs_ba_optimize_rounds(S.h, rd, 1, None, None, None, None, None, 0) == -1
    S.close()
