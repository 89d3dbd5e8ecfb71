"""Stereo projection edges (EdgeStereoSE3ProjectXYZ) in the device bundle adjustment against tests/ba_stereo_ref.py, a float64 numpy
restatement that shares no code with the product (pinned on the CPU by tests/test_ba_stereo_ref.py).

One graph family (ba_stereo_ref.make_family): 24 cameras, ~585 landmarks, camera 0 and landmark 0 fixed, track lengths 2 3 5 6 7 8 10 11 13 (every
class of the fused Schur schedule), one track of 18 cameras (the long-track kernel), a camera set seen by 40 landmarks (two segments), one seen by
a single landmark, half of the edges stereo with the kinds mixed inside tracks, one landmark behind a single stereo edge (its H_ll has full rank),
one with mono edges only.

Tolerances.  The Hessian blocks hold no single-precision quantity except through rho': 1e-9 of each block's largest entry.  chi2 and b contain the
stereo error, whose float invz moves by up to 6e-8 relative when z moves by an ulp: the project's standing 1e-5 relative.  The LM trajectory: the
same iterations, trials and accept / reject decisions (the reference's |rho| > 1e-6 for these seeds is asserted on the CPU), chi2 history and final
state within 1e-5 relative; three iterations, as tests/test_pose_only_gpu.py explains.

Not compared: the host-evaluated external-edge fallback (cs_ba_set_external_terms).  That interface gives a marginalised point unary terms only,
so it cannot express the point-camera block H_pl of a projection edge of either kind; the comparison the stereo edges would need does not exist in it.
"""
import os
import subprocess

import numpy as np
import pytest

import ba_stereo_ref as ref
from cube_slam_wu_amd import capi

pytestmark = pytest.mark.gpu
HUB = (np.sqrt(5.991), np.sqrt(7.815))


def _device(f, huber=None, mono=True, stereo=True):
    P = capi.BaProblem(f["cams"], f["cam_fixed"], None, None, f["points"], f["pt_fixed"])
    m, s = list(f["mono"]), list(f["stereo"])
    if huber is not None:
        m[5] = np.full(len(m[0]), huber[0]); s[5] = np.full(len(s[0]), huber[1])
    if mono and len(m[0]):
        P.set_edges_proj(*m[:5], m[5] if huber is not None else None)
    if stereo and len(s[0]):
        P.set_edges_proj_stereo(*s[:5], s[5] if huber is not None else None)
    return P


@pytest.fixture(scope="module")
def fam():
    return ref.make_family(seed=1)


def _rel(a, b, scale=None):
    return float(np.abs(a - b).max() / (np.abs(b).max() if scale is None else scale))


def _check_system(P, G, what):
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
        worst["Hll"] = max(worst["Hll"], _rel(hp[p], Hpt[p]))
        assert np.array_equal(Hll[G.lm[p]].reshape(3, 3), hp[p])
    nz = np.abs(Hpl_r).max((1, 2)) > 0
    assert np.array_equal(np.abs(Hpl).max(1) > 0, nz)             # the same edges have a block (free point and free camera), mono rows first
    d = np.abs(Hpl.reshape(-1, 6, 3) - Hpl_r).max((1, 2))[nz] / np.abs(Hpl_r).max((1, 2))[nz]
    worst["Hpl"] = float(d.max())
    worst["chi2"], worst["b"] = abs(chi_d - chi_r) / chi_r, _rel(b, b_r)
    print(what, "worst relative differences:", worst)
    assert max(worst["Hcc"], worst["Hll"], worst["Hpl"]) <= 1e-9
    assert worst["chi2"] <= 1e-5 and worst["b"] <= 1e-5
    return worst


def test_stepwise_system_equals_the_reference(fam):
    """chi2, every H_cc, H_ll, H_pl block and b at the initial state: no kernel, Huber on both classes, Cauchy on the stereo class alone."""
    P = _device(fam)
    G = ref.graph_of(fam)
    assert P.sizes() == (G.n_pose, 3 * int((G.lm >= 0).sum()))
    _check_system(P, G, "no kernel:")
    # the landmark behind one stereo edge has a full-rank H_ll; one behind one mono edge could not
    _, _, hp = P.vertex_hessians()
    assert np.linalg.matrix_rank(hp[fam["single_stereo"]]) == 3
    P.close()
    P = _device(fam, huber=HUB)
    _check_system(P, ref.graph_of(fam, huber=HUB), "Huber on both:")
    ns = len(fam["stereo"][0])
    kinds, deltas = np.full(ns, capi.RK_CAUCHY, np.int32), np.full(ns, 2.0)
    kinds[::3] = capi.RK_NONE
    P.set_robust_kernels(capi.EDGE_PROJ_STEREO, kinds, deltas)
    G = ref.graph_of(fam, huber=HUB, rk_stereo=(kinds, np.where(kinds > 0, deltas, 0.0)))
    _check_system(P, G, "Huber on mono, Cauchy on two thirds of the stereo edges:")
    assert P.check_finite()[0] == 0
    P.close()


def _check_trajectory(P, G, iters=3):
    n_d, n_r = P.optimize(iters), G.optimize(iters)
    chi_d, lam_d, tr_d = P.history()
    chi_r, lam_r, tr_r = G.history()
    assert all(abs(r) > 1e-6 for r in G.rho_log)
    print("chi2 device", chi_d, "reference", chi_r, "trials", tr_d, tr_r)
    assert n_d == n_r and np.array_equal(tr_d, tr_r)
    assert np.allclose(chi_d, chi_r, rtol=1e-5) and np.allclose(lam_d, lam_r, rtol=1e-4)
    cams_d, _, pts_d = P.state()
    cams_r, _, pts_r = G.state()
    scale = np.abs(pts_r).max()
    print("state: points", np.abs(pts_d - pts_r).max() / scale, "translations", np.abs(cams_d[:, :3] - cams_r[:, :3]).max() / scale)
    assert np.abs(pts_d - pts_r).max() <= 1e-5 * scale and np.abs(cams_d[:, :3] - cams_r[:, :3]).max() <= 1e-5 * scale
    assert np.abs(np.abs(np.sum(cams_d[:, 3:] * cams_r[:, 3:], axis=1)) - 1).max() <= 1e-5


def test_lm_trajectory_equals_the_reference(fam):
    P = _device(fam, huber=HUB)
    _check_trajectory(P, ref.graph_of(fam, huber=HUB))
    P.close()


def _check_fused_equals_stepwise(f, huber):
    """The body of test_fused_linearisation_equals_the_stepwise_calls on the graph f with the deltas huber (one per class, or an array per class)."""
    A = _device(f, huber=huber)
    assert A.optimize(3) == 3
    fused, n_seg, _, _ = A.schur_layout()
    assert fused and n_seg > 0 and A.solver_path() == "band"      # what cs_ba_optimize asks for before it fuses the linearisation
    chi_a, lam_a, tr_a = A.history()
    G = ref.graph_of(f, huber=huber)                                  # the fused route against the reference as well
    assert G.optimize(3) == 3 and all(abs(r) > 1e-6 for r in G.rho_log)
    assert np.array_equal(G.history()[2], tr_a) and np.allclose(chi_a, G.history()[0], rtol=1e-5)
    assert np.abs(A.state()[2] - G.state()[2]).max() <= 1e-5 * np.abs(G.state()[2]).max()
    B = _device(f, huber=huber)
    lam, ni, chi_b = 0.0, 2.0, []
    for it in range(3):
        cur = B.compute_errors()
        B.build_system(dense_hpp=False)
        if it == 0:
            hc, _, hp = B.vertex_hessians()
            free_c, free_p = np.asarray(f["cam_fixed"]) == 0, np.asarray(f["pt_fixed"]) == 0
            lam = 1e-5 * max(np.abs(np.einsum("cii->ci", hc[free_c])).max(), np.abs(np.einsum("pii->pi", hp[free_p])).max())
        q = 0
        while True:
            ok, x = B.solve(lam)
            assert ok
            b, _ = B.system_vectors()
            B.push(); B.update()
            tmp = B.compute_errors()
            rho = (cur - tmp) / (float(np.sum(x * (lam * x + b))) + 1e-3)
            if rho > 0:
                lam *= max(1.0 / 3.0, min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)); ni = 2.0; cur = tmp
            else:
                lam *= ni; ni *= 2; B.pop()
            q += 1
            if not (rho < 0 and q < 10):
                break
        assert q == tr_a[it]
        chi_b.append(cur)
    assert np.allclose(chi_b, chi_a, rtol=1e-9)
    for a, b in zip(A.state(), B.state()):
        if a.size:
            assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max()
    # and the classic pair inside cs_ba_optimize itself
    os.environ["CS_BA_FUSE_LIN"] = "0"
    try:
        Cc = _device(f, huber=huber)
        assert Cc.optimize(3) == 3
    finally:
        del os.environ["CS_BA_FUSE_LIN"]
    assert np.array_equal(Cc.history()[2], tr_a) and np.allclose(Cc.history()[0], chi_a, rtol=1e-9)
    for a, b in zip(A.state(), Cc.state()):
        if a.size:
            assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max()
    A.close(); B.close(); Cc.close()


def test_fused_linearisation_equals_the_stepwise_calls():
    """cs_ba_optimize linearises the landmark side inside the Schur kernels from its second iteration on (the fused schedule, no long track, banded
    solve: a 60-camera member of the family); the same LM steps driven through compute_errors / build_system / solve / push / update / pop use the classic kernels.  Same states to 1e-9."""
    f = ref.make_family(seed=2, long_track=False, n_cams=60)      # (60 cameras: the reduced system is banded, which the 24-camera graphs' is not)
    _check_fused_equals_stepwise(f, HUB)


def test_all_stereo_and_all_mono_graphs():
    """Share 1.0 against the reference; share 0.0 -- a handle that went through the stereo entry points but holds mono edges only -- bit for bit
    against a handle that never touched them."""
    f1 = ref.make_family(seed=1, stereo_share=1.0)
    P = _device(f1)
    _check_system(P, ref.graph_of(f1), "all stereo:")
    _check_trajectory(P, ref.graph_of(f1))
    P.close()
    f0 = ref.make_family(seed=1)
    A = _device(f0, huber=HUB, stereo=False)
    A.optimize(3)
    B = _device(f0, huber=HUB, stereo=True)          # stereo edges set, then taken away again, then an empty append
    s = f0["stereo"]
    B.set_edges_proj_stereo(s[0][:0], s[1][:0], s[2][:0], s[3][:0], s[4][:0])
    B.append_edges_proj_stereo(s[0][:0], s[1][:0], s[2][:0], s[3][:0], s[4][:0])
    B.optimize(3)
    for a, b in zip(A.history(), B.history()):
        assert np.array_equal(a, b)
    for a, b in zip(A.state(), B.state()):
        assert np.array_equal(a, b)
    A.close(); B.close()


def _two_components(seed=5):
    """Component A: cameras 0..11 (0 fixed), landmarks 0..59, mono edges only -- landmarks 0..47 seen by all 12 cameras (576 edges in the first
    group of 48 landmarks: more than ba_lin_pt_kernel stages, so the group walks its edges per landmark), landmarks 48..59 with tracks of 2..5 views.
    Component B: cameras 12..14 (12 fixed), landmarks 60..65, stereo edges only, every landmark seen by the three cameras.  No shared vertex."""
    rng = np.random.default_rng(seed)
    nc, n_pts = 15, 66
    cams = np.zeros((nc, 7)); cams[:, 6] = 1.0
    cams[:, :3] = rng.uniform(-0.3, 0.3, (nc, 3))
    q = np.concatenate([rng.uniform(-0.03, 0.03, (nc, 3)), np.ones((nc, 1))], axis=1)
    cams[:, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    pts = np.concatenate([rng.uniform(-2, 2, (n_pts, 2)), rng.uniform(4, 8, (n_pts, 1))], axis=1)
    fx, fy, cx, cy, bf = 520.0, 515.0, 320.0, 240.0, 40.0

    def project(c, p):
        x, y, z, w = cams[c, 3:]
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        pc = R @ pts[p] + cams[c, :3]
        u = fx * pc[0] / pc[2] + cx
        return u, fy * pc[1] / pc[2] + cy, u - bf / pc[2]

    m_pt, m_cam = [], []
    for p in range(48):
        m_pt += [p] * 12; m_cam += list(range(12))
    for p in range(48, 60):
        seen = np.sort(rng.choice(12, 2 + (p - 48) % 4, replace=False))
        m_pt += [p] * len(seen); m_cam += seen.tolist()
    s_pt = np.repeat(np.arange(60, 66), 3); s_cam = np.tile(np.arange(12, 15), 6)
    m_pt, m_cam = np.array(m_pt, np.int32), np.array(m_cam, np.int32)
    m_uv = np.array([project(c, p)[:2] for p, c in zip(m_pt, m_cam)]) + rng.normal(0, 1.5, (len(m_pt), 2))      # (1.5 px at unit information: a good part beyond Huber's width)
    s_uvr = np.array([project(c, p) for p, c in zip(s_pt, s_cam)]) + rng.normal(0, 1.5, (len(s_pt), 3))
    cam_fixed = np.zeros(nc, np.int32); cam_fixed[[0, 12]] = 1
    return dict(cams=cams, points=pts, cam_fixed=cam_fixed, pt_fixed=np.zeros(n_pts, np.int32),
                mono=(m_pt, m_cam, m_uv, np.tile(np.array([1.3, 0.2, 0.2, 0.9]), (len(m_pt), 1)), np.tile(np.array([fx, fy, cx, cy]), (len(m_pt), 1))),
                stereo=(s_pt.astype(np.int32), s_cam.astype(np.int32), s_uvr, np.tile(np.eye(3).ravel(), (len(s_pt), 1)), np.tile(np.array([fx, fy, cx, cy, bf]), (len(s_pt), 1))))


def test_mono_edges_in_a_stereo_graph_equal_the_mono_graph_bitwise():
    """A graph that holds a stereo edge runs the kernels' 3-row instantiations for ALL its edges; a mono edge fills rows 0 and 1 there and 'adds
    exact zeros to the sums the mono code forms' (ba_proj_edge.h).  Held here: component A (mono) together with component B (stereo, no shared
    vertex) against A alone, after compute_errors + build_system -- every A camera's 6 x 6 block, every A landmark's 3 x 3 block, every A edge's
    H_pl block and A's part of b, np.array_equal (which takes -0 for +0, as intended).  Without kernels, with Huber widths, with three A edges at level 1."""
    t = _two_components()
    mono, stereo = t["mono"], t["stereo"]
    n_m, n_a_cams, n_a_pts = len(mono[0]), 12, 60
    assert n_m > 576 and np.count_nonzero(mono[0] < 48) == 576      # the first group's edges: beyond LIN_PT_CAP
    levels = np.zeros(n_m, np.uint8); levels[[5, 300, n_m - 2]] = 1
    for what, huber, lvl in (("no kernel", None, None), ("Huber", HUB, None), ("three edges at level 1", HUB, levels)):
        U = capi.BaProblem(t["cams"], t["cam_fixed"], None, None, t["points"], t["pt_fixed"])
        A = capi.BaProblem(t["cams"][:n_a_cams], t["cam_fixed"][:n_a_cams], None, None, t["points"][:n_a_pts], t["pt_fixed"][:n_a_pts])
        hm = np.full(n_m, huber[0]) if huber is not None else None
        U.set_edges_proj(*mono, hm); A.set_edges_proj(*mono, hm)
        U.set_edges_proj_stereo(*stereo, np.full(len(stereo[0]), huber[1]) if huber is not None else None)
        if lvl is not None:
            U.set_edge_levels(capi.EDGE_PROJ, lvl); A.set_edge_levels(capi.EDGE_PROJ, lvl)
        U.compute_errors(); A.compute_errors()
        _, _, Hpl_u, b_u = U.build_system()
        _, _, Hpl_a, b_a = A.build_system()
        hc_u, _, hp_u = U.vertex_hessians()
        hc_a, _, hp_a = A.vertex_hessians()
        assert np.abs(hc_a[1:]).min(axis=(1, 2)).max() > 0 and np.abs(Hpl_a).max() > 0, what
        assert np.array_equal(hc_u[:n_a_cams], hc_a), what
        assert np.array_equal(hp_u[:n_a_pts], hp_a), what
        assert np.array_equal(Hpl_u[:n_m], Hpl_a), what
        # b in g2o's order: free cameras by id (A's eleven in front of B's two), then the landmarks by id (A's sixty in front of B's six)
        n_u, n_a = U.sizes()[0], A.sizes()[0]
        assert (n_u, n_a) == (6 * 13, 6 * 11) and len(b_a) == n_a + 3 * n_a_pts and np.abs(b_a).min() > 0, what
        assert np.array_equal(b_u[:n_a], b_a[:n_a]), what
        assert np.array_equal(b_u[n_u:n_u + 3 * n_a_pts], b_a[n_a:]), what
        if lvl is not None:
            assert np.all(Hpl_a[lvl == 1] == 0) and np.all(Hpl_u[:n_m][lvl == 1] == 0)
        U.close(); A.close()


def test_append_and_dump_load(fam, tmp_path):
    """A frame's stereo edges appended to an optimised graph = the graph built in one go at the same estimates; dump -> load -> the same run."""
    s = fam["stereo"]
    last = s[1] == 23                                  # the stereo edges of the last camera arrive later
    first = tuple(a[~last] for a in s[:5]); late = tuple(a[last] for a in s[:5])
    assert last.sum() > 0
    A = capi.BaProblem(fam["cams"], fam["cam_fixed"], None, None, fam["points"], fam["pt_fixed"])
    A.set_edges_proj(*fam["mono"][:5]); A.set_edges_proj_stereo(*first)
    A.optimize(2)
    cams, _, pts = A.state()
    A.append_edges_proj_stereo(*late)
    A.optimize(3)
    B = capi.BaProblem(cams, fam["cam_fixed"], None, None, pts, fam["pt_fixed"])
    B.set_edges_proj(*fam["mono"][:5]); B.set_edges_proj_stereo(*(np.concatenate([a, b]) for a, b in zip(first, late)))
    B.optimize(3)
    assert np.array_equal(A.history()[2], B.history()[2]) and np.allclose(A.history()[0], B.history()[0], rtol=1e-9)
    for a, b in zip(A.state(), B.state()):
        if a.size:
            assert np.abs(a - b).max() <= 1e-9 * np.abs(b).max()
    A.close(); B.close()
    # dump / load, kernels of both classes included; a mono graph's dump is what it was before the stereo class existed
    C1 = _device(fam, huber=HUB)
    ns = len(s[0])
    C1.set_robust_kernels(capi.EDGE_PROJ_STEREO, np.full(ns, capi.RK_CAUCHY, np.int32), np.full(ns, 2.0))
    path = str(tmp_path / "stereo.csba")
    C1.dump(path)
    C2 = capi.BaProblem.load(path, (len(fam["cams"]), 0, len(fam["points"]), len(fam["mono"][0]) + ns))
    C1.optimize(3); C2.optimize(3)
    for a, b in zip(C1.history(), C2.history()):
        assert np.array_equal(a, b)
    for a, b in zip(C1.state(), C2.state()):
        assert np.array_equal(a, b)
    C1.close(); C2.close()
    M = _device(fam, stereo=False)
    pm = str(tmp_path / "mono.csba")
    M.dump(pm)
    raw = open(pm, "rb").read()
    nm = len(fam["mono"][0])
    assert len(raw) == 8 + 64 + 24 * (7 * 8 + 4) + len(fam["points"]) * (3 * 8 + 4) + nm * (4 + 4 + 16 + 32 + 32)      # header, vertices, mono edges: nothing else
    assert np.frombuffer(raw[8:72], np.int32)[13:].tolist() == [0, 0, 0]
    M.close()


def test_refusals(fam):
    L = capi.lib()
    s = fam["stereo"]
    P = _device(fam)
    assert L.cs_ba_set_shard(P.h, 0, 2) == -1 and "stereo" in capi.last_error()
    assert L.cs_ba_set_shard(P.h, 0, 1) == 0
    pt, cam = np.ascontiguousarray(s[0][:4]), np.ascontiguousarray(s[1][:4])
    uvr, i9, k5 = (np.ascontiguousarray(a[:4], np.float64) for a in s[2:5])
    dp, ip = capi._dp, capi._ip
    assert L.cs_ba_set_edges_proj_stereo(P.h, 4, ip(pt), ip(cam), dp(uvr), None, dp(k5), None) == -1
    assert L.cs_ba_append_edges_proj_stereo(P.h, 4, ip(pt), ip(cam), dp(uvr), dp(i9), None, None) == -1
    P.close()
    Q = capi.BaProblem(fam["cams"], fam["cam_fixed"], None, None, fam["points"], fam["pt_fixed"])
    bad = s[0][:4].copy(); bad[2] = len(fam["points"])
    Q.set_edges_proj_stereo(bad, s[1][:4], s[2][:4], s[3][:4], s[4][:4])
    with pytest.raises(RuntimeError, match="out of range"):
        Q.compute_errors()
    Q.close()
    # a sharded handle takes no stereo edges either
    S = capi.BaProblem(fam["cams"], fam["cam_fixed"], None, None, fam["points"], fam["pt_fixed"])
    assert L.cs_ba_set_shard(S.h, 0, 2) == 0
    assert L.cs_ba_set_edges_proj_stereo(S.h, 4, ip(pt), ip(cam), dp(uvr), dp(i9), dp(k5), None) == -1
    S.close()
