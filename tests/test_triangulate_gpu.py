"""cs_triangulate_* / capi.Triangulate (csrc/triangulate_kernels.hip, triangulate_host.cpp, cs_triangulate.h) against the numpy statement
tests/triangulate_ref.py.

The batches and their reference runs are tests/triangulate_cases.py's; the conditions under which a float64 reference can be compared at
all (float64 and long double give every match the same status and route, and for every threshold comparison made the two differ by at
most a hundredth of the compared quantity's distance to its threshold) are asserted there for every match used here, in
tests/test_triangulate_ref.py, without a GPU.

Contract: status, route, ran and n_accepted identical to the reference; n_accepted the count of a pair's OK flags; X, normal, min_distance
and max_distance within max(100 x the reference's own float64-against-long-double deviation of that match, 1e-13), relative to |X|; the
inspection outputs cosRays, cosS1, cosS2 the same (absolute); a match's outputs the same bits at any position in any batch, through the
handle or the one-shot call.  Measured on an MI355X: deviation 0 of X, normal, the distances and
the three cosines on every batch (the reference's own float64-against-long-double spread is at most 2.2e-14 of |X|).
"""
import ctypes as C

import numpy as np
import pytest

from cube_slam_wu_amd import capi
from cube_slam_wu_amd import synth_ba
from cube_slam_wu_amd import synth_triangulate as st
import triangulate_cases as pc
import triangulate_ref as ref

pytestmark = pytest.mark.gpu

MATCH_OUT = ("X", "normal", "min_distance", "max_distance", "status", "route")
PAIR_OUT = ("ran", "n_accepted")
INVALID = -1      # CS_ERR_INVALID_ARG


def _prm(name="mixed"):
    return capi.triangulate_default_params(**pc.params_of(name))


def _same(a, b, what=""):
    for k in MATCH_OUT + PAIR_OUT:
        assert np.array_equal(a[k], b[k]), (what, k)


def _invariants(batch, got):
    ptr = batch["match_ptr"]
    assert got["n_accepted"].tolist() == [int((got["status"][ptr[f]:ptr[f + 1]] == ref.OK).sum()) for f in range(len(ptr) - 1)]
    assert set(np.unique(got["ran"]).tolist()) <= {0, 1} and got["status"].max(initial=0) <= ref.SCALE and got["route"].max(initial=0) <= ref.STEREO2
    off = np.repeat(got["ran"] == 0, np.diff(ptr))
    assert np.all(got["status"][off] == ref.PAIR_NOT_RUN) and np.all(got["status"][~off] != ref.PAIR_NOT_RUN)
    no_point = np.isin(got["status"], (ref.PAIR_NOT_RUN, ref.LOW_PARALLAX, ref.W_ZERO))
    assert np.all(got["X"][no_point] == 0) and np.all(np.isfinite(got["X"]))
    bad = got["status"] != ref.OK
    assert np.all(got["normal"][bad] == 0) and np.all(got["min_distance"][bad] == 0) and np.all(got["max_distance"][bad] == 0)
    assert np.all(got["route"][np.isin(got["status"], (ref.PAIR_NOT_RUN, ref.LOW_PARALLAX))] == ref.ROUTE_NONE)
    assert np.all(got["route"][~np.isin(got["status"], (ref.PAIR_NOT_RUN, ref.LOW_PARALLAX))] != ref.ROUTE_NONE)


@pytest.mark.parametrize("name", pc.NAMES)
def test_batches_against_the_reference(name):
    """Every batch of tests/triangulate_cases.py: the easy one (0, 1, 63, 64, 65 and 129 matches around the 64-match chunk, a monocular
    and a stereo pair that are not run), the mixed one (16 pairs x 70 matches, every sensor combination, the match families interleaved so
    that a wave holds several routes and statuses), and one pair with one match."""
    batch = pc.batch_of(name)
    got = capi.triangulate_pairs(batch, _prm(name))
    pc.compare_with_reference(got, pc.run(name), "device " + name)
    _invariants(batch, got)


def test_inspection_on_the_mixed_batch():
    batch = pc.mixed_batch()
    got = capi.triangulate_inspect(batch, _prm())
    pc.compare_with_reference(got, pc.run("mixed"), "device, inspection, mixed", cos=True)
    _same(got, capi.triangulate_pairs(batch, _prm()), "inspection against the run")
    # a pair that is not run hands out zeros
    got = capi.triangulate_inspect(st.take_pairs(pc.easy_batch(), pc.EASY_NOT_RUN), _prm("easy"))
    assert np.all(got["cos3"] == 0) and np.all(got["status"] == ref.PAIR_NOT_RUN) and not got["ran"].any()


def _per_pair(batch, out, f):
    a, b = int(batch["match_ptr"][f]), int(batch["match_ptr"][f + 1])
    return [out[k][a:b] for k in MATCH_OUT] + [out[k][f] for k in PAIR_OUT]


def test_same_bits_at_any_position_alone_and_through_the_handle():
    batch, p = st.concat_batches([pc.mixed_batch(), pc.easy_batch()]), _prm()
    whole = capi.triangulate_pairs(batch, p)
    _invariants(batch, whole)
    for name, first in (("mixed", 0), ("easy", pc.MIXED_PAIRS)):      # a concatenation gives each part the bits it has alone
        part, alone = pc.batch_of(name), capi.triangulate_pairs(pc.batch_of(name), p)
        for f in range(len(part["match_ptr"]) - 1):
            for x, y in zip(_per_pair(part, alone, f), _per_pair(batch, whole, first + f)):
                assert np.array_equal(x, y), (name, f)
    n = len(batch["match_ptr"]) - 1
    order = np.random.default_rng(1).permutation(n)
    sub = st.take_pairs(batch, order)
    shuffled = capi.triangulate_pairs(sub, p)
    for k, f in enumerate(order):
        for x, y in zip(_per_pair(sub, shuffled, k), _per_pair(batch, whole, f)):
            assert np.array_equal(x, y), f
    for f in (0, 5, pc.MIXED_PAIRS + 1, pc.MIXED_PAIRS + 5, n - 1):
        sub = st.take_pairs(batch, [f])
        for x, y in zip(_per_pair(sub, capi.triangulate_pairs(sub, p), 0), _per_pair(batch, whole, f)):
            assert np.array_equal(x, y), f
    h = capi.Triangulate()
    try:
        _same(h.run(batch, p), whole, "handle")
        _same(h.run(pc.single_batch(), p), capi.triangulate_pairs(pc.single_batch(), p), "handle, a smaller batch")
        _same(h.run(batch, p), whole, "handle, again")
        t = h.timing()
        assert t["kernel_ms"] > 0 and t["host_ms"] >= t["kernel_ms"]
        bad = {k: np.array(v, copy=True) for k, v in batch.items()}
        bad["kp1"][3, 4] = -1.0
        with pytest.raises(RuntimeError):
            h.run(bad, p)
        assert h.timing() == t                                      # a refused call leaves the last run's timing in place
    finally:
        h.close()


def test_empty_batches_and_pairs_are_valid():
    p = _prm()
    empty = st.take_pairs(pc.easy_batch(), [])
    got = capi.triangulate_pairs(empty, p)
    assert len(got["status"]) == 0 and len(got["ran"]) == 0
    got = capi.triangulate_pairs(st.take_pairs(pc.easy_batch(), [0, 0, 6]), p)      # pairs without a match; one of them not run
    assert len(got["status"]) == 40 and got["ran"].tolist() == [1, 1, 0] and got["n_accepted"].tolist() == [0, 0, 0]
    got = capi.triangulate_pairs(st.take_pairs(pc.easy_batch(), [0]), p)              # no match at all: nothing is launched
    assert len(got["status"]) == 0 and got["ran"].tolist() == [1] and got["n_accepted"].tolist() == [0]


def test_every_argument_check_refuses_and_leaves_the_outputs_untouched():
    L = capi.lib()
    b = st.take_pairs(pc.mixed_batch(), [1, 2, 3])
    n, N = 3, int(b["match_ptr"][-1])

    def call(batch, prm=None, n_pairs=None, null=None, fn="pairs"):
        """-> (return code, outputs untouched)"""
        p = prm if prm is not None else capi.triangulate_default_params()
        _, _, keep, args = capi._triangulate_inputs(batch)
        args = list(args)
        if null is not None:
            args[null] = None
        f3 = [np.full((N, 3), 7.0) for _ in range(3)]
        f1 = [np.full(N, 7.0) for _ in range(2)]
        u8 = [np.full(N, 9, np.uint8), np.full(N, 9, np.uint8), np.full(n, 9, np.uint8)]
        acc = np.full(n, 77, np.int32)
        tail = (capi._dp(f3[2]),) if fn == "inspect" else ()
        rc = getattr(L, "cs_triangulate_" + fn)(0, C.byref(p) if p != "null" else None, n if n_pairs is None else n_pairs, *args, capi._dp(f3[0]), capi._dp(f3[1]), capi._dp(f1[0]),
                                                capi._dp(f1[1]), capi._u8p(u8[0]), capi._u8p(u8[1]), capi._u8p(u8[2]), capi._ip(acc), *tail)
        return rc, bool(all(np.all(v == 7.0) for v in f3[:2] + f1) and all(np.all(v == 9) for v in u8) and np.all(acc == 77))

    def changed(key, at, value):
        c = {k: np.array(v, copy=True) for k, v in b.items()}
        c[key][at] = value
        return c

    assert call(b) == (0, False)
    stereo_at = int(np.flatnonzero(b["kp1"][:, 2] >= 0)[0])
    mono_at = int(np.flatnonzero(b["kp1"][:, 2] < 0)[0])
    zero_q = changed("Tcw2", (1, 3), 0.0)
    zero_q["Tcw2"][1, 3:] = 0.0
    for what, bad in (("a NaN quaternion", changed("Tcw1", (0, 4), np.nan)), ("an infinite quaternion", changed("Tcw2", (2, 6), np.inf)), ("a quaternion of zero norm", zero_q),
                      ("a NaN translation", changed("Tcw1", (1, 0), np.nan)),
                      ("fx = 0", changed("cam1", (0, 0), 0.0)), ("fy < 0", changed("cam2", (1, 1), -700.0)), ("fx NaN", changed("cam2", (2, 0), np.nan)), ("fy infinite", changed("cam1", (2, 1), np.inf)),
                      ("sigma2 = 0", changed("kp1", (5, 4), 0.0)), ("sigma2 NaN", changed("kp2", (N - 1, 4), np.nan)), ("scale < 0", changed("kp2", (0, 5), -1.2)),
                      ("scale infinite", changed("kp1", (7, 5), np.inf)),
                      ("depth = 0 beside ur >= 0", changed("kp1", (stereo_at, 3), 0.0)), ("depth NaN beside ur >= 0", changed("kp1", (stereo_at, 3), np.nan)),
                      ("depth infinite beside ur >= 0", changed("kp1", (stereo_at, 3), np.inf)),
                      ("a decreasing match_ptr", changed("match_ptr", 2, int(b["match_ptr"][1]) - 1)), ("match_ptr[0] != 0", changed("match_ptr", 0, 1))):
        assert call(bad) == (INVALID, True), what
        assert capi.last_error(), what
        assert call(bad, fn="inspect") == (INVALID, True), what
    assert call(changed("kp1", (mono_at, 3), np.nan)) == (0, False)      # a depth beside ur < 0 is not read
    for key in ref.PARAM_KEYS:
        for value in (0.0, -1.0, float("nan"), float("inf")):
            assert call(b, capi.triangulate_default_params(**{key: value})) == (INVALID, True), (key, value)
    assert call(b, "null") == (INVALID, True)
    assert call(b, n_pairs=-1) == (INVALID, True)
    for null in range(8):
        assert call(b, null=null) == (INVALID, True), null
    # null outputs
    p = capi.triangulate_default_params()
    _, _, keep, args = capi._triangulate_inputs(b)
    outs = [np.full((N, 3), 7.0), np.full((N, 3), 7.0), np.full(N, 7.0), np.full(N, 7.0), np.full(N, 9, np.uint8), np.full(N, 9, np.uint8), np.full(n, 9, np.uint8), np.full(n, 77, np.int32)]
    ptrs = [capi._dp(outs[0]), capi._dp(outs[1]), capi._dp(outs[2]), capi._dp(outs[3]), capi._u8p(outs[4]), capi._u8p(outs[5]), capi._u8p(outs[6]), capi._ip(outs[7])]
    for k in range(8):
        assert L.cs_triangulate_pairs(0, C.byref(p), n, *args, *[None if j == k else q for j, q in enumerate(ptrs)]) == INVALID, k
    assert L.cs_triangulate_inspect(0, C.byref(p), n, *args, *ptrs, None) == INVALID
    assert all(np.all(v == 7.0) for v in outs[:4]) and all(np.all(v == 9) for v in outs[4:7]) and np.all(outs[7] == 77)
    # the handle entry checks the same
    h = capi.Triangulate()
    try:
        with pytest.raises(RuntimeError):
            h.run(changed("cam1", (0, 0), 0.0), p)
        with pytest.raises(RuntimeError):
            h.timing()                                                 # nothing has run on it
        assert L.cs_triangulate_run(None, C.byref(p), n, *args, *ptrs) == INVALID
    finally:
        h.close()


def test_chain_new_points_into_bundle_adjustment():
    """LocalMapping's next step: the accepted points become landmarks of cs_ba, observed by the two keyframes that made them -- a mono
    edge where the keypoint has no right-image coordinate, a stereo edge where it has one, information 1 / sigma2.  cs_ba takes the
    vertices and edges, linearises them, and every new edge's plain chi2 is below the gate that accepted the match (5.991 / 7.8).  Nothing
    is optimised."""
    batch = st.take_pairs(pc.easy_batch(), [2, 3, 4])                  # stereo-stereo, mono-stereo, mono-mono: 63, 64 and 65 matches
    prm = _prm("easy")
    new = st.keep_accepted(batch, capi.triangulate_pairs(batch, prm))
    k = len(new["index"])
    assert k > 150 and np.all(np.isfinite(new["X"])) and np.all(new["min_distance"] < new["max_distance"])
    pr = synth_ba.make_stereo_problem(0.5, n_cams=10, n_points=200, n_cuboids=0, seed=9, huber=False)
    G = capi.ba_from_dict(pr)
    try:
        nc, npt = len(pr["cams"]), len(pr["points"])
        n_mono0, n_stereo0 = len(pr["e_pt"]), len(pr["se_pt"])
        n = len(batch["Tcw1"])
        G.append_vertices(cams=np.concatenate([batch["Tcw1"], batch["Tcw2"]]), cam_fixed=np.ones(2 * n), points=new["X"], pt_fixed=np.zeros(k))
        pt = np.concatenate([npt + np.arange(k)] * 2)
        cam = np.concatenate([nc + new["pair"], nc + n + new["pair"]])
        kp = np.concatenate([new["kp1"], new["kp2"]])
        intr = np.concatenate([batch["cam1"][new["pair"]], batch["cam2"][new["pair"]]])
        stereo = kp[:, 2] >= 0
        m, s = ~stereo, stereo
        assert m.sum() > 50 and s.sum() > 50
        G.append_edges_proj(pt[m], cam[m], kp[m, :2], np.array([1.0, 0, 0, 1.0]) / kp[m, 4:5], intr[m, :4], np.zeros(int(m.sum())))
        G.append_edges_proj_stereo(pt[s], cam[s], kp[s, :3], np.eye(3).ravel() / kp[s, 4:5], intr[s, :5], np.zeros(int(s.sum())))
        chi2 = G.compute_errors()
        assert np.isfinite(chi2)
        G.build_system(dense_hpp=False)
        _, c_mono, c_stereo = G.classify_edges(chi2_mono=prm.chi2_mono, chi2_stereo=prm.chi2_stereo, want_chi2=True)
        c_mono, c_stereo = c_mono[n_mono0:], c_stereo[n_stereo0:]
        assert len(c_mono) == m.sum() and len(c_stereo) == s.sum()
        print("%d new points, %d mono and %d stereo edges: largest chi2 %.3g (gate %.4g) and %.3g (gate %.4g)" % (k, m.sum(), s.sum(), c_mono.max(), prm.chi2_mono, c_stereo.max(), prm.chi2_stereo))
        assert np.all(c_mono < prm.chi2_mono) and np.all(c_stereo < prm.chi2_stereo)
        levels_m, levels_s = G.edge_levels(capi.EDGE_PROJ)[n_mono0:], G.edge_levels(capi.EDGE_PROJ_STEREO)[n_stereo0:]
        assert not levels_m.any() and not levels_s.any()               # positive depth in both keyframes, inside the gates: no new edge is an outlier
    finally:
        G.close()
