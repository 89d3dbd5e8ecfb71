"""cs_sim3_ransac_* / capi.Sim3Ransac (csrc/sim3_ransac_kernels.hip, sim3_ransac_host.cpp, cs_sim3_ransac.h) against the numpy statement
tests/sim3_ransac_ref.py.

The batches and their reference runs are tests/sim3_ransac_cases.py's; the conditions under which a float64 reference can be compared at
all (float64 and long double classify every match of every hypothesis alike, and differ by at most a hundredth of the error's distance to
its threshold) are asserted there for every pair used here, in tests/test_sim3_ransac_ref.py, without a GPU.

Contract: found, hyp, iterations, n_inliers and the inlier flags identical; S12 within max(100 x the reference's own
float64-against-long-double deviation of that pair's S12, 1e-13), relative to the pair's largest entry; n_inliers the sum of the flags; a
fix_scale pair's s exactly 1; a pair's outputs the same bits at any position in any batch, through the handle or the one-shot call.  Measured on an MI355X: S12 deviation 0 on every batch and on all 300 hypotheses of the inspected pair.
"""
import ctypes as C

import numpy as np
import pytest

from cube_slam_wu_amd import capi
from cube_slam_wu_amd import synth_sim3_ransac as sr
import sim3_pair_ref as pair_ref
import sim3_ransac_cases as pc
import sim3_ransac_ref as ref

pytestmark = pytest.mark.gpu

OUT_KEYS = ("found", "hyp", "iterations", "S12", "inlier", "n_inliers")
INVALID = -1      # CS_ERR_INVALID_ARG


def _prm(name):
    p = pc.params_of(name)
    return capi.sim3_ransac_default_params(probability=p["probability"], min_inliers=p["min_inliers"], max_iterations=p["max_iterations"])


def _same(a, b, what=""):
    for k in OUT_KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)


def _invariants(batch, got):
    ptr = batch["match_ptr"]
    assert got["n_inliers"].tolist() == [int(got["inlier"][ptr[f]:ptr[f + 1]].sum()) for f in range(len(ptr) - 1)]
    assert set(np.unique(got["inlier"]).tolist()) <= {0, 1} and np.isfinite(got["S12"]).all()
    ran = got["hyp"] >= 0
    assert np.all(got["S12"][ran & (batch["fix_scale"] != 0), 7] == 1.0)
    assert np.all(got["S12"][~ran] == np.array(ref.IDENTITY)) and np.all(got["n_inliers"][~ran] == 0) and np.all(got["found"][~ran] == 0)
    assert np.all(got["iterations"][got["found"] == 1] == got["hyp"][got["found"] == 1] + 1)


@pytest.mark.parametrize("name", pc.NAMES)
def test_batches_against_the_reference(name):
    """Every batch of tests/sim3_ransac_cases.py: the easy one (match counts around the 64-match chunk and the 64-hypothesis block, pairs
    too small to run), the hard one (winners in the second and a later hypothesis block, pairs exhausted at 149 and at 300, a stored best
    that is the last of equals), the hard pairs at max_iterations 1, 63, 64, 65, and the degenerate pairs."""
    batch = pc.batch_of(name)
    got = capi.sim3_ransac_pairs(batch, _prm(name))
    pc.compare_with_reference(got, pc.run(name), "device " + name)
    _invariants(batch, got)


def test_every_hypothesis_of_a_hard_pair():
    sub = sr.take_pairs(pc.hard_batch(), [pc.HYPOTHESES_PAIR])
    S, cnt = capi.sim3_ransac_hypotheses(sub, pc.HYPOTHESES_COUNT)
    pc.compare_hypotheses(cnt[0], S[0], "device, every hypothesis of hard pair %d" % pc.HYPOTHESES_PAIR)
    # what the selection makes of them is what the run hands out
    got = capi.sim3_ransac_pairs(sub, _prm("hard"))
    h = int(got["hyp"][0])
    assert np.array_equal(S[0, h], got["S12"][0]) and cnt[0, h] == got["n_inliers"][0]
    # a pair without three matches has no hypothesis
    S, cnt = capi.sim3_ransac_hypotheses(sr.take_pairs(pc.degenerate_batch(), [1, 3]), 70)
    assert np.all(cnt == -1) and np.all(S == np.array(ref.IDENTITY))


def test_same_bits_at_any_position_alone_and_through_the_handle():
    batch, p = sr.concat_batches([pc.hard_batch(), pc.easy_batch()]), _prm("hard")
    whole = capi.sim3_ransac_pairs(batch, p)
    n = len(batch["intr"])
    ptr = batch["match_ptr"]
    order = np.random.default_rng(1).permutation(n)
    shuffled = capi.sim3_ransac_pairs(sr.take_pairs(batch, order), p)
    at = 0
    for k, f in enumerate(order):
        cnt = int(ptr[f + 1] - ptr[f])
        for key in ("found", "hyp", "iterations", "S12", "n_inliers"):
            assert np.array_equal(shuffled[key][k], whole[key][f]), (key, f)
        assert np.array_equal(shuffled["inlier"][at:at + cnt], whole["inlier"][ptr[f]:ptr[f + 1]]), f
        at += cnt
    for f in (0, 2, 5, n - 1):
        alone = capi.sim3_ransac_pairs(sr.take_pairs(batch, [f]), p)
        for key in ("found", "hyp", "iterations", "S12", "n_inliers"):
            assert np.array_equal(alone[key][0], whole[key][f]), (key, f)
        assert np.array_equal(alone["inlier"], whole["inlier"][ptr[f]:ptr[f + 1]]), f
    h = capi.Sim3Ransac()
    try:
        _same(h.run(batch, p), whole, "handle")
        _same(h.run(pc.degenerate_batch(), _prm("degenerate")), capi.sim3_ransac_pairs(pc.degenerate_batch(), _prm("degenerate")), "handle, a smaller batch")
        _same(h.run(batch, p), whole, "handle, again")
        t = h.timing()
        assert t["kernel_ms"] > 0 and t["host_ms"] >= t["kernel_ms"]
        bad = {k: np.array(v, copy=True) for k, v in batch.items()}
        bad["max_err1"][3] = -1.0
        with pytest.raises(RuntimeError):
            h.run(bad, p)
        assert h.timing() == t                                      # a refused call leaves the last run's timing in place
    finally:
        h.close()


def test_every_argument_check_refuses_and_leaves_the_outputs_untouched():
    L = capi.lib()
    b = pc.degenerate_batch()
    n = len(b["intr"])
    N = int(b["match_ptr"][-1])

    def call(batch, prm=None, n_pairs=None):
        """-> (return code, outputs untouched)"""
        p = prm if prm is not None else capi.sim3_ransac_default_params(min_inliers=2)
        _, _, keep, args = capi._sim3_ransac_inputs(batch)
        ints = [np.full(n, 77, np.int32) for _ in range(4)]
        S, inl = np.full((n, 8), 7.0), np.full(N, 9, np.uint8)
        rc = L.cs_sim3_ransac_pairs(0, C.byref(p), n if n_pairs is None else n_pairs, *args, capi._ip(ints[0]), capi._ip(ints[1]), capi._ip(ints[2]), capi._dp(S), capi._u8p(inl), capi._ip(ints[3]))
        return rc, bool(all(np.all(v == 77) for v in ints) and np.all(S == 7.0) and np.all(inl == 9))

    def changed(key, at, value):
        c = {k: np.array(v, copy=True) for k, v in b.items()}
        c[key][at] = value
        return c

    assert call(b) == (0, False)
    for what, bad in (("a NaN point", changed("P1", (5, 1), np.nan)), ("an infinite point", changed("P2", (0, 0), np.inf)), ("a NaN intrinsic", changed("intr", (2, 5), np.nan)),
                      ("a NaN threshold", changed("max_err1", 4, np.nan)), ("an infinite threshold", changed("max_err2", 4, np.inf)),
                      ("a negative threshold", changed("max_err2", N - 1, -1e-300)), ("a decreasing match_ptr", changed("match_ptr", 3, int(b["match_ptr"][2]) - 1)),
                      ("match_ptr[0] != 0", changed("match_ptr", 0, 1))):
        assert call(bad) == (INVALID, True), what
        assert capi.last_error(), what
    for what, kw in (("probability 0", dict(probability=0.0)), ("probability 1", dict(probability=1.0)), ("probability NaN", dict(probability=float("nan"))),
                     ("min_inliers < 0", dict(min_inliers=-1)), ("max_iterations 0", dict(max_iterations=0)), ("max_iterations 1025", dict(max_iterations=1025))):
        assert call(b, capi.sim3_ransac_default_params(**kw)) == (INVALID, True), what
    assert call(b, n_pairs=-1) == (INVALID, True)
    _, _, keep, args = capi._sim3_ransac_inputs(b)
    _, _, keep_nan, nan = capi._sim3_ransac_inputs(changed("P2", (0, 2), np.nan))
    S, cnt = np.full((n, 5, 8), 7.0), np.full((n, 5), 77, np.int32)
    assert L.cs_sim3_ransac_hypotheses(0, n, *nan, 5, capi._dp(S), capi._ip(cnt)) == INVALID
    for n_hyp in (0, 1025):
        assert L.cs_sim3_ransac_hypotheses(0, n, *args, n_hyp, capi._dp(S), capi._ip(cnt)) == INVALID
    assert L.cs_sim3_ransac_hypotheses(0, -1, *args, 5, capi._dp(S), capi._ip(cnt)) == INVALID
    assert np.all(S == 7.0) and np.all(cnt == 77)
    assert L.cs_sim3_ransac_hypotheses(0, n, *args, 5, capi._dp(S), capi._ip(cnt)) == 0 and not np.any(cnt == 77)
    # max_iterations 1024 is the largest budget, and is accepted
    got = capi.sim3_ransac_pairs(pc.hard_batch(), capi.sim3_ransac_default_params(max_iterations=1024, min_inliers=1000))
    assert np.all(got["hyp"] == -1) and np.all(got["iterations"] == 0)
    got = capi.sim3_ransac_pairs(pc.hard_batch(), capi.sim3_ransac_default_params(max_iterations=1024, probability=0.999999))
    assert got["iterations"].max() <= 1024 and np.all(got["found"] >= [r["found"] for r in pc.run("hard")])      # (the same hypotheses, more of them)
    _invariants(pc.hard_batch(), got)


def test_chain_ransac_then_optimize_pairs():
    """LoopClosing::ComputeSim3 on the device: RANSAC, keep the flagged matches, cs_sim3_optimize_pairs from S12_out.  The first round's
    robust chi2 does not exceed the robust chi2 at the RANSAC state (Levenberg-Marquardt accepts no step that raises it)."""
    batch = pc.easy_batch()
    got = capi.sim3_ransac_pairs(batch, _prm("easy"))
    found = np.flatnonzero(got["found"] == 1)
    assert len(found) >= 8
    sub = sr.keep_flagged(batch, got["inlier"], found)
    assert np.array_equal(np.diff(sub["match_ptr"]), got["n_inliers"][found]) and np.all(np.diff(sub["match_ptr"]) > 20)
    sub["S12"] = got["S12"][found].copy()
    prm = capi.sim3_pair_default_params()
    err, _ = capi.sim3_pairs_linearize(sub)
    out = capi.sim3_optimize_pairs(sub, prm)
    ptr = sub["match_ptr"]
    for k in range(len(found)):
        a, b = int(ptr[k]), int(ptr[k + 1])
        c12, _ = pair_ref.chi2_each(sub["info12"][a:b].reshape(-1, 2, 2), err[a:b, :2])
        c21, _ = pair_ref.chi2_each(sub["info21"][a:b].reshape(-1, 2, 2), err[a:b, 2:])
        start = float(pair_ref.huber(c12, prm.huber_delta)[0].sum() + pair_ref.huber(c21, prm.huber_delta)[0].sum())
        print("pair %d: %d matches kept, robust chi2 %.6g at the RANSAC state, %.6g after round one (%d iterations)" % (found[k], b - a, start, out["chi2"][k, 0], out["iterations"][k, 0]))
        assert out["chi2"][k, 0] <= start * (1 + 1e-12)
