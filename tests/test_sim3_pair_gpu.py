"""cs_sim3_* / capi.Sim3Pairs (csrc/sim3_pair_kernels.hip, sim3_pair_host.cpp, cs_sim3_pair.h) against the numpy statement
tests/sim3_pair_ref.py.

The batches and their reference runs are tests/sim3_pair_cases.py's; the conditions under which a float64 reference can be compared at
all (same trials in float64 and long double, |rho| > 1e-6, classification margin > 1e-6, states of the two precisions within 1e-6) are
asserted there for every pair used here, in tests/test_sim3_pair_ref.py, without a GPU.

Contract: iterations_done and inlier flags identical; states (each pair against the largest of its eight numbers) and chi2 within 1e-5
relative; a fix_scale pair's scale bit for bit its input's; a pair's outputs the same bits at any position in any batch, through the
handle or the one-shot call.
"""
import numpy as np
import pytest

from cube_slam_wu_amd import capi
from cube_slam_wu_amd import synth_sim3_pairs as sp
import sim3_pair_cases as pc
import sim3_pair_ref as ref

pytestmark = pytest.mark.gpu

OUT_KEYS = ("S12", "inlier", "n_inliers", "chi2", "iterations")
INVALID = -1      # CS_ERR_INVALID_ARG


def _prm(**kw):
    return capi.sim3_pair_default_params(**kw)


def _same(a, b, what=""):
    for k in OUT_KEYS:
        assert np.array_equal(a[k], b[k]), (what, k)


def test_edge_blocks():
    """48 matches over 4 pairs (one fix_scale) through cs_sim3_pairs_linearize.  Tolerances: 100 x the reference's own
    float64-against-long-double deviation for the errors (floor 1e-13), 10 x for the Jacobians -- the device's libm differs from glibc by
    an ulp just as the two precisions differ, and 1 / (2 delta) = 5e8 multiplies it.  Reference's own deviation (per match, against the
    block's largest entry): errors 1.3e-14, Jacobians 1.7e-7.  Measured on an MI355X against the float64 reference: errors 0, Jacobians 0
    -- on these 48 matches the device's chain (no libm call sees more than a 1e-9 step) is the float64 reference's bit for bit."""
    b = pc.edge_batch()
    (e64, j64), (eld, jld) = pc.edge_blocks(), pc.edge_blocks(True)
    err, jac = capi.sim3_pairs_linearize(b)
    fs = np.repeat(b["fix_scale"].astype(bool), np.diff(b["match_ptr"]))
    assert np.isfinite(err).all() and np.isfinite(jac).all()
    assert fs.sum() == 12 and np.all(jac[fs][..., 6] == 0)          # a fix_scale pair: the seventh column exactly zero
    assert np.all(jac[~fs][:, 1, :, 6] != 0)
    failures = []
    for nm, got, r64, rld, factor, floor in (("err", err, e64, eld, 100, 1e-13), ("jac", jac, j64, jld, 10, 0.0)):
        ref_dev, dev = ref.block_deviation(r64, rld).max(), ref.block_deviation(got, r64).max()
        tol = max(factor * ref_dev, floor)
        print("%s: device %.3g, reference's own %.3g, tolerance %.3g" % (nm, dev, ref_dev, tol))
        if not dev <= tol:
            failures.append((nm, dev, tol))
    assert not failures, failures


def test_edge_blocks_with_distinct_intrinsics():
    """The same 48 matches with every pair's two cameras its own and fx != fy (tests/sim3_pair_cases.py: dense_edge_batch), under the
    tolerance rule of test_edge_blocks, unchanged.  Reference's own deviation: errors 1.2e-14, Jacobians 1.4e-7."""
    b = pc.dense_edge_batch()
    (e64, j64), (eld, jld) = pc.edge_blocks(False, True), pc.edge_blocks(True, True)
    err, jac = capi.sim3_pairs_linearize(b)
    fs = np.repeat(b["fix_scale"].astype(bool), np.diff(b["match_ptr"]))
    assert np.isfinite(err).all() and np.isfinite(jac).all() and np.all(jac[fs][..., 6] == 0)
    failures = []
    for nm, got, r64, rld, factor, floor in (("err", err, e64, eld, 100, 1e-13), ("jac", jac, j64, jld, 10, 0.0)):
        ref_dev, dev = ref.block_deviation(r64, rld).max(), ref.block_deviation(got, r64).max()
        tol = max(factor * ref_dev, floor)
        print("%s: device %.3g, reference's own %.3g, tolerance %.3g" % (nm, dev, ref_dev, tol))
        if not dev <= tol:
            failures.append((nm, dev, tol))
    assert not failures, failures


def test_dense_information_and_distinct_intrinsics_against_numpy_reference():
    """24 pairs over the lane-stride counts at schedule (3, 2), every pair with its own two cameras (fx != fy) and every edge with its own
    dense 2 x 2 information; min_inliers 8, under which 21 of the 24 run a second round (asserted in tests/test_sim3_pair_ref.py)."""
    b = pc.dense_batch()
    got = capi.sim3_optimize_pairs(b, _prm(**pc.DENSE))
    pc.compare_with_reference(got, pc.run("dense"), "device dense")
    assert 2 * int((got["iterations"][:, 1] > 0).sum()) >= 24


def test_batch_against_numpy_reference():
    """96 pairs at schedule (3, 2), match counts on the lane-stride boundaries, every second pair fix_scale.  Measured on an MI355X:
    states within 3.4e-7, chi2 within 7.9e-9 of the float64 reference (whose own long double spread is 4.4e-7 on the states)."""
    b = pc.main_batch()
    assert set(np.diff(b["match_ptr"]).tolist()) == set(pc.COUNTS)
    got = capi.sim3_optimize_pairs(b, _prm(**pc.SHORT))
    pc.compare_with_reference(got, pc.run("main"), "device main")
    fs = b["fix_scale"].astype(bool)
    assert fs.sum() == 48 and np.array_equal(got["S12"][fs, 7], b["S12"][fs, 7])       # exp(0) = 1 and s * 1 = s
    assert np.all(got["S12"][~fs, 7] != b["S12"][~fs, 7])


def test_degenerate_pairs():
    # a pair with 0 matches between two ordinary ones
    three = sp.synth_sim3_pairs(3, [20, 0, 20], 0.1, 21, pc.START)
    got = capi.sim3_optimize_pairs(three, _prm(**pc.SHORT))
    assert np.array_equal(got["S12"][1], three["S12"][1]) and got["iterations"][1].tolist() == [0, 0] and got["n_inliers"][1] == 0 and np.all(got["chi2"][1] == 0)
    _same(capi.sim3_optimize_pairs(sp.take_pairs(three, [1]), _prm(**pc.SHORT, min_inliers=0)), {k: v[1:2] if k != "inlier" else v[:0] for k, v in got.items()}, "alone")
    # 1, 2 and 3 matches: under-determined, nothing to compare -- finite states, and LM never accepts a step that raises chi2
    few = sp.synth_sim3_pairs(6, [1, 2, 3, 1, 2, 3], 0.0, 22, pc.START)
    got = capi.sim3_optimize_pairs(few, _prm(**pc.SHORT, min_inliers=0))
    assert np.isfinite(got["S12"]).all() and np.isfinite(got["chi2"]).all()
    err, _ = capi.sim3_pairs_linearize(few)
    for f in range(6):
        p = ref.pair_of(few, f)
        a, z = few["match_ptr"][f], few["match_ptr"][f + 1]
        c12, c21 = ref.chi2_each(p["W12"], err[a:z, :2])[0], ref.chi2_each(p["W21"], err[a:z, 2:])[0]
        initial = float((ref.huber(c12, np.sqrt(10.0))[0] + ref.huber(c21, np.sqrt(10.0))[0]).sum())
        assert got["chi2"][f, 0] <= initial * (1 + 1e-12), (f, got["chi2"][f, 0], initial)
        # round two runs on a subset of round one's matches, from the state and with the kernel round one ended with
        assert got["chi2"][f, 1] <= got["chi2"][f, 0] * (1 + 1e-12), (f, got["chi2"][f].tolist())
    # under min_inliers after round one: 0 inliers, no second round
    small = sp.synth_sim3_pairs(2, [12, 40], 0.1, 23, pc.START)
    got = capi.sim3_optimize_pairs(small, _prm(**pc.SHORT, min_inliers=13))
    assert got["n_inliers"][0] == 0 and got["iterations"][0].tolist() == [3, 0] and not got["inlier"][:12].any() and got["chi2"][0, 1] == 0
    assert got["n_inliers"][1] >= 13 and got["iterations"][1, 1] > 0 and got["inlier"][12:].sum() == got["n_inliers"][1]


def test_position_and_batch_size_do_not_change_a_pairs_bits():
    b = sp.take_pairs(pc.main_batch(), range(24))
    p = _prm(**pc.SHORT)
    whole = capi.sim3_optimize_pairs(b, p)
    perm = np.random.default_rng(5).permutation(24)
    shuffled = capi.sim3_optimize_pairs(sp.take_pairs(b, perm), p)
    ptr = b["match_ptr"]
    h = capi.Sim3Pairs()
    for pos, f in enumerate(perm):
        one = h.optimize(sp.take_pairs(b, [f]), p)
        sl = slice(ptr[f], ptr[f + 1])
        for k in ("S12", "n_inliers", "chi2", "iterations"):
            assert np.array_equal(shuffled[k][pos], whole[k][f]) and np.array_equal(one[k][0], whole[k][f]), (k, f)
        assert np.array_equal(one["inlier"], whole["inlier"][sl])
    assert np.array_equal(shuffled["inlier"], np.concatenate([whole["inlier"][ptr[f]:ptr[f + 1]] for f in perm]))
    h.close()


def test_handle_reused_over_growing_and_shrinking_batches_equals_one_shot():
    b = pc.main_batch()
    p = _prm(**pc.SHORT)
    h = capi.Sim3Pairs()
    with pytest.raises(RuntimeError):
        h.timing()                                                  # CS_ERR_NOT_RUN before the first call
    for idx in (range(2), range(40), range(5, 8), range(30, 96), range(1)):
        sub = sp.take_pairs(b, idx)
        _same(h.optimize(sub, p), capi.sim3_optimize_pairs(sub, p), str(idx))
        t = h.timing()
        assert t["kernel_ms"] > 0 and t["host_ms"] >= t["kernel_ms"]
    bad = {k: np.array(v, copy=True) for k, v in sub.items()}
    bad["S12"][0, 7] = -1.0
    with pytest.raises(RuntimeError):
        h.optimize(bad, p)
    assert h.timing() == t                                          # a refused call leaves the last run's timing in place
    h.close()


def test_default_schedule_agrees_where_rounding_cannot_decide():
    """32 pairs at the default parameters (5 iterations, then 10 or 5).  Iteration counts are NOT compared: at this schedule LM reaches the
    rounding floor of a 1e-9 central difference -- |rho| goes down to 2.5e-13 in the reference, and its float64 and long double runs already
    take different trial counts (tests/test_sim3_pair_ref.py) -- so the counts are decided by rounding in any implementation.  What
    rounding cannot decide is compared: the inlier flags (the reference's smallest margin |chi2 / th2 - 1| is 1.2e-4, asserted > 1e-6 here),
    states and chi2 within 1e-5 (the two precisions agree to 1.2e-7)."""
    res = pc.run("default")
    assert min(r["margin"] for r in res) > 1e-6
    got = capi.sim3_optimize_pairs(pc.default_batch())
    pc.compare_with_reference(got, res, "device default", iterations=False)
    assert np.all(got["iterations"][:, 0] >= 1) and np.all(got["iterations"] <= 10)


@pytest.mark.parametrize("name", list(pc.VARIANTS))
def test_parameter_variants(name):
    got = capi.sim3_optimize_pairs(pc.variant_pairs(name), _prm(**pc.VARIANTS[name]))
    pc.compare_with_reference(got, pc.run(name), "device " + name)
    if name == "clean_and_outlier_counts":
        its = [tuple(r) for r in got["iterations"].tolist()]
        assert (2, 1) in its and (2, 2) in its


def test_variants_differ_from_the_short_schedule():
    """The variants' parameters reach the kernel: each changes some pair's bits against the plain short schedule."""
    b = pc.variant_pairs("no_kernel")
    base = capi.sim3_optimize_pairs(b, _prm(**pc.SHORT))
    for name in ("no_kernel", "plain_second_round"):
        assert not np.array_equal(capi.sim3_optimize_pairs(b, _prm(**pc.VARIANTS[name]))["S12"], base["S12"]), name


def test_arguments_are_refused_before_any_launch():
    L = capi.lib()
    b = sp.take_pairs(pc.main_batch(), range(3))
    p = _prm()

    def call(batch, n_pairs=None):
        n, N, keep, args = capi._sim3_pair_inputs(batch)
        out = dict(S12=np.full((n, 8), 7.0), inlier=np.full(N, 7, np.uint8), n_inliers=np.full(n, 7, np.int32), chi2=np.full((n, 2), 7.0), iterations=np.full((n, 2), 7, np.int32))
        rc = L.cs_sim3_optimize_pairs(0, capi.C.byref(p), n if n_pairs is None else n_pairs, *args, capi._dp(keep[8]), capi._dp(keep[9]),
                                      capi._dp(out["S12"]), capi._u8p(out["inlier"]), capi._ip(out["n_inliers"]), capi._dp(out["chi2"]), capi._ip(out["iterations"]))
        return rc, all(np.all(v == 7) for v in out.values())

    def changed(key, index, value):
        c = {k: np.array(v, copy=True) for k, v in b.items()}
        c[key][index] = value
        return c

    assert call(b) == (0, False)
    for what, bad in (("a NaN point", changed("P1", (5, 1), np.nan)), ("an infinite keypoint", changed("obs2", (0, 0), np.inf)), ("s = 0", changed("S12", (1, 7), 0.0)),
                      ("s < 0", changed("S12", (2, 7), -1.2)), ("a decreasing match_ptr", changed("match_ptr", 2, int(b["match_ptr"][1]) - 1)),
                      ("match_ptr[0] != 0", changed("match_ptr", 0, 1))):
        assert call(bad) == (INVALID, True), what
        assert capi.last_error(), what
    assert call(b, n_pairs=-1) == (INVALID, True)
    n, N, keep, args = capi._sim3_pair_inputs(b)
    err, jac = np.full((N, 4), 7.0), np.full((N, 2, 2, 7), 7.0)
    nan = capi._sim3_pair_inputs(changed("P2", (0, 0), np.nan))
    assert L.cs_sim3_pairs_linearize(0, n, *nan[3], capi._dp(err), capi._dp(jac)) == INVALID and np.all(err == 7) and np.all(jac == 7)
    assert L.cs_sim3_pairs_linearize(0, -1, *args, capi._dp(err), capi._dp(jac)) == INVALID
    bad_p = _prm(iterations_first=101)
    with pytest.raises(RuntimeError):
        capi.sim3_optimize_pairs(b, bad_p)
