"""cs_pose_optimize_batch / capi.PoseBatch (csrc/pose_kernels.hip) against the float64 numpy statement tests/pose_only_ref.py.

Tolerances: pose and chi2 within 1e-5 relative (the project's standing contract for BA states after the same iteration count; a pose
is compared against the largest magnitude of its seven numbers), iterations_done and inlier flags identical.

Condition on the inputs, asserted on the reference for every frame used (_checked_ref): no observation's chi2 within 1e-6 relative of its
threshold at any classification point, no LM trial's rho within 1e-6 of 0 -- a decision that close is taken by rounding, and no two
implementations need agree on it.  That is why these batches run 3 iterations per round from a start 0.1 rad / 0.5 m off: measured on
the reference, LM reaches its rounding floor in the 4th iteration from a 0.01 rad start (the 3rd with stereo edges, whose cam_project
keeps 1 / z in a float); from there every further trial is accepted or rejected by the sign of rounding noise (|rho| ~ 1e-10) and the
default schedule of 4 x 10 iterations meets the condition for no frame at all.  The default schedule is still run, in
test_default_schedule_agrees_where_rounding_cannot_decide, for what rounding cannot move: inlier flags, pose, chi2.

The generator's batches give every frame one camera with fx == fy and every observation a scalar times the identity as its information.
The second half of this file runs on tests/pose_cases.py's batches, which take those symmetries away (per-frame intrinsics, dense
per-observation information, garbage where a mono edge has no information) and pin the observation counts around the lane stride; their
conditions -- the two above and, for every factorisation, no pivot within 1e-6 of zero relative to the largest diagonal entry -- are
asserted for every frame in tests/test_pose_only_ref.py, without a GPU.  cs_pose_linearize_batch hands out the system itself, so that H
and b are compared directly and not only through where three LM iterations lead.

A trial whose factorisation fails: with positive semi-definite information H = sum J^T (rho' Omega) J is positive semi-definite and
lambda > 0, so no such batch produces one.  The ABI takes any 3 x 3 matrix, though, as g2o does, and with the information of some
observations sign-flipped H is indefinite: the reference then takes the branch deterministically (no pivot within 1e-6 of zero),
and test_failed_factorisations runs dense_lm_round's `!solved` path, lm_trial's DBL_MAX substitution and the pop against it.
"""
import numpy as np
import pytest

from cube_slam_wu_amd import capi, synth_pose
import pose_cases as pc
import pose_only_ref as ref

pytestmark = pytest.mark.gpu

SCHEDULE = dict(iterations=[3, 3, 3, 3])
START = (0.1, 0.5)


def _params(**kw):
    kw = dict(SCHEDULE, **kw)
    return capi.pose_default_params(**kw), kw


def _batch(stereo_share, seed, n_main=254):
    main = synth_pose.synth_pose_batch(n_main, (50, 1000), stereo_share, 0.1, seed, pose_sigma=START)
    edge = synth_pose.synth_pose_batch(2, [0, 3], stereo_share, 0.0, seed + 1000, pose_sigma=START)
    return synth_pose.concat_batches([main, edge])


def _checked_ref(batch, kw):
    res = ref.optimize_batch(batch, kw)
    for f, r in enumerate(res):
        assert r["margin"] > 1e-6, (f, r["margin"])
        assert len(r["rho"]) == 0 or np.abs(r["rho"]).min() > 1e-6, (f, np.abs(r["rho"]).min())
    return res


def _compare(got, res, batch, what):
    ptr = batch["obs_ptr"]
    worst_pose = worst_chi = 0.0
    for f, r in enumerate(res):
        assert np.array_equal(got["iterations"][f], r["iterations"]), (what, f, got["iterations"][f], r["iterations"])
        assert np.array_equal(got["inlier"][ptr[f]:ptr[f + 1]].astype(bool), r["inlier"]), (what, f)
        worst_pose = max(worst_pose, np.abs(got["Tcw"][f] - r["pose"]).max() / np.abs(r["pose"]).max())
        worst_chi = max(worst_chi, np.abs(got["chi2"][f] - r["chi2"]).max() / max(np.abs(r["chi2"]).max(), 1e-300))
    print("%s: %d frames, worst relative pose error %.3g, worst relative chi2 error %.3g" % (what, len(res), worst_pose, worst_chi))
    assert worst_pose < 1e-5 and worst_chi < 1e-5, (what, worst_pose, worst_chi)


@pytest.mark.parametrize("stereo_share,seed", [(0.0, 11), (0.5, 12), (1.0, 13)], ids=["mono", "mixed", "stereo"])
def test_batch_against_numpy_reference(stereo_share, seed):
    batch = _batch(stereo_share, seed)
    counts = np.diff(batch["obs_ptr"])
    assert len(counts) >= 256 and 0 in counts and 3 in counts and counts.max() <= 1000
    p, kw = _params()
    res = _checked_ref(batch, kw)
    got = capi.pose_optimize_batch(batch, p)
    _compare(got, res, batch, "stereo share %.1f" % stereo_share)
    empty = int(np.where(counts == 0)[0][0])
    assert np.array_equal(got["iterations"][empty], [0, 0, 0, 0])
    assert np.array_equal(got["Tcw"][empty], ref.se3_from_vector(batch["Tcw"][empty]))


def test_mono_frames_against_cs_ba_optimize():
    """One round, no classification: the same frame as a one-camera BaProblem whose points are all fixed, on the same device."""
    batch = synth_pose.synth_pose_batch(12, (50, 400), 0.0, 0.1, 21, pose_sigma=START)
    p, kw = _params(n_rounds=1, iterations=[3], robust_rounds=1, chi2_mono=0.0, chi2_stereo=0.0)
    _checked_ref(batch, kw)
    got = capi.pose_optimize_batch(batch, p)
    ptr = batch["obs_ptr"]
    for f in range(12):
        s = slice(ptr[f], ptr[f + 1])
        n = ptr[f + 1] - ptr[f]
        G = capi.BaProblem(batch["Tcw"][f][None], [0], points=batch["Xw"][s], pt_fixed=np.ones(n))
        G.set_edges_proj(np.arange(n), np.zeros(n), batch["meas"][s][:, :2], batch["info"][s][:, [0, 1, 3, 4]], np.tile(batch["intr"][f][:4], (n, 1)),
                         np.full(n, p.huber_mono))
        done = G.optimize(3)
        chi = G.history()[0]
        pose = G.state()[0][0]
        G.close()
        assert done == got["iterations"][f][0]
        assert np.abs(pose - got["Tcw"][f]).max() < 1e-5 * np.abs(pose).max(), (f, pose, got["Tcw"][f])
        assert abs(chi[done - 1] - got["chi2"][f][0]) < 1e-5 * chi[done - 1], (f, chi, got["chi2"][f])
        assert got["inlier"][s].all()


def test_position_and_batch_size_do_not_change_a_frames_bits():
    batch = _batch(0.5, 31, n_main=62)
    p, _ = _params()
    n = len(batch["Tcw"])
    got = capi.pose_optimize_batch(batch, p)
    perm = np.random.default_rng(5).permutation(n)
    got_p = capi.pose_optimize_batch(synth_pose.take_frames(batch, perm), p)
    ptr = batch["obs_ptr"]
    ptr_p = np.concatenate([[0], np.cumsum(np.diff(ptr)[perm])])
    for k, f in enumerate(perm):
        assert np.array_equal(got_p["Tcw"][k], got["Tcw"][f]) and np.array_equal(got_p["chi2"][k], got["chi2"][f])
        assert np.array_equal(got_p["iterations"][k], got["iterations"][f])
        assert np.array_equal(got_p["inlier"][ptr_p[k]:ptr_p[k + 1]], got["inlier"][ptr[f]:ptr[f + 1]])
    for f in (0, 17, n - 1):
        one = capi.pose_optimize_batch(synth_pose.take_frames(batch, [f]), p)
        assert np.array_equal(one["Tcw"][0], got["Tcw"][f]) and np.array_equal(one["chi2"][0], got["chi2"][f])
        assert np.array_equal(one["iterations"][0], got["iterations"][f]) and np.array_equal(one["inlier"], got["inlier"][ptr[f]:ptr[f + 1]])


def test_handle_reused_over_growing_and_shrinking_batches_equals_one_shot():
    p, _ = _params()
    h = capi.PoseBatch()
    for n_frames, seed in ((8, 41), (96, 42), (3, 43)):
        batch = synth_pose.synth_pose_batch(n_frames, (50, 600), 0.5, 0.1, seed, pose_sigma=START)
        a, b = h.optimize(batch, p), capi.pose_optimize_batch(batch, p)
        for k in ("Tcw", "inlier", "chi2", "iterations"):
            assert np.array_equal(a[k], b[k]), (n_frames, k)
        t = h.timing()
        assert t["kernel_ms"] > 0 and t["host_ms"] >= t["kernel_ms"]
    h.close()


@pytest.mark.parametrize("kw", [dict(robust_rounds=0), dict(restart_each_round=0, n_rounds=2, iterations=[2, 2], robust_rounds=1), dict(n_rounds=1, iterations=[3])],
                         ids=["robust_rounds=0", "restart_each_round=0", "n_rounds=1"])
def test_parameter_variants(kw):
    batch = synth_pose.synth_pose_batch(32, (50, 400), 0.5, 0.1, 54, pose_sigma=START)
    p, kw = _params(**kw)
    res = _checked_ref(batch, kw)
    _compare(capi.pose_optimize_batch(batch, p), res, batch, str(kw))


def test_default_schedule_agrees_where_rounding_cannot_decide():
    """cs_pose_default_params as it is (4 x 10 iterations, 0.01 rad / 0.05 m start): both sides run LM to its rounding floor, where the count of
    iterations and trials is decided by noise (module docstring); the inlier flags, the pose and chi2 are not."""
    batch = synth_pose.synth_pose_batch(64, (100, 500), 0.5, 0.1, 61)
    res = ref.optimize_batch(batch)
    for r in res:
        assert r["margin"] > 1e-6
    got = capi.pose_optimize_batch(batch)
    ptr = batch["obs_ptr"]
    for f, r in enumerate(res):
        assert np.array_equal(got["inlier"][ptr[f]:ptr[f + 1]].astype(bool), r["inlier"]), f
        assert np.abs(got["Tcw"][f] - r["pose"]).max() < 1e-5 * np.abs(r["pose"]).max(), f
        assert np.allclose(got["chi2"][f], r["chi2"], rtol=1e-5), f


# ---------------------------------------------------------------- batches that tell their fields apart (tests/pose_cases.py)
def _run_case(name):
    kw = pc.params_of(name)
    got = capi.pose_optimize_batch(pc.batch_of(name), capi.pose_default_params(**kw))
    _compare(got, pc.run(name), pc.batch_of(name), name)
    return got


@pytest.mark.parametrize("skew", [0.0, pc.SKEW], ids=["symmetric", "skewed"])
@pytest.mark.parametrize("robust", [True, False], ids=["robust", "plain"])
@pytest.mark.parametrize("kind", list(pc.SHARES))
def test_system_blocks(kind, robust, skew):
    """cs_pose_linearize_batch -- pose_kernels.hip's frame_linearize, the routine every LM iteration starts with -- against the
    reference's linearize on the boundary batch: 16 frames of 1 .. 256 observations around the lane stride, each with its own camera
    (fx != fy) and every observation with its own dense information; `skewed` adds an antisymmetric part to it, which is what tells a
    transposed read of Omega from a straight one.  Per frame, H against its largest entry, b and chi2 likewise.  Tolerance: 100 x the
    reference's own float64-against-long-double deviation on the same frames, floor 1e-13 -- sums of products with no libm call but
    sqrt; the margin is for the order of summation (64 lane shares and a butterfly against einsum), not for another function.
    Over the twelve cases, the largest deviation of any frame:
      reference's own (float64 against long double):  H 9.2e-16 .. 3.5e-15,  b 1.5e-15 .. 3.6e-15,  chi2 4.7e-16 .. 2.3e-15
      measured on an MI355X against the float64 one:   H 8.9e-16 .. 3.7e-15,  b 1.8e-15 .. 4.9e-15,  chi2 5.0e-16 .. 2.6e-15
    so the tolerances come out at 1e-13 .. 3.6e-13 and the device sits a factor of 50 and more inside them."""
    b = pc.boundary_batch(kind, skew)
    r64, rld = pc.blocks(kind, robust, False, skew), pc.blocks(kind, robust, True, skew)
    got = capi.pose_linearize_batch(b, robust)
    failures = []
    for nm, g, a, l in zip(("H", "b", "chi2"), got, r64, rld):
        assert np.isfinite(g).all()
        ref_dev, dev = pc.block_deviation(a, l).max(), pc.block_deviation(g, a).max()
        tol = max(100 * ref_dev, 1e-13)
        print("%s %s robust=%s skew=%s: device %.3g, reference's own %.3g, tolerance %.3g" % (nm, kind, robust, skew, dev, ref_dev, tol))
        if not dev <= tol:
            failures.append((nm, dev, tol))
    assert not failures, failures


def test_system_blocks_ignore_what_a_mono_edge_does_not_have():
    """A mono observation's information is the upper-left 2 x 2: whatever the caller left in the third row and column changes no bit."""
    for kind in ("mono", "mixed"):
        b = pc.boundary_batch(kind)
        clean = pc.without_mono_garbage(b)
        assert not np.array_equal(b["info"], clean["info"])
        for x, y in zip(capi.pose_linearize_batch(b), capi.pose_linearize_batch(clean)):
            assert np.array_equal(x, y), kind
    p = capi.pose_default_params(**pc.SCHEDULE)
    b = pc.boundary_batch("mixed")
    x, y = capi.pose_optimize_batch(b, p), capi.pose_optimize_batch(pc.without_mono_garbage(b), p)
    for k in ("Tcw", "inlier", "chi2", "iterations"):
        assert np.array_equal(x[k], y[k]), k


def test_system_blocks_are_the_same_bits_at_any_position():
    b = pc.boundary_batch("mixed")
    H, g, chi = capi.pose_linearize_batch(b)
    perm = np.random.default_rng(5).permutation(len(pc.COUNTS))
    Hp, gp, chip = capi.pose_linearize_batch(synth_pose.take_frames(b, perm))
    assert np.array_equal(Hp, H[perm]) and np.array_equal(gp, g[perm]) and np.array_equal(chip, chi[perm])
    for f in (0, 7, 15):
        H1, g1, chi1 = capi.pose_linearize_batch(synth_pose.take_frames(b, [f]))
        assert np.array_equal(H1[0], H[f]) and np.array_equal(g1[0], g[f]) and chi1[0] == chi[f]
    # the kernel's flag and widths arrive: without the kernel, or with a narrow one, other numbers
    assert np.all(capi.pose_linearize_batch(b, False)[2] != chi) and np.all(capi.pose_linearize_batch(b, True, 1.0, 1.0)[2] != chi)
    # a frame without observations: zeros
    empty = synth_pose.synth_pose_batch(3, [4, 0, 4], 0.5, 0.0, 1, pose_sigma=START)
    H0, g0, chi0 = capi.pose_linearize_batch(empty)
    assert not H0[1].any() and not g0[1].any() and chi0[1] == 0 and H0[0].any() and H0[2].any()


@pytest.mark.parametrize("kind", list(pc.SHARES))
def test_boundary_counts_with_dense_information_and_distinct_intrinsics(kind):
    """Schedule 4 x 3 from the 0.1 rad / 0.5 m start; the one- and two-observation frames, where 63 or 62 lanes add zeros to every sum,
    are compared like the rest: the reference meets the conditions for them.  Measured on an MI355X: poses within 6.8e-13, chi2 within
    1.1e-7 (a one-observation frame's chi2 of 1e-9; the reference's own two precisions differ by 8e-8 there), 8.2e-11 and 3.8e-13."""
    got = _run_case("boundary_" + kind)
    assert np.all(got["iterations"] == 3)


def test_trials_rejected_because_the_linearisation_does_not_hold():
    """24 frames started 0.5 rad / 2 m off; in two of them the reference rejects trials of a solved system (up to five in one iteration)."""
    _run_case("nonlinear")


def test_failed_factorisations():
    """24 frames with the information of 1.2 % of the observations sign-flipped: 14 of them run trials whose LDL^T meets a negative pivot --
    between one and six in an iteration, then an accepted one -- and 10 run none.  The seed is one at which the reference's two precisions
    agree to 2.5e-13 on every round's chi2 (tests/test_pose_only_ref.py says what other seeds can do)."""
    got = _run_case("not_pd")
    assert np.isfinite(got["Tcw"]).all() and np.isfinite(got["chi2"]).all()


@pytest.mark.parametrize("name", ["zero_round", "zero_round_continued"])
def test_a_round_of_no_iterations(name):
    """iterations[1] = 0 between two rounds that run: dense_lm_round's `chi = P.chi2(S)` path.  It reports 0 iterations and the active
    robust chi2 of the pose it was handed (the start pose under restart_each_round, round one's otherwise), and is classified after."""
    got = _run_case(name)
    assert np.all(got["iterations"][:, 1] == 0) and np.all(got["chi2"][:, 1] > 0) and np.any(got["iterations"][:, 2] > 0)


def test_a_frame_that_loses_every_observation_gets_them_back_after_a_restart():
    got = _run_case("no_inliers")
    assert np.all(got["iterations"][:, 1] == 0) and np.all(got["chi2"][:, 1] == 0)
    assert got["iterations"][:, 2].tolist() == [1, 1, 1, 0, 0]
    ptr = pc.batch_of("no_inliers")["obs_ptr"]
    assert all(got["inlier"][ptr[f]:ptr[f + 1]].sum() >= 6 for f in range(3)) and not got["inlier"][ptr[3]:].any()


def test_input_quaternions_of_norm_three_and_negative_w():
    got = _run_case("quaternion")
    b = pc.batch_of("quaternion")
    empty = int(np.where(np.diff(b["obs_ptr"]) == 0)[0][0])
    assert np.array_equal(got["Tcw"][empty], ref.se3_from_vector(b["Tcw"][empty])) and got["Tcw"][empty][6] > 0
    # the same frames with the unit quaternions they stand for: the rounding of the normalisation apart, the same results
    unit = {k: np.array(v, copy=True) for k, v in b.items()}
    unit["Tcw"][:, 3:] /= -3.0
    same = capi.pose_optimize_batch(unit, capi.pose_default_params(**pc.SCHEDULE))
    assert np.array_equal(same["iterations"], got["iterations"]) and np.array_equal(same["inlier"], got["inlier"])
    assert np.allclose(same["Tcw"], got["Tcw"], rtol=0, atol=1e-9)


def test_a_point_on_the_camera_plane_stays_its_own_frames_affair():
    """A frame with identity rotation, zero translation and the map point (1, 1, 0) among its observations: every input finite, the
    point's depth 0, its projection infinite, H, b and chi2 not numbers.  Every factorisation then fails, every trial is rejected, and
    no loop of cs_dense_lm.h is unbounded: the call returns, the frame reports iteration counts within the schedule, and the three
    frames that share its workgroup, and the two of the next one, come out bit for bit as without it."""
    b = pc.boundary_batch("mixed")
    six = synth_pose.take_frames(b, [6, 3, 9, 12, 7, 15])
    ptr = six["obs_ptr"]
    s = slice(ptr[1], ptr[2])
    assert ptr[2] - ptr[1] == 4
    six["Tcw"][1] = [0, 0, 0, 0, 0, 0, 1]
    six["Xw"][s] = [[1.0, 1.0, 0.0], [0.5, -0.2, 9.0], [-1.0, 0.4, 15.0], [2.0, 1.0, 30.0]]
    assert np.isfinite(six["Xw"]).all() and np.isfinite(six["meas"]).all() and np.isfinite(six["info"]).all()
    p = capi.pose_default_params(**pc.SCHEDULE)
    got = capi.pose_optimize_batch(six, p)
    others = [0, 2, 3, 4, 5]
    base = capi.pose_optimize_batch(synth_pose.take_frames(six, others), p)
    assert np.all(got["iterations"][1] >= 0) and np.all(got["iterations"][1] <= 3)
    ptr_b = np.concatenate([[0], np.cumsum(np.diff(ptr)[others])])
    for k, f in enumerate(others):
        assert np.array_equal(got["Tcw"][f], base["Tcw"][k]) and np.array_equal(got["chi2"][f], base["chi2"][k]) and np.array_equal(got["iterations"][f], base["iterations"][k])
        assert np.array_equal(got["inlier"][ptr[f]:ptr[f + 1]], base["inlier"][ptr_b[k]:ptr_b[k + 1]])
        assert np.isfinite(got["Tcw"][f]).all()
    H, g, chi = capi.pose_linearize_batch(six)
    assert not np.isfinite(chi[1]) and np.isfinite(np.delete(chi, 1)).all() and np.isfinite(np.delete(H, 1, 0)).all()
