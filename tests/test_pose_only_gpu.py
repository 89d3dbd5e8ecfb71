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

A frame whose first trial is not positive definite: H = sum J^T (rho' Omega) J is positive semi-definite and lambda > 0, so the
generator cannot produce one short of a NaN; the failed-trial branch is the same code as cs_ba_optimize's and stays untested here.
"""
import numpy as np
import pytest

from cube_slam_wu_amd import capi, synth_pose
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
