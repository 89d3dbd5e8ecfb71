"""tests/pose_only_ref.py (the numpy statement the GPU test of cs_pose_optimize_batch leans on) against the CPU oracle, mono frames.

A frame is the oracle's Problem with one free camera and every point fixed: EdgeSE3ProjectXYZ's camera block is EdgeSE3ProjectXYZOnlyPose's
Jacobian, the 6 x 6 pose system has no landmarks to eliminate, and the oracle's LM driver is the same restatement of
optimization_algorithm_levenberg.cpp.  The rounds are rebuilt here per inlier subset, the classification goes through compute_errors().
Required: the same LM trials per iteration, chi2 and pose within 1e-5 relative (the project's standing contract), identical inlier flags.
The condition on the inputs (no chi2 within 1e-6 relative of its threshold, no rho within 1e-6 of 0) is asserted on the reference; the
schedule of 3 iterations per round from a 0.1 rad / 0.5 m start is what keeps LM off its rounding floor (tests/test_pose_only_gpu.py).
"""
import numpy as np
import pytest

from cube_slam_wu_amd import synth_pose
from oracle import ba_oracle_py
import pose_cases as pc
import pose_only_ref as ref

PARAMS = dict(iterations=[3, 3, 3, 3])


def _oracle_rounds(T0, intr, Xw, meas, info9, p):
    n = len(Xw)
    info4 = info9[:, [0, 1, 3, 4]]
    intr4 = np.tile(intr[:4], (n, 1))
    level0 = np.ones(n, bool)
    T = T0
    out = dict(trials=[], chi2=[], iterations=[])
    for r in range(p["n_rounds"]):
        if p["restart_each_round"]:
            T = T0
        a = np.where(level0)[0]
        if len(a):
            P = ba_oracle_py.Problem(T[None], [0], points=Xw[a], pt_fixed=np.ones(len(a)))
            hub = np.full(len(a), p["huber_mono"] if r < p["robust_rounds"] else 0.0)
            P.set_edges_proj(np.arange(len(a)), np.zeros(len(a)), meas[a, :2], info4[a], intr4[a], hub)
            done = P.optimize(p["iterations"][r])
            chi, _, tr = P.history()
            T = P.state()[0][0].copy()
            P.close()
            out["trials"].append(list(tr[:done])); out["chi2"].append(chi[done - 1]); out["iterations"].append(done)
        else:
            out["trials"].append([]); out["chi2"].append(0.0); out["iterations"].append(0)
        P = ba_oracle_py.Problem(T[None], [0], points=Xw, pt_fixed=np.ones(n))
        P.set_edges_proj(np.arange(n), np.zeros(n), meas[:, :2], info4, intr4, None)
        _, ep, _, _ = P.compute_errors()
        P.close()
        each = np.einsum("ni,nij,nj->n", ep, info4.reshape(-1, 2, 2), ep)
        level0 = ~(each > p["chi2_mono"])
    out["pose"], out["inlier"] = T, level0
    return out


def test_reference_equals_the_oracle_on_mono_frames():
    batch = synth_pose.synth_pose_batch(24, (50, 400), 0.0, 0.1, 71, pose_sigma=(0.1, 0.5))
    p = dict(ref.DEFAULTS, **PARAMS)
    ptr = batch["obs_ptr"]
    res = ref.optimize_batch(batch, PARAMS)
    n_outliers_found = 0
    for f, r in enumerate(res):
        assert r["margin"] > 1e-6 and np.abs(r["rho"]).min() > 1e-6, (f, r["margin"], np.abs(r["rho"]).min())
        s = slice(ptr[f], ptr[f + 1])
        o = _oracle_rounds(batch["Tcw"][f], batch["intr"][f], batch["Xw"][s], batch["meas"][s], batch["info"][s], p)
        assert [list(t) for t in r["trials"]] == [list(t) for t in o["trials"]], (f, r["trials"], o["trials"])
        assert np.array_equal(r["iterations"], o["iterations"])
        assert np.allclose(r["chi2"], o["chi2"], rtol=1e-5), (f, r["chi2"], o["chi2"])
        assert np.abs(r["pose"] - o["pose"]).max() < 1e-5 * np.abs(o["pose"]).max(), (f, r["pose"], o["pose"])
        assert np.array_equal(r["inlier"], o["inlier"]), f
        n_outliers_found += int((~r["inlier"]).sum())
        # the optimisation did its job: the pose ends closer to the truth than it started
        assert np.abs(r["pose"] - batch["Tcw_true"][f]).max() < np.abs(batch["Tcw"][f] - batch["Tcw_true"][f]).max()
    assert n_outliers_found > 0


def test_reference_building_blocks():
    rng = np.random.default_rng(3)
    # Huber: identity under delta^2 (as a float), 2 sqrt(e) delta - delta^2 above it
    d = np.sqrt(5.991)
    dsqr = float(np.float32(d * d))
    rho, w = ref.huber(np.array([1.0, dsqr, 100.0]), d)
    assert rho[0] == 1.0 and w[0] == 1.0 and rho[1] == dsqr and w[1] == 1.0
    assert rho[2] == 2 * 10.0 * d - dsqr and w[2] == d / 10.0
    # exp of a small and a large update is a rigid motion; oplus composes on the left
    for u in (rng.normal(0, 1e-7, 6), rng.normal(0, 0.5, 6)):
        T = ref.se3_exp(u)
        assert abs(np.linalg.norm(T[3:]) - 1) < 1e-15 and T[6] >= 0
    # the analytic Jacobian is the derivative of the error under the left-multiplied update
    T = ref.se3_exp(rng.normal(0, 0.3, 6))
    X = np.array([[0.5, -0.2, 9.0], [-1.0, 0.4, 15.0]]) - T[:3]
    intr = synth_pose.KITTI_INTR5
    for stereo in (np.array([False, False]), np.array([True, True])):
        meas = np.zeros((2, 3))
        e0, pc = ref.errors(T, intr, X, meas, stereo)
        J = ref.jacobians(pc, intr, stereo)
        for k in range(6):
            du = np.zeros(6); du[k] = 1e-3
            ep, _ = ref.errors(ref.se3_mul(ref.se3_exp(du), T), intr, X, meas, stereo)
            em, _ = ref.errors(ref.se3_mul(ref.se3_exp(-du), T), intr, X, meas, stereo)
            assert np.allclose((ep - em) / 2e-3, J[:, :, k], rtol=1e-3, atol=0.1)      # (entries are 10 .. 1000; the stereo error's float 1 / z rules out a finer step)
    # LDL^T: solves an SPD system, refuses an indefinite one
    A = rng.normal(size=(6, 6)); A = A @ A.T + np.eye(6)
    b = rng.normal(size=6)
    assert np.allclose(ref.ldlt_solve(A, b), np.linalg.solve(A, b))
    A[2, 2] = -1.0
    assert ref.ldlt_solve(A, b) is None


# ---------------------------------------------------------------- the batches that tell their fields apart (tests/pose_cases.py)
def test_builders_take_the_generators_symmetries_away():
    plain = synth_pose.synth_pose_batch(6, [1, 5, 64, 65, 0, 130], 0.5, 0.1, 7, pose_sigma=pc.START)
    kept = {k: v.copy() for k, v in plain.items()}
    b = pc.told_apart(plain, 7)
    for k, v in kept.items():
        assert np.array_equal(plain[k], v), k                      # the builders copy
    assert np.all(plain["intr"] == synth_pose.KITTI_INTR5)        # what they start from: one row, fx == fy
    intr = b["intr"]
    assert np.all(np.abs(intr[:, 1] / intr[:, 0] - 1) >= 0.02) and np.all(np.abs(intr[:, 2:4] - plain["intr"][:, 2:4]) > 0) and np.all(intr[:, 4] != plain["intr"][:, 4])
    assert all(len(np.unique(intr[:, k])) == len(intr) for k in range(5))
    st = b["is_stereo"].astype(bool)
    assert st.any() and (~st).any()
    W = b["info"].reshape(-1, 3, 3)
    w = plain["info"][:, 0]
    ev = np.linalg.eigvalsh(W[st])
    assert np.array_equal(W[st], np.swapaxes(W[st], 1, 2)) and ev.min() > 0
    assert np.all(ev[:, 2] / ev[:, 0] <= 5 * (1 + 1e-12)) and (ev[:, 2] / ev[:, 0]).max() > 2.5
    assert np.all(ev[:, 0] >= w[st] / np.sqrt(5) * (1 - 1e-12)) and np.all(ev[:, 2] <= w[st] * np.sqrt(5) * (1 + 1e-12))
    assert np.all(np.abs(W[st][:, [0, 0, 1], [1, 2, 2]]) > 0)
    ev2 = np.linalg.eigvalsh(W[~st][:, :2, :2])
    assert ev2.min() > 0 and np.all(W[~st][:, 0, 1] == W[~st][:, 1, 0]) and np.all(W[~st][:, 0, 1] != 0)
    assert np.all(W[~st][:, 2, :] != 0) and np.all(W[~st][:, :, 2] != 0)       # the garbage
    # the reference ignores the garbage, and the measurements moved with the cameras: at the true pose the inliers' errors are the noise
    assert np.array_equal(ref.omega3(b["info"], st), ref.omega3(pc.without_mono_garbage(b)["info"], st))
    ptr = b["obs_ptr"]
    for f in range(len(intr)):
        s = slice(ptr[f], ptr[f + 1])
        e0, _ = ref.errors(ref.se3_from_vector(plain["Tcw_true"][f]), plain["intr"][f], plain["Xw"][s], plain["meas"][s], st[s])
        e1, _ = ref.errors(ref.se3_from_vector(b["Tcw_true"][f]), intr[f], b["Xw"][s], b["meas"][s], st[s])
        assert np.allclose(e0, e1, rtol=0, atol=1e-4)              # (the stereo edge's float 1 / z: 1e-7 of a few hundred pixels)
    # an antisymmetric part on request, and only then
    sk = pc.told_apart(plain, 7, skew=0.2)["info"].reshape(-1, 3, 3)
    off = ([0, 0, 1], [1, 2, 2])
    assert np.all(sk[st][:, off[0], off[1]] != sk[st][:, off[1], off[0]]) and np.all(sk[:, 0, 1] != sk[:, 1, 0])
    assert np.allclose(0.5 * (sk[st] + np.swapaxes(sk[st], 1, 2)), W[st], rtol=0, atol=1e-15)


def test_ldlt_logs_every_pivot_relative_to_the_largest_diagonal_entry():
    A = np.diag([4.0, 2.0, 1.0, 8.0, 0.5, 2.0])
    b = np.ones(6)
    piv = []
    assert np.allclose(ref.ldlt_solve(A, b, piv), 1 / np.diag(A)) and piv == [0.5, 0.25, 0.125, 1.0, 0.0625, 0.25]
    A[2, 2] = -1.0
    piv = []
    assert ref.ldlt_solve(A, b, piv) is None and piv == [0.5, 0.25, -0.125]      # the failing pivot is the last one logged


@pytest.mark.parametrize("kind", list(pc.SHARES))
@pytest.mark.parametrize("robust", [True, False], ids=["robust", "plain"])
def test_system_blocks_in_long_double_are_the_float64_ones_to_rounding(kind, robust):
    """The reference's own error on H, b and chi2 of the boundary batch: float64 against long double, per frame against the block's
    largest entry.  It is what the device's tolerance is a multiple of (tests/test_pose_only_gpu.py), so it has to be rounding and
    nothing else: under 1e-13 (measured: 1.3e-15 at the most; 53 bits give 1.1e-16 per operation)."""
    for skew in (0.0, pc.SKEW):
        r64, rld = pc.blocks(kind, robust, False, skew), pc.blocks(kind, robust, True, skew)
        assert rld[0].dtype == np.longdouble
        dev = [pc.block_deviation(a, b).max() for a, b in zip(r64, rld)]
        print("%s robust=%s skew=%s: H %.3g  b %.3g  chi2 %.3g" % ((kind, robust, skew) + tuple(dev)))
        assert max(dev) < 1e-13
    # the kernel's flag and the garbage reach the numbers
    H, _, chi = pc.blocks(kind, robust)
    Ho, _, chio = pc.blocks(kind, not robust)
    assert np.all(H != Ho) and np.all(chi != chio)


# Frames with fewer than three observations: H has rank 2 per mono and 3 per stereo observation, under 6, and the pivots of its null
# space ARE lambda.  lambda starts at 1e-5 of the largest diagonal entry and falls to a ninth of that in a round's three accepted steps,
# while under the Huber kernel the entry itself grows 40-fold as the residuals come in from a 0.1 rad start: 2.1e-8 is measured, and no
# seed can bring it over 1e-6 (none of 7 .. 199 does).  Nothing is decided there by rounding: H is a sum of positive semi-definite terms,
# so such a pivot is lambda plus something non-negative, against a rounding error of the factorisation of 6 * 2^-53 = 7e-16 of the
# largest entry.  For these frames the bound is 1e-12: a thousand times that error.
PIVOT_MARGIN, PIVOT_MARGIN_RANK_DEFICIENT = 1e-6, 1e-12


@pytest.mark.parametrize("name", list(pc.CASES))
def test_reference_meets_the_conditions_on_every_frame(name):
    res, counts = pc.run(name), np.diff(pc.batch_of(name)["obs_ptr"])
    cond = np.array(pc.conditions(res))
    print(name, "min |rho| %.3g, margin %.3g, pivot margin %.3g (frames of three observations and more: %.3g)" % (tuple(cond.min(0)) + (cond[counts >= 3, 2].min(),)))
    for f, (rho, margin, pivot) in enumerate(cond):
        assert rho > 1e-6 and margin > 1e-6, (name, f, rho, margin)
        assert pivot > (PIVOT_MARGIN if counts[f] >= 3 else PIVOT_MARGIN_RANK_DEFICIENT), (name, f, counts[f], pivot)
    for r in res:
        assert np.all(r["iterations"] <= pc.params_of(name)["iterations"])


@pytest.mark.parametrize("name", list(pc.CASES))
def test_reference_takes_the_same_decisions_in_long_double(name):
    """A fourth condition, which the three above do not imply: with its edges evaluated in long double the reference runs the same
    trials, classifies alike and ends within 1e-6 of its float64 self, on every frame.  Flipped information makes some frames' objective
    unbounded below -- LM then runs off to a chi2 of -1e8 and further -- and a frame whose result that leaves to rounding (met while
    choosing the seed: 1.0e-5 between the two precisions on one round's chi2) cannot be held to 1e-5 against anything."""
    sp = pc.spread(pc.run(name), pc.run(name, True))
    print(name, "pose %.3g, chi2 %.3g" % (max(s[1] for s in sp), max(s[2] for s in sp)))
    for f, (same, pose, chi) in enumerate(sp):
        assert same and pose < 1e-6 and chi < 1e-6, (name, f, same, pose, chi)


def test_boundary_batches_hold_every_count_and_class():
    for kind, share in pc.SHARES.items():
        b = pc.boundary_batch(kind)
        assert tuple(np.diff(b["obs_ptr"])) == pc.COUNTS and b["is_stereo"].mean() == pytest.approx(share, abs=0.05)
        assert all((r["iterations"] == 3).all() for r in pc.run("boundary_" + kind))      # the one- and two-observation frames included


def test_nonlinear_batch_rejects_trials_with_a_solved_system():
    res = pc.run("nonlinear")
    rejected = [f for f, r in enumerate(res) if any(q > 1 for t in r["trials"] for q in t)]
    assert len(res) == 24 and len(rejected) >= 2, rejected
    assert all(r["not_pd_trials"] == 0 for r in res)


def test_flipped_information_fails_factorisations_in_some_frames_and_not_in_others():
    res = pc.run("not_pd")
    failed = np.array([r["not_pd_trials"] for r in res])
    print("not positive definite trials per frame:", failed.tolist())
    assert 2 * (failed > 0).sum() >= len(res) and (failed == 0).sum() >= 4
    assert all(r["pivot_margin"] > PIVOT_MARGIN for r in res)
    # a failed trial's rho is -inf; an iteration that fails has its accepted trial behind the failed ones
    per_iteration = sorted(set(q for r in res if r["not_pd_trials"] for t in r["trials"] for q in t))
    assert per_iteration[0] == 1 and per_iteration[-1] >= 7 and len(per_iteration) >= 5, per_iteration
    assert min(failed[failed > 0]) <= 8      # a frame that fails once or twice per round, not six times
    assert all(np.isneginf(r["rho"]).sum() == r["not_pd_trials"] for r in res)


def test_schedule_corners_in_the_reference():
    for name in ("zero_round", "zero_round_continued"):
        res = pc.run(name)
        first = pc.params_of(name)["iterations"][0]
        assert all(r["iterations"][0] == first and r["iterations"][1] == 0 and r["chi2"][1] > 0 for r in res)
        assert any(r["iterations"][2] > 0 for r in res)
    assert all(r["iterations"][2] == 2 for r in pc.run("zero_round_continued"))
    res, b = pc.run("no_inliers"), pc.batch_of("no_inliers")
    ptr = b["obs_ptr"]
    for f, r in enumerate(res):
        assert r["iterations"][0] == 3 and r["iterations"][1] == 0 and r["chi2"][1] == 0      # round two: nothing at level 0
        if f < 3:      # brought back by round two's classification at the start pose: exactly the frame's clean observations
            assert r["iterations"][2] == 1 and r["chi2"][2] > 0
            assert np.array_equal(r["inlier"], ~b["is_outlier"][ptr[f]:ptr[f + 1]]) and r["inlier"].sum() >= 6
        else:
            assert r["iterations"][2] == 0 and not r["inlier"].any()
    b = pc.batch_of("quaternion")
    assert np.allclose(np.linalg.norm(b["Tcw"][:, 3:], axis=1), 3.0) and np.all(b["Tcw"][:, 6] < 0) and 0 in np.diff(b["obs_ptr"])
    for f, r in enumerate(pc.run("quaternion")):
        assert abs(np.linalg.norm(r["pose"][3:]) - 1) < 1e-15 and r["pose"][6] > 0
