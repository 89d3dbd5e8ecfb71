"""tests/pose_only_ref.py (the numpy statement the GPU test of cs_pose_optimize_batch leans on) against the CPU oracle, mono frames.

A frame is the oracle's Problem with one free camera and every point fixed: EdgeSE3ProjectXYZ's camera block is EdgeSE3ProjectXYZOnlyPose's
Jacobian, the 6 x 6 pose system has no landmarks to eliminate, and the oracle's LM driver is the same restatement of
optimization_algorithm_levenberg.cpp.  The rounds are rebuilt here per inlier subset, the classification goes through compute_errors().
Required: the same LM trials per iteration, chi2 and pose within 1e-5 relative (the project's standing contract), identical inlier flags.
The condition on the inputs (no chi2 within 1e-6 relative of its threshold, no rho within 1e-6 of 0) is asserted on the reference; the
schedule of 3 iterations per round from a 0.1 rad / 0.5 m start is what keeps LM off its rounding floor (tests/test_pose_only_gpu.py).
"""
import numpy as np

from cube_slam_wu_amd import synth_pose
from oracle import ba_oracle_py
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
