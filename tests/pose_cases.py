"""Pose batches that tell their fields apart, and the cases tests/test_pose_only_gpu.py runs on them with their reference results
(tests/pose_only_ref.py), built once per process.  tests/test_pose_only_ref.py asserts, without a GPU, the conditions under which the
float64 reference may be compared at all -- for every frame of every case here, none dropped: the seeds below are ones for which the
reference alone meets them.

cube_slam_wu_amd/synth_pose.py gives every frame the same intrinsics with fx == fy and every observation a scalar times the identity as
its information: a kernel that reads frame 0's intrinsics for every frame, fx where fy belongs, a transposed or permuted information
matrix, or that drops an off-diagonal entry computes the same numbers on such a batch.  with_distinct_intrinsics and
with_dense_information take those symmetries away; the generator's defaults (the benchmark's workload) are not touched."""
import functools

import numpy as np

from cube_slam_wu_amd import synth_pose
import pose_only_ref as ref

COUNTS = (1, 2, 3, 4, 5, 6, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256)      # lane l owns observations l, l + 64, ...
SCHEDULE = dict(iterations=[3, 3, 3, 3])      # the schedule at which trial counts can be compared (tests/test_pose_only_gpu.py)
START = (0.1, 0.5)
SHARES = {"mono": 0.0, "mixed": 0.5, "stereo": 1.0}
SKEW = 0.2      # the antisymmetric part of the information that is not symmetric, relative to the observation's level weight


def _copy(batch):
    return {k: np.array(v, copy=True) for k, v in batch.items()}


def _project(T, intr, Xw):
    fx, fy, cx, cy, bf = intr
    pc = Xw @ ref._rot(T[3:]).T + T[:3]
    u = pc[:, 0] / pc[:, 2] * fx + cx
    return np.stack([u, pc[:, 1] / pc[:, 2] * fy + cy, u - bf / pc[:, 2]], 1)


def with_distinct_intrinsics(batch, seed):
    """Every frame its own camera: fx within 5 % of the generator's, fy 2 .. 6 % off fx to either side, cx and cy moved by up to 8 and 5
    pixels, bf scaled by 0.9 .. 1.1.  Every measurement is moved by what the new camera changes in the projection at the true pose, so
    its noise and the outliers stay what they were."""
    rng = np.random.default_rng(seed)
    out = _copy(batch)
    n = len(batch["Tcw"])
    fx = batch["intr"][:, 0] * rng.uniform(0.95, 1.05, n)
    fy = fx * (1 + rng.choice([-1.0, 1.0], n) * rng.uniform(0.02, 0.06, n))
    out["intr"] = np.stack([fx, fy, batch["intr"][:, 2] + rng.uniform(-8, 8, n), batch["intr"][:, 3] + rng.uniform(-5, 5, n),
                            batch["intr"][:, 4] * rng.uniform(0.9, 1.1, n)], 1)
    ptr = batch["obs_ptr"]
    for f in range(n):
        s = slice(ptr[f], ptr[f + 1])
        out["meas"][s] += _project(batch["Tcw_true"][f], out["intr"][f], batch["Xw"][s]) - _project(batch["Tcw_true"][f], batch["intr"][f], batch["Xw"][s])
    out["meas"][~batch["is_stereo"].astype(bool), 2] = 0.0
    assert np.all(np.abs(out["intr"][:, 1] / out["intr"][:, 0] - 1) >= 0.02)
    for k in range(5):
        assert len(np.unique(out["intr"][:, k])) == n
    return out


def _rotations(rng, n):
    """n random 3 x 3 rotations (QR of a normal matrix, the determinant made +1)."""
    Q = np.linalg.qr(rng.normal(size=(n, 3, 3)))[0]
    Q[:, :, 0] *= np.sign(np.linalg.det(Q))[:, None]
    return Q


def with_dense_information(batch, seed, skew=0.0):
    """Every observation its own dense information Q diag(d) Q^T, symmetric to the last bit and positive definite: Q a random rotation, d
    the observation's level weight times factors of 1 / sqrt(5) .. sqrt(5) (eigenvalue ratios up to 5).  A stereo row gets a 3 x 3; a mono
    row a dense 2 x 2 in the corner and NON-ZERO GARBAGE in the third row and column, which the edge does not have and every
    implementation must ignore.  skew > 0 adds an antisymmetric part of that relative size (to the stereo 3 x 3 and the mono 2 x 2):
    the ABI takes any row-major matrix and uses it as written, Omega e and J^T (Omega J), as g2o does -- only such a matrix tells a
    transposed read from a straight one."""
    rng = np.random.default_rng(seed)
    out = _copy(batch)
    N = len(batch["Xw"])
    if N == 0:
        return out
    w = batch["info"][:, 0]
    st = batch["is_stereo"].astype(bool)
    d = w[:, None] * np.exp(rng.uniform(-0.5 * np.log(5.0), 0.5 * np.log(5.0), (N, 3)))
    Q = _rotations(rng, N)
    W3 = np.einsum("nij,nj,nkj->nik", Q, d, Q)
    W3 = 0.5 * (W3 + np.swapaxes(W3, 1, 2))
    ang = rng.uniform(0, 2 * np.pi, N)
    c, s = np.cos(ang), np.sin(ang)
    W2 = np.zeros((N, 3, 3))
    W2[:, 0, 0] = c * c * d[:, 0] + s * s * d[:, 1]
    W2[:, 1, 1] = s * s * d[:, 0] + c * c * d[:, 1]
    W2[:, 0, 1] = W2[:, 1, 0] = c * s * (d[:, 0] - d[:, 1])
    garbage = w[:, None] * rng.uniform(0.5, 2.0, (N, 5)) * rng.choice([-1.0, 1.0], (N, 5))
    W2[:, 0, 2], W2[:, 1, 2], W2[:, 2, 0], W2[:, 2, 1], W2[:, 2, 2] = garbage.T
    if skew > 0:
        a = skew * w[:, None] * rng.uniform(0.5, 1.0, (N, 3)) * rng.choice([-1.0, 1.0], (N, 3))
        for k, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
            W3[:, i, j] += a[:, k]; W3[:, j, i] -= a[:, k]
        W2[:, 0, 1] += a[:, 0]; W2[:, 1, 0] -= a[:, 0]
    out["info"] = np.where(st[:, None, None], W3, W2).reshape(N, 9)
    return out


def without_mono_garbage(batch):
    """The same batch with the third row and column of every mono row's information zeroed."""
    out = _copy(batch)
    m = ~batch["is_stereo"].astype(bool)
    W = out["info"].reshape(-1, 3, 3)
    W[m, 2, :] = 0
    W[m, :, 2] = 0
    return out


def with_flipped_information(batch, share, seed):
    """-Omega on a random `share` of the observations: H = sum J^T (rho' Omega) J is then indefinite, and a trial's LDL^T meets a negative
    pivot until lambda has grown past it."""
    rng = np.random.default_rng(seed)
    out = _copy(batch)
    out["info"][rng.random(len(batch["Xw"])) < share] *= -1.0
    return out


def told_apart(batch, seed, skew=0.0):
    return with_dense_information(with_distinct_intrinsics(batch, seed + 100), seed + 200, skew)


# ---------------------------------------------------------------- the cases
BOUNDARY_SEED, NONLINEAR_SEED, NOT_PD_SEED, CORNER_SEED = 7, 23, 12, 3
NOT_PD_SHARE = 0.012


@functools.lru_cache(None)
def boundary_batch(kind, skew=0.0, seed=BOUNDARY_SEED):
    """16 frames, one per count of COUNTS, dense information and distinct intrinsics; kind = a key of SHARES."""
    return told_apart(synth_pose.synth_pose_batch(len(COUNTS), list(COUNTS), SHARES[kind], 0.1, seed, pose_sigma=START), seed, skew)


@functools.lru_cache(None)
def nonlinear_batch(seed=NONLINEAR_SEED):
    """24 frames started 0.5 rad / 2 m off: far enough for LM to reject trials because the linearisation does not hold."""
    return told_apart(synth_pose.synth_pose_batch(24, (50, 300), 0.5, 0.1, seed, pose_sigma=(0.5, 2.0)), seed)


@functools.lru_cache(None)
def not_pd_batch(seed=NOT_PD_SEED, share=NOT_PD_SHARE):
    """24 frames whose information is sign-flipped on a share of the observations."""
    return with_flipped_information(told_apart(synth_pose.synth_pose_batch(24, (50, 300), 0.5, 0.1, seed, pose_sigma=START), seed), share, seed + 300)


# A round of no iterations between two others: it reports 0 iterations and the active robust chi2 of the pose it was handed -- the start
# pose under restart_each_round, the first round's otherwise -- and is followed by a classification like any other.
ZERO_ROUND = dict(n_rounds=3, iterations=[3, 0, 3], robust_rounds=2)
ZERO_ROUND_CONTINUED = dict(n_rounds=3, iterations=[2, 0, 2], robust_rounds=1, restart_each_round=0)


@functools.lru_cache(None)
def zero_round_batch(seed=CORNER_SEED):
    return told_apart(synth_pose.synth_pose_batch(8, [5, 40, 64, 65, 100, 129, 200, 300], 0.5, 0.1, seed, pose_sigma=START), seed)


# A frame that loses every observation after round one and gets them back: it starts at the truth with 0.01 px of noise on its inliers
# and a quarter of gross outliers, and round one has no kernel, so the outliers drag the pose off and at the pose round one ends on
# every observation is over the tight threshold.  Round two then has no level-0 edge: 0 iterations, chi2 0, and under restart_each_round
# its classification is taken at the start pose, where the inliers are under the threshold again; round three optimises them.  Its one
# iteration is what has something to gain: after it LM sits on the minimum of a nearly exact quadratic (module docstring of
# tests/test_pose_only_gpu.py).  The two ordinary frames beside them start 0.1 rad off, are over the threshold at either pose and never
# come back.
NO_INLIERS = dict(n_rounds=3, iterations=[3, 3, 1], robust_rounds=0, chi2_mono=0.05, chi2_stereo=0.05)


@functools.lru_cache(None)
def no_inliers_batch(seed=CORNER_SEED):
    lost = synth_pose.synth_pose_batch(3, [12, 64, 130], 0.0, 0.25, seed + 1, pose_sigma=(0.0, 0.0), pixel_sigma=0.01)
    plain = synth_pose.synth_pose_batch(2, [40, 100], 0.5, 0.1, seed + 2, pose_sigma=START)
    return told_apart(synth_pose.concat_batches([lost, plain]), seed)


@functools.lru_cache(None)
def quaternion_batch(seed=CORNER_SEED):
    """Input quaternions of norm 3 with a negative w, a frame without observations among them."""
    b = told_apart(synth_pose.synth_pose_batch(6, [30, 0, 64, 65, 129, 200], 0.5, 0.1, seed + 3, pose_sigma=START), seed)
    b["Tcw"][:, 3:] *= -3.0
    assert np.all(b["Tcw"][:, 6] < 0)
    return b


CASES = {
    "boundary_mono": (lambda: boundary_batch("mono"), SCHEDULE),
    "boundary_mixed": (lambda: boundary_batch("mixed"), SCHEDULE),
    "boundary_stereo": (lambda: boundary_batch("stereo"), SCHEDULE),
    "nonlinear": (nonlinear_batch, SCHEDULE),
    "not_pd": (not_pd_batch, SCHEDULE),
    "zero_round": (zero_round_batch, ZERO_ROUND),
    "zero_round_continued": (zero_round_batch, ZERO_ROUND_CONTINUED),
    "no_inliers": (no_inliers_batch, NO_INLIERS),
    "quaternion": (quaternion_batch, SCHEDULE),
}


def batch_of(name):
    return CASES[name][0]()


def params_of(name):
    return dict(CASES[name][1])


@functools.lru_cache(None)
def run(name, long_double=False):
    """The reference's results of a case, one dict per frame; long_double: with the edges evaluated in long double."""
    return ref.optimize_batch(batch_of(name), params_of(name), np.longdouble if long_double else np.float64)


def spread(r64, rld):
    """Per frame, what the two precisions make of it: (same trials, iterations and inlier flags; pose deviation against the largest of its
    seven numbers; chi2 deviation against the largest of the rounds')."""
    out = []
    for a, b in zip(r64, rld):
        same = a["trials"] == b["trials"] and np.array_equal(a["iterations"], b["iterations"]) and np.array_equal(a["inlier"], b["inlier"])
        top = np.abs(a["chi2"]).max()
        out.append((same, np.abs(a["pose"] - b["pose"]).max() / np.abs(a["pose"]).max(), np.abs(a["chi2"] - b["chi2"]).max() / top if top > 0 else 0.0))
    return out


def conditions(res):
    """Per frame (min |rho|, classification margin, pivot margin) of reference results."""
    return [(np.abs(r["rho"]).min() if len(r["rho"]) else np.inf, r["margin"], r["pivot_margin"]) for r in res]


@functools.lru_cache(None)
def blocks(kind, robust, long_double=False, skew=0.0):
    """(H (16, 21), b (16, 6), chi2 (16)) of boundary_batch(kind, skew) at its start poses."""
    return ref.linearize_batch(boundary_batch(kind, skew), robust, None, np.longdouble if long_double else np.float64)


def block_deviation(a, b):
    """Per frame: the largest difference against the largest entry of b's block (a frame without a non-zero entry: 0 when a has none either)."""
    a, b = np.asarray(a, np.longdouble), np.asarray(b, np.longdouble)
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    top = np.abs(b).max(-1)
    return (np.abs(a - b).max(-1) / np.where(top > 0, top, 1)).astype(np.float64)
