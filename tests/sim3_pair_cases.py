"""The batches tests/test_sim3_pair_gpu.py runs and their reference results (tests/sim3_pair_ref.py), built once per process.
tests/test_sim3_pair_ref.py asserts, without a GPU, the conditions under which a float64 reference may be compared at all -- for every
pair of every batch here, none dropped: the seeds below are ones for which the reference alone meets them.

cube_slam_wu_amd/synth_sim3_pairs.py gives every pair the same two cameras, each with fx == fy, and every edge a scalar times the identity
as its information: reading pair 0's intrinsics for every pair, fx for fy, camera 1 for camera 2, or dropping an off-diagonal entry of
Omega changes little or nothing there.  with_distinct_intrinsics and with_dense_information take those symmetries away (dense_batch,
dense_edge_batch); the generator's defaults are not touched."""
import functools

import numpy as np

from cube_slam_wu_amd import synth_sim3_pairs as sp
import sim3_pair_ref as ref

COUNTS = (12, 20, 63, 64, 65, 100, 128, 129, 300)      # the lane-stride boundaries of a 64-lane wave
START = (0.05, 0.1, 0.05)
SHORT = dict(iterations_first=3, iterations_more_clean=2, iterations_more_outliers=2)      # the schedule at which trial counts can be compared

MAIN_SEED, DEFAULT_SEED, VARIANT_SEED, EDGE_SEED, DENSE_SEED = 2, 4, 11, 3, 31
DENSE = dict(SHORT, min_inliers=8)      # dense information upweights some residuals: more matches go after round one than in main_batch

VARIANTS = {
    "no_kernel": dict(SHORT, huber_delta=0.0),
    "plain_second_round": dict(SHORT, robust_second_round=0),
    "clean_and_outlier_counts": dict(iterations_first=2, iterations_more_clean=1, iterations_more_outliers=2),
}


@functools.lru_cache(None)
def main_batch(seed=MAIN_SEED):
    """96 pairs, every count of COUNTS at least ten times, every second pair fix_scale, 10 % outliers."""
    rng = np.random.default_rng(seed)
    counts = np.concatenate([np.array(COUNTS), rng.choice(COUNTS, 96 - len(COUNTS))])
    counts[:2 * len(COUNTS)] = np.repeat(COUNTS, 2)          # each count with and without fix_scale
    return sp.synth_sim3_pairs(96, counts, 0.1, seed, START)


@functools.lru_cache(None)
def default_batch(seed=DEFAULT_SEED):
    """32 pairs for the default schedule (5, then 10 or 5)."""
    rng = np.random.default_rng(seed)
    return sp.synth_sim3_pairs(32, rng.choice(COUNTS, 32), 0.1, seed, START)


@functools.lru_cache(None)
def variant_batch(seed=VARIANT_SEED):
    """12 pairs: the first four without an outlier and with less noise (of these some lose no match after round one: "clean"), the rest with 15 % outliers."""
    clean = sp.synth_sim3_pairs(4, [20, 20, 64, 65], 0.0, seed, START, pixel_sigma=0.7, point_sigma=0.002)
    dirty = sp.synth_sim3_pairs(8, [20, 63, 64, 65, 100, 128, 129, 40], 0.15, seed + 1000, START)
    return sp.concat_batches([clean, dirty])


def variant_pairs(name, seed=VARIANT_SEED):
    """The batch a variant runs on: only the one about the two second-round counts needs the clean pairs.  A clean pair's second round
    repeats the problem of its first, so that variant's first round is 2 iterations long: after 3 these low-noise pairs have converged and
    the second round's rho is rounding noise (7.5e-9, 8.5e-10); after 2 it is >= 6e-4 and both precisions run the same trials."""
    b = variant_batch(seed)
    return b if name == "clean_and_outlier_counts" else sp.take_pairs(b, range(4, 12))


@functools.lru_cache(None)
def edge_batch():
    """48 matches over 4 pairs, the second one fix_scale."""
    return sp.synth_sim3_pairs(4, 12, 0.1, EDGE_SEED, START, fix_scale=[0, 1, 0, 0])


def _copy(batch):
    return {k: np.array(v, copy=True) for k, v in batch.items()}


def _cam(P, K):
    return np.stack([P[:, 0] / P[:, 2] * K[0] + K[2], P[:, 1] / P[:, 2] * K[1] + K[3]], 1)


def with_distinct_intrinsics(batch, seed):
    """Every pair its own two cameras: fx within 5 % of the generator's, fy 2 .. 6 % off fx to either side, cx and cy moved by up to 8 and 5
    pixels, drawn per camera.  Every keypoint is moved by what the new camera changes in the projection of its stored point, so its noise
    and the outliers stay what they were."""
    rng = np.random.default_rng(seed)
    out = _copy(batch)
    n = len(batch["S12"])
    for c in (0, 4):
        fx = batch["intr"][:, c] * rng.uniform(0.95, 1.05, n)
        out["intr"][:, c] = fx
        out["intr"][:, c + 1] = fx * (1 + rng.choice([-1.0, 1.0], n) * rng.uniform(0.02, 0.06, n))
        out["intr"][:, c + 2] += rng.uniform(-8, 8, n)
        out["intr"][:, c + 3] += rng.uniform(-5, 5, n)
    ptr = batch["match_ptr"]
    for f in range(n):
        s = slice(ptr[f], ptr[f + 1])
        out["obs1"][s] += _cam(batch["P1"][s], out["intr"][f, :4]) - _cam(batch["P1"][s], batch["intr"][f, :4])
        out["obs2"][s] += _cam(batch["P2"][s], out["intr"][f, 4:]) - _cam(batch["P2"][s], batch["intr"][f, 4:])
    assert np.all(np.abs(out["intr"][:, [1, 5]] / out["intr"][:, [0, 4]] - 1) >= 0.02)
    assert all(len(np.unique(out["intr"][:, k])) == n for k in range(8)) and np.all(out["intr"][:, :4] != out["intr"][:, 4:])
    return out


def with_dense_information(batch, seed):
    """Every edge its own dense 2 x 2 information Q diag(d) Q^T, symmetric to the last bit and positive definite: Q a random rotation, d the
    edge's level weight times factors of 1 / sqrt(5) .. sqrt(5) (eigenvalue ratio up to 5); info12 and info21 drawn independently."""
    rng = np.random.default_rng(seed)
    out = _copy(batch)
    N = len(batch["P1"])
    for key in ("info12", "info21"):
        w = batch[key][:, 0]
        d = w[:, None] * np.exp(rng.uniform(-0.5 * np.log(5.0), 0.5 * np.log(5.0), (N, 2)))
        ang = rng.uniform(0, 2 * np.pi, N)
        c, s = np.cos(ang), np.sin(ang)
        off = c * s * (d[:, 0] - d[:, 1])
        out[key] = np.stack([c * c * d[:, 0] + s * s * d[:, 1], off, off, s * s * d[:, 0] + c * c * d[:, 1]], 1)
    return out


def told_apart(batch, seed):
    return with_dense_information(with_distinct_intrinsics(batch, seed + 100), seed + 200)


@functools.lru_cache(None)
def dense_batch(seed=DENSE_SEED):
    """24 pairs over COUNTS, every second pair fix_scale, 10 % outliers, each pair with its own cameras and each edge with its own dense information."""
    rng = np.random.default_rng(seed)
    counts = np.concatenate([np.array(COUNTS), np.array(COUNTS), rng.choice(COUNTS, 24 - 2 * len(COUNTS))])
    return told_apart(sp.synth_sim3_pairs(24, counts, 0.1, seed, START), seed)


@functools.lru_cache(None)
def dense_edge_batch():
    """edge_batch() with per-pair, per-camera intrinsics (cs_sim3_pairs_linearize takes no information: its blocks are the errors and Jacobians)."""
    return told_apart(edge_batch(), EDGE_SEED)


@functools.lru_cache(None)
def run(name, long_double=False, seed=None):
    """Reference results of a named case: 'main', 'default', 'dense', or a key of VARIANTS (seed: another batch of the same make, for choosing seeds)."""
    dtype = np.longdouble if long_double else np.float64
    kw = {} if seed is None else dict(seed=seed)
    if name == "dense":
        return ref.optimize_batch(dense_batch(**kw), ref.params(**DENSE), dtype)
    if name == "main":
        return ref.optimize_batch(main_batch(**kw), ref.params(**SHORT), dtype)
    if name == "default":
        return ref.optimize_batch(default_batch(**kw), ref.params(), dtype)
    return ref.optimize_batch(variant_pairs(name, **kw), ref.params(**VARIANTS[name]), dtype)


@functools.lru_cache(None)
def edge_blocks(long_double=False, dense=False):
    """(err (48, 4), jac (48, 2, 2, 7)) of edge_batch() -- dense: of dense_edge_batch() -- at its start states."""
    b = dense_edge_batch() if dense else edge_batch()
    dtype = np.longdouble if long_double else np.float64
    errs, jacs = [], []
    for f in range(len(b["S12"])):
        p = ref.pair_of(b, f, dtype)
        e12, e21, J12, J21 = ref.linearize(p, p["S"])
        errs.append(np.concatenate([e12, e21], -1))
        jacs.append(np.stack([J12, J21], 1))
    return np.concatenate(errs), np.concatenate(jacs)


def state_deviation(a, b):
    """Per pair: the largest state difference against the largest of b's eight numbers."""
    a, b = np.asarray(a, np.longdouble).reshape(-1, 8), np.asarray(b, np.longdouble).reshape(-1, 8)
    return (np.abs(a - b).max(-1) / np.abs(b).max(-1)).astype(np.float64)


def comparable(name, seed=None):
    """The conditions of a case, measured: dict of same_trials, same_inliers, min_abs_rho, min_margin, state_dev."""
    r64, rld = run(name, False, seed), run(name, True, seed)
    return dict(same_trials=all(a["trials"] == b["trials"] and a["iterations"] == b["iterations"] for a, b in zip(r64, rld)),
                same_inliers=all(np.array_equal(a["inlier"], b["inlier"]) for a, b in zip(r64, rld)),
                min_abs_rho=min(ref.min_abs_rho(r64), ref.min_abs_rho(rld)),
                min_margin=min(min(a["margin"] for a in r64), min(a["margin"] for a in rld)),
                state_dev=float(state_deviation([a["S"] for a in r64], [a["S"] for a in rld]).max()))


def compare_with_reference(got, res, what, iterations=True):
    """The contract: iterations_done and inlier flags identical, states and chi2 within 1e-5 relative.  Returns the deviations."""
    assert len(got["S12"]) == len(res)
    if iterations:
        assert got["iterations"].tolist() == [r["iterations"] for r in res], what
    assert np.array_equal(got["inlier"], np.concatenate([r["inlier"] for r in res])), what
    assert got["n_inliers"].tolist() == [r["n_inliers"] for r in res], what
    dev = float(state_deviation(got["S12"], [r["S"] for r in res]).max())
    ref_chi = np.array([[float(c) for c in r["chi2"]] for r in res])
    ran = ref_chi > 0
    chi_dev = float((np.abs(got["chi2"] - ref_chi)[ran] / ref_chi[ran]).max())
    assert np.all(got["chi2"][~ran] == 0), what
    print("%s: states %.3g, chi2 %.3g" % (what, dev, chi_dev))
    assert dev < 1e-5 and chi_dev < 1e-5, (what, dev, chi_dev)
    return dev, chi_dev
