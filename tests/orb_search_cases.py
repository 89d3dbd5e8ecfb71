"""The batches tests/test_orb_search_gpu.py runs and their reference results (tests/orb_search_ref.py), built once per process.
tests/test_orb_search_ref.py asserts, without a GPU, the conditions under which a float64 reference may be compared at all -- for every
query of every batch here, none dropped: the seeds below are ones for which the reference alone meets them, for which the crowded batch
holds every status, and for which the single query is matched."""
import functools

import numpy as np

from cube_slam_wu_amd import synth_orb_search as so
import orb_search_ref as ref

CHUNK = 64                                                   # csrc/orb_search_types.h: ORB_CHUNK; 0, 1, CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 1 are among the counts
EASY_SEED, CROWDED_SEED, SINGLE_SEED, TWO_WAY_SEED = 2, 7, 1, 4
EASY_FRAME_KEYPOINTS = (0, 1, 65, 300, 300)                  # frames 0, 2 and 4 are stereo, 1 and 3 mono
EASY_JOBS = (dict(frame=3, count=0, flags=so.FUSE, th=3.0, max_hamming=so.TH_LOW), dict(frame=3, count=1, flags=so.FUSE, th=3.0, max_hamming=so.TH_LOW),
             dict(frame=3, count=63, flags=so.FUSE_SIM3, th=4.0, max_hamming=so.TH_LOW), dict(frame=4, count=64, flags=so.SEARCH_BY_SIM3, th=7.5, max_hamming=so.TH_HIGH, s=0.8),
             dict(frame=4, count=65, flags=so.FUSE, th=3.0, max_hamming=so.TH_LOW), dict(frame=3, count=129, flags=so.FUSE, th=3.0, max_hamming=so.TH_LOW),
             dict(frame=0, count=40, flags=so.FUSE, th=3.0, max_hamming=so.TH_LOW), dict(frame=1, count=40, flags=so.SEARCH_BY_SIM3, th=7.5, max_hamming=so.TH_HIGH),
             dict(frame=2, count=65, flags=so.FUSE_SIM3, th=4.0, max_hamming=so.TH_LOW, s=1.3), dict(frame=4, count=129, flags=so.FUSE_SIM3, th=4.0, max_hamming=so.TH_LOW))
EASY_COUNTS = tuple(j["count"] for j in EASY_JOBS)
CROWDED_GRID = (4, 3)
CROWDED_KEYPOINTS = 200
CROWDED_JOBS = (dict(frame=0, count=150, flags=so.SEARCH_BY_SIM3, th=40.0, max_hamming=so.TH_HIGH), dict(frame=0, count=150, flags=so.FUSE, th=40.0, max_hamming=so.TH_LOW),
                dict(frame=0, count=100, flags=so.FUSE_SIM3, th=40.0, max_hamming=so.TH_LOW))
CROWDED_PLANT_JOB = 0

NAMES = ("easy", "crowded", "single")


@functools.lru_cache(None)
def easy_batch(seed=EASY_SEED):
    """One job per count of EASY_COUNTS over frames of 0, 1, 65 and 300 keypoints, the default grid, all three flag combinations."""
    return so.synth_orb_search(EASY_FRAME_KEYPOINTS, EASY_JOBS, seed)


@functools.lru_cache(None)
def crowded_batch(seed=CROWDED_SEED):
    """A 4 x 3 grid over 200 keypoints and windows of 40 px times the level's scale: cells hold many keypoints, windows span several cells.
    Job 0 holds the planted ties and the off-grid keypoints."""
    return so.synth_orb_search((CROWDED_KEYPOINTS,), CROWDED_JOBS, seed, grid=CROWDED_GRID, plant_job=CROWDED_PLANT_JOB, stereo=(1,))


@functools.lru_cache(None)
def single_batch(seed=SINGLE_SEED):
    return so.synth_orb_search((1,), (dict(frame=0, count=1, flags=so.FUSE, th=3.0, max_hamming=so.TH_LOW),), seed, n_points=1, families=("good",))


@functools.lru_cache(None)
def two_way_batch(seed=TWO_WAY_SEED):
    """SearchBySim3's two directions over two crowded keyframes: job 0 searches keyframe 1 for the points of keyframe 0's keypoints (query
    i belongs to keypoint i of keyframe 0), job 1 the other way round."""
    return so.two_directions((CROWDED_KEYPOINTS, CROWDED_KEYPOINTS), seed, th=40.0, max_hamming=so.TH_HIGH, grid=CROWDED_GRID)


def batch_of(name):
    return {"easy": easy_batch, "crowded": crowded_batch, "single": single_batch, "two_way": two_way_batch}[name]()


def params_of(name):
    g = batch_of(name)["grid"]
    return ref.params(grid_cols=int(g[0]), grid_rows=int(g[1]))


def _insp(r, dt=np.float64):
    return np.stack([np.asarray(r[k], dt) for k in ref.INSPECT], axis=1)


def _ratios(d64, dld):
    """Per comparison |d64 - dld| / |d64| (inf where d64 is 0) and |d64|."""
    d, dl = np.asarray(d64, np.float64), np.asarray(dld, np.longdouble)
    gap = np.abs(d)
    with np.errstate(all="ignore"):
        ratio = np.where(gap > 0, (np.abs(d - dl) / gap).astype(np.float64), np.inf)
    return np.where(np.isnan(ratio), np.inf, ratio), gap


@functools.lru_cache(None)
def run(name):
    """The float64 reference's result over the batch, with what the comparison with the long-double run found:
    flips        queries whose integer outputs differ between the two, plus comparisons made by only one of the two, plus keypoints whose
                 cell differs
    worst_ratio  over every threshold comparison made, |d64 - dld| / |d64| with d = lhs - rhs (inf where d64 is 0); for a keypoint's cell
                 d is the distance of the floor's argument to the nearer integer
    min_gap      the smallest |d64| met, with the comparison's name;  n_comparisons  how many were made
    dev          (Q) the inspection outputs' own deviation |v64 - vld| relative to `scale` = max(1, the largest of their magnitudes)"""
    batch, prm = batch_of(name), params_of(name)
    r64, rld = ref.run(batch, prm, np.float64), ref.run(batch, prm, np.longdouble)
    flips = int(sum(np.sum(np.asarray(r64[k]) != np.asarray(rld[k])) for k in ref.INTEGER_OUT + ("n_ok",)))
    worst, min_gap, count = 0.0, (np.inf, ""), 0
    for (cname, key, d), (_, keyl, dl) in zip(r64["comparisons"], rld["comparisons"]):
        if key.shape != keyl.shape or not np.array_equal(key, keyl):
            flips += 1
            continue
        if not len(d):
            continue
        ratio, gap = _ratios(d, dl)
        worst, count = max(worst, float(ratio.max())), count + len(d)
        if gap.min() < min_gap[0]:
            min_gap = (float(gap.min()), cname)
    for f in range(len(r64["cells"])):
        flips += int(np.sum(r64["cells"][f] != rld["cells"][f]))
        for axis in range(2):
            a, al, fl = r64["cell_args"][f][axis], rld["cell_args"][f][axis], r64["cell_floors"][f][axis]
            if not len(a):
                continue
            to_lower, to_upper = a - fl, (fl + 1.0) - a
            nearer = np.where(to_lower < to_upper, to_lower, -to_upper)            # a - the nearer integer
            nearer_l = np.where(to_lower < to_upper, al - fl.astype(np.longdouble), al - (fl.astype(np.longdouble) + 1))
            ratio, gap = _ratios(nearer, nearer_l)
            worst, count = max(worst, float(ratio.max())), count + len(a)
            if gap.min() < min_gap[0]:
                min_gap = (float(gap.min()), "a keypoint's cell")
    i64, ild = _insp(r64, np.longdouble), _insp(rld, np.longdouble)
    scale = np.maximum(1.0, np.abs(_insp(r64)).max(axis=1)) if len(i64) else np.zeros(0)
    dev = (np.abs(i64 - ild).max(axis=1) / scale).astype(np.float64) if len(i64) else np.zeros(0)
    out = dict(r64)
    out.update(flips=flips, worst_ratio=worst, min_gap=min_gap, n_comparisons=count, dev=dev, scale=scale)
    return out


def tolerance(dev):
    return np.maximum(100.0 * np.asarray(dev), 1e-13)


def compare_with_reference(got, res, what, inspect=False, exact=False):
    """got: dict of arrays over the batch (status, best_idx, best_dist, level, n_ok[, insp5, n_window, n_candidates]); res: run(name).
    exact: the inspection doubles must be the reference's bits.  -> the largest deviation of the inspection doubles met, relative to `scale`."""
    keys = ("status", "best_idx", "best_dist", "level", "n_ok") + (("n_window", "n_candidates") if inspect else ())
    for k in keys:
        a, b = np.asarray(got[k]).astype(np.int64), np.asarray(res[k]).astype(np.int64)
        assert np.array_equal(a, b), (what, k, np.flatnonzero(a != b)[:10], a[a != b][:10], b[a != b][:10])
    if not inspect or not len(res["scale"]):
        return 0.0
    want = _insp(res)
    dev = np.abs(np.asarray(got["insp5"]) - want).max(axis=1) / res["scale"]
    tol = tolerance(res["dev"])
    print("%s: %d queries, u v ur dist radius worst deviation %.3g of their scale (its tolerance %.3g); the reference's own worst %.3g" % (what, len(dev), dev.max(), tol[np.argmax(dev / tol)], res["dev"].max()))
    assert np.all(dev <= tol), (what, np.flatnonzero(dev > tol), dev.max())
    if exact:
        assert np.array_equal(np.asarray(got["insp5"]), want), (what, "the inspection doubles are not the reference's bits")
    return float(dev.max())
