"""The batches tests/test_sim3_ransac_gpu.py runs and their reference results (tests/sim3_ransac_ref.py), built once per process.
tests/test_sim3_ransac_ref.py asserts, without a GPU, the conditions under which a float64 reference may be compared at all -- for every
hypothesis the reference evaluates on every pair of every batch here, none dropped: the seeds below are ones for which the reference
alone meets them, and for which the hard batch holds the selection cases it is there for."""
import functools

import numpy as np

from cube_slam_wu_amd import synth_sim3_pairs as sp
from cube_slam_wu_amd import synth_sim3_ransac as sr
import sim3_ransac_ref as ref

CHUNK = 64                                                   # csrc/sim3_ransac_types.h: SIM3_RANSAC_CHUNK; CHUNK - 1, CHUNK, CHUNK + 1 and 2 CHUNK + 1 are among the counts
EASY_COUNTS = (3, 19, 20, 21, 40, 63, 64, 65, 100, 127, 128, 129, 200, 257)
HARD_COUNTS = (64, 100, 129, 200, 257, 257)
EASY_SEED, HARD_SEED, DEGENERATE_SEED = 5, 19, 9
MISMATCH_SHARE = 0.75
POINT_SIGMA = 0.005                                          # 5 mm on a stored point 3 .. 10 m away: about a pixel

VARIANTS = {"max_iterations_1": 1, "max_iterations_63": 63, "max_iterations_64": 64, "max_iterations_65": 65}
NAMES = ("easy", "hard") + tuple(VARIANTS) + ("degenerate",)


@functools.lru_cache(None)
def easy_batch(seed=EASY_SEED):
    """One pair per count of EASY_COUNTS, every second pair fix_scale, no mismatch."""
    return sr.synth_sim3_ransac(len(EASY_COUNTS), list(EASY_COUNTS), 0.0, seed, point_sigma=POINT_SIGMA)


@functools.lru_cache(None)
def hard_batch(seed=HARD_SEED):
    """One pair per count of HARD_COUNTS, three of four matches mismatched."""
    return sr.synth_sim3_ransac(len(HARD_COUNTS), list(HARD_COUNTS), MISMATCH_SHARE, seed, point_sigma=POINT_SIGMA)


@functools.lru_cache(None)
def degenerate_batch(seed=DEGENERATE_SEED):
    """Run at min_inliers = 2.  Pairs: 0 ordinary (40 matches), 1 without a match, 2 ordinary (65), 3 three matches to ONE camera-2 point
    (collinear in camera 1: the centred camera-2 triple is zero, s = 0 / 0, every hypothesis refused), 4 a proper, exact triple,
    5 40 matches of which one has P1.z = 0 and another P2.z = 0."""
    b = sr.synth_sim3_ransac(6, [40, 0, 65, 3, 3, 40], 0.0, seed, point_sigma=POINT_SIGMA, fix_scale=[0, 0, 1, 0, 0, 0])
    ptr = b["match_ptr"]
    a = int(ptr[3])
    b["P1"][a:a + 3] = b["P1"][a] + np.outer([0.0, 1.0, 2.5], [0.3, -0.2, 0.4])
    b["P2"][a:a + 3] = [0.5, -0.25, 4.0]                     # (three times a dyadic value, and a third of that, are exact: the centred triple is exactly zero)
    a = int(ptr[4])
    q, t, s = b["S12_true"][4, :4], b["S12_true"][4, 4:7], b["S12_true"][4, 7]
    R = sp._quat_rot(q)
    b["P2"][a:a + 3] = ((b["P1"][a:a + 3] - t) @ R) / s
    a = int(ptr[5])
    b["P1"][a + 7, 2] = 0.0
    b["P2"][a + 11, 2] = 0.0
    return b


def batch_of(name):
    return easy_batch() if name == "easy" else degenerate_batch() if name == "degenerate" else hard_batch()


def params_of(name):
    if name in VARIANTS:
        return ref.params(max_iterations=VARIANTS[name])
    return ref.params(min_inliers=2) if name == "degenerate" else ref.params()


@functools.lru_cache(None)
def run(name):
    """Per pair: the float64 reference's result, with `dev` = its S12's deviation from the long-double run of the same hypothesis, and what
    the comparison of the two precisions over every hypothesis evaluated found (`flips`, `worst_ratio`, `min_margin`)."""
    batch, prm = batch_of(name), params_of(name)
    out = []
    for f in range(len(batch["match_ptr"]) - 1):
        p64, pld = ref.pair_of(batch, f), ref.pair_of(batch, f, np.longdouble)
        trace = []
        res = ref.run_pair(p64, prm, trace)
        flips, worst, margin, refusals_differ = 0, 0.0, np.inf, 0
        for h, hyp, e1, e2, fl in trace:
            hyp_ld, l1, l2, fl_ld = ref.evaluate(pld, h)
            if (hyp is None) != (hyp_ld is None):
                refusals_differ += 1
            if hyp is None or hyp_ld is None:
                continue
            flips += int(np.sum(fl != fl_ld))
            for e, l, th in ((e1, l1, p64["th1"]), (e2, l2, p64["th2"])):
                ok = np.isfinite(e) & np.isfinite(np.asarray(l, np.float64))
                flips += int(np.sum(np.isfinite(e) != np.isfinite(np.asarray(l, np.float64))))
                if ok.any():
                    gap = np.abs(e[ok] - th[ok])
                    with np.errstate(divide="ignore", invalid="ignore"):
                        ratio = np.float64(np.abs(e[ok] - l[ok])) / gap
                    worst = max(worst, float(np.nanmax(np.where(gap > 0, ratio, np.inf))))
                    pos = th[ok] > 0
                    if pos.any():
                        margin = min(margin, float(np.abs(e[ok][pos] / th[ok][pos] - 1).min()))
            if h == res["hyp"]:
                res["dev"] = float(ref.s12_deviation(ref.s12_of(hyp), ref.s12_of(hyp_ld, np.longdouble)))
        res.setdefault("dev", 0.0)
        res.update(flips=flips, worst_ratio=worst, min_margin=margin, refusals_differ=refusals_differ)
        out.append(res)
    return out


def tolerance(dev):
    """Of an S12, relative to its largest entry."""
    return max(100.0 * dev, 1e-13)


def compare_with_reference(got, res, what):
    """got: dict of arrays over the batch (found, hyp, iterations, n_inliers, S12, inlier); res: run(name)."""
    n = len(res)
    for k in ("found", "hyp", "iterations", "n_inliers"):
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), [r[k] for r in res]), (what, k, np.asarray(got[k]).tolist(), [r[k] for r in res])
    assert np.array_equal(np.asarray(got["inlier"]).astype(np.uint8), np.concatenate([r["inlier"] for r in res]).astype(np.uint8)), (what, "inlier")
    worst = 0.0
    for f in range(n):
        dev = float(ref.s12_deviation(res[f]["S12"], np.asarray(got["S12"])[f]))
        worst = max(worst, dev / tolerance(res[f]["dev"]))
        print("%s pair %d: S12 deviation %.3g, reference's own %.3g, tolerance %.3g" % (what, f, dev, res[f]["dev"], tolerance(res[f]["dev"])))
        assert dev <= tolerance(res[f]["dev"]), (what, f, dev, res[f]["dev"])
    return worst


HYPOTHESES_PAIR, HYPOTHESES_COUNT = 1, 300      # of the hard batch: the pair cs_sim3_ransac_hypotheses is held to the reference on


@functools.lru_cache(None)
def hypotheses(f=HYPOTHESES_PAIR, n_hyp=HYPOTHESES_COUNT):
    """Every hypothesis 0 .. n_hyp - 1 of hard pair f without selection: (count (n_hyp), -1 = refused; S12 (n_hyp, 8) in float64; the
    deviation of each from its long-double evaluation)."""
    p64, pld = ref.pair_of(hard_batch(), f), ref.pair_of(hard_batch(), f, np.longdouble)
    cnt, S, dev = np.zeros(n_hyp, np.int64), np.zeros((n_hyp, 8)), np.zeros(n_hyp)
    for h in range(n_hyp):
        hyp, _, _, fl = ref.evaluate(p64, h)
        hyp_ld = ref.evaluate(pld, h)[0]
        assert (hyp is None) == (hyp_ld is None), h
        cnt[h] = -1 if hyp is None else int(fl.sum())
        S[h] = ref.s12_of(hyp)
        dev[h] = 0.0 if hyp is None else float(ref.s12_deviation(ref.s12_of(hyp), ref.s12_of(hyp_ld, np.longdouble)))
    return cnt, S, dev


def compare_hypotheses(cnt, S, what):
    """cnt (n_hyp), S (n_hyp, 8) of hard pair HYPOTHESES_PAIR against hypotheses()."""
    rc, rS, rdev = hypotheses()
    assert np.array_equal(np.asarray(cnt).astype(np.int64), rc), (what, np.flatnonzero(np.asarray(cnt) != rc))
    dev = ref.s12_deviation(rS, np.asarray(S))
    tol = np.maximum(100.0 * rdev, 1e-13)
    print("%s: %d hypotheses, worst S12 deviation %.3g (its tolerance %.3g); the reference's own worst %.3g" % (what, len(rc), dev.max(), tol[np.argmax(dev / tol)], rdev.max()))
    assert np.all(dev <= tol), (what, np.flatnonzero(dev > tol), dev.max())
