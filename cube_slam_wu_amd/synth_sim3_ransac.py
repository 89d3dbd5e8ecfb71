"""Seeded synthetic batches for the Sim(3) RANSAC of keyframe pairs (capi.Sim3Ransac / cs_sim3_ransac_pairs).

Takes a synth_sim3_pairs batch and adds what the RANSAC stage needs: the squared pixel thresholds of ORB-SLAM2's Sim3Solver
(9.210 * sigma2 of the keypoint's octave = 9.210 / the information's diagonal), one 64-bit seed per pair, and MISMATCHES.  The pair
generator's own outliers move keypoints only, which this stage never reads (it tests a hypothesis against the projections of the stored
points); a mismatch is a share of a pair's matches whose P2 rows are permuted among themselves -- the point in camera 2 then belongs to
another match."""
from __future__ import annotations

import numpy as np

from . import synth_sim3_pairs as sp

CHI2_2DOF_99 = 9.210

PAIR_KEYS = sp.PAIR_KEYS + ("seed",)
MATCH_KEYS = sp.MATCH_KEYS + ("max_err1", "max_err2", "is_mismatch")


def add_ransac_inputs(batch, mismatch_share=0.0, seed=0):
    """A copy of `batch` (synth_sim3_pairs layout) with max_err1, max_err2 (N), is_mismatch (N, bool) and seed (n, uint64).
    Per pair round(mismatch_share * count) matches (none where that is fewer than two) get each other's P2, by a cyclic shift of a random order: none keeps its own."""
    rng = np.random.default_rng([int(seed), 0x51B3])
    out = {k: np.array(v, copy=True) for k, v in batch.items()}
    out["max_err1"] = CHI2_2DOF_99 / out["info12"][:, 0]
    out["max_err2"] = CHI2_2DOF_99 / out["info21"][:, 0]
    ptr = out["match_ptr"]
    bad = np.zeros(int(ptr[-1]), bool)
    for f in range(len(ptr) - 1):
        a, n = int(ptr[f]), int(ptr[f + 1] - ptr[f])
        k = int(round(mismatch_share * n))
        if k < 2:
            continue
        who = a + rng.permutation(n)[:k]
        out["P2"][who] = out["P2"][np.roll(who, 1)]
        bad[who] = True
    out["is_mismatch"] = bad
    out["seed"] = rng.integers(0, 2 ** 63, len(ptr) - 1, dtype=np.uint64)
    return out


def synth_sim3_ransac(n_pairs, n_matches, mismatch_share=0.3, seed=0, **kw):
    """synth_sim3_pairs(n_pairs, n_matches, seed=seed, **kw) with the RANSAC inputs added."""
    return add_ransac_inputs(sp.synth_sim3_pairs(n_pairs, n_matches, seed=seed, **kw), mismatch_share, seed)


def take_pairs(batch, idx):
    """The pairs `idx` of a batch, in that order, as a batch of their own."""
    idx = [int(i) for i in idx]
    ptr = batch["match_ptr"]
    sl = [np.arange(ptr[i], ptr[i + 1]) for i in idx]
    sel = np.concatenate(sl).astype(np.int64) if sl else np.zeros(0, np.int64)
    out = {k: batch[k][idx] for k in PAIR_KEYS}
    out.update({k: batch[k][sel] for k in MATCH_KEYS})
    match_ptr = np.zeros(len(idx) + 1, np.int32)
    match_ptr[1:] = np.cumsum([len(s) for s in sl])
    out["match_ptr"] = match_ptr
    return out


def concat_batches(batches):
    out = {k: np.concatenate([b[k] for b in batches]) for k in PAIR_KEYS + MATCH_KEYS}
    counts = np.concatenate([np.diff(b["match_ptr"]) for b in batches])
    out["match_ptr"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return out


def keep_flagged(batch, flags, pairs=None):
    """What LoopClosing::ComputeSim3 hands to OptimizeSim3: the pairs `pairs` (default: all) with only the matches whose flag is set."""
    pairs = [int(i) for i in (range(len(batch["match_ptr"]) - 1) if pairs is None else pairs)]
    sub = take_pairs(batch, pairs)
    ptr = batch["match_ptr"]
    keep = np.concatenate([np.asarray(flags[ptr[i]:ptr[i + 1]]).astype(bool) for i in pairs]) if pairs else np.zeros(0, bool)
    counts = [int(np.asarray(flags[ptr[i]:ptr[i + 1]]).astype(bool).sum()) for i in pairs]
    for k in MATCH_KEYS:
        sub[k] = sub[k][keep]
    sub["match_ptr"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return sub


def write_dump(path, batch, probability, min_inliers, max_iterations):
    """The batch as the text dump tools/hostonly/sim3_ransac_host_check.cpp reads (every double in %.17g)."""
    n, N = len(batch["intr"]), int(batch["match_ptr"][-1])
    g = lambda v: " ".join("%.17g" % float(x) for x in np.ravel(v))
    with open(path, "w") as f:
        f.write("%d %d\n" % (n, N))
        f.write("%.17g %d %d\n" % (probability, min_inliers, max_iterations))
        for i in range(n):
            f.write("%s %d %d %d %d\n" % (g(batch["intr"][i]), int(batch["fix_scale"][i]), int(batch["seed"][i]), int(batch["match_ptr"][i]), int(batch["match_ptr"][i + 1])))
        for m in range(N):
            f.write("%s\n" % g(np.concatenate([batch["P1"][m], batch["P2"][m], [batch["max_err1"][m], batch["max_err2"][m]]])))
