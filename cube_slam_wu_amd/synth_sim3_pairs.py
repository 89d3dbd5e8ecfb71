"""Seeded synthetic batches for the Sim(3) alignment of keyframe pairs (capi.Sim3Pairs / cs_sim3_optimize_pairs).

Per pair: two pinhole cameras (the KITTI odometry intrinsics of sequences 00-02 and 04-12), a true S12 (camera-2 to camera-1 coordinates:
a rotation of about 0.2 rad, a translation of about 0.4 m, scale 1.2 -- or scale exactly 1 with fix_scale), points 3 .. 10 m deep in
camera 1, keypoints with 1 px noise at level 0 (sigma = 1.2^level, information 1 / 1.2^(2 level), level 0 .. 7), 2 cm noise on both
stored points, a share of outliers whose two keypoints are moved by up to 40 px, and a start S12 that is off by a (rad, m, log-scale) sigma
triple.  States are qx qy qz qw tx ty tz s (Sim3::operator[] order).
"""
from __future__ import annotations

import numpy as np

from .synth_pose import IMG_H, IMG_W, _axis_angle_quat, _quat_mul, _quat_rot

INTR_CAM1 = np.array([718.856, 718.856, 607.1928, 185.2157])
INTR_CAM2 = np.array([707.0912, 707.0912, 601.8873, 183.1104])

PAIR_KEYS = ("S12", "S12_true", "intr", "fix_scale")
MATCH_KEYS = ("P1", "P2", "obs1", "obs2", "info12", "info21", "is_outlier")


def _unit(q):
    q = q / np.linalg.norm(q)
    return q if q[3] >= 0 else -q


def synth_sim3_pairs(n_pairs, n_matches, outlier_share=0.1, seed=0, start_sigma=(0.05, 0.1, 0.05), fix_scale=None, pixel_sigma=1.0, point_sigma=0.02):
    """n_pairs pairs; n_matches = matches per pair: an int, a (lo, hi) tuple drawn per pair, or a list / array of n_pairs counts.
    fix_scale: None = every second pair (the odd ones), or one flag per pair.  pixel_sigma / point_sigma: the keypoint noise at level 0 (px)
    and the noise of the stored points (m).

    Returns a dict of flat arrays in the C ABI's layout: S12 (n, 8) the start, S12_true, intr (n, 8), fix_scale (n, uint8), match_ptr
    (n + 1, int32), P1, P2 (N, 3), obs1, obs2 (N, 2), info12, info21 (N, 4), is_outlier (N, bool)."""
    rng = np.random.default_rng(seed)
    if np.isscalar(n_matches):
        counts = np.full(n_pairs, int(n_matches))
    elif isinstance(n_matches, tuple) and len(n_matches) == 2:
        counts = rng.integers(int(n_matches[0]), int(n_matches[1]) + 1, n_pairs)
    else:
        counts = np.asarray(n_matches, np.int64)
        assert len(counts) == n_pairs
    fs = (np.arange(n_pairs) % 2 == 1) if fix_scale is None else np.asarray(fix_scale).astype(bool)
    assert len(fs) == n_pairs
    out = {k: [] for k in PAIR_KEYS + MATCH_KEYS}
    for f in range(n_pairs):
        n = int(counts[f])
        q = _unit(_axis_angle_quat(rng.normal(0, 0.2 / np.sqrt(3), 3)))
        t = rng.normal(0, 0.4 / np.sqrt(3), 3)
        s = 1.0 if fs[f] else 1.2
        R = _quat_rot(q)
        u, v = rng.uniform(20, IMG_W - 20, n), rng.uniform(20, IMG_H - 20, n)
        z = rng.uniform(3.0, 10.0, n)
        P1 = np.stack([(u - INTR_CAM1[2]) / INTR_CAM1[0] * z, (v - INTR_CAM1[3]) / INTR_CAM1[1] * z, z], 1)
        P2 = ((P1 - t) @ R) / s                                     # S12^-1: R^T (P1 - t) / s
        proj = lambda P, K: np.stack([P[:, 0] / P[:, 2] * K[0] + K[2], P[:, 1] / P[:, 2] * K[1] + K[3]], 1)
        lv1, lv2 = rng.integers(0, 8, n), rng.integers(0, 8, n)
        obs1 = proj(P1, INTR_CAM1) + rng.normal(0, pixel_sigma, (n, 2)) * (1.2 ** lv1)[:, None]
        obs2 = proj(P2, INTR_CAM2) + rng.normal(0, pixel_sigma, (n, 2)) * (1.2 ** lv2)[:, None]
        bad = rng.random(n) < outlier_share
        k = int(bad.sum())
        for obs in (obs1, obs2):
            ang, mag = rng.uniform(0, 2 * np.pi, k), rng.uniform(0, 40.0, k)
            obs[bad] += np.stack([mag * np.cos(ang), mag * np.sin(ang)], 1)
        eye = np.array([1.0, 0.0, 0.0, 1.0])
        info12, info21 = eye[None] / (1.2 ** (2 * lv1))[:, None], eye[None] / (1.2 ** (2 * lv2))[:, None]
        P1n, P2n = P1 + rng.normal(0, point_sigma, (n, 3)), P2 + rng.normal(0, point_sigma, (n, 3))
        # the start: exp of a small twist times the truth (rotation and translation perturbed, the scale by a log-normal factor unless fixed)
        dq = _axis_angle_quat(rng.normal(0, start_sigma[0] / np.sqrt(3), 3))
        ds = 1.0 if fs[f] else float(np.exp(rng.normal(0, start_sigma[2])))
        q0 = _unit(_quat_mul(dq, q))
        t0 = ds * (_quat_rot(dq) @ t) + rng.normal(0, start_sigma[1] / np.sqrt(3), 3)
        out["S12"].append(np.concatenate([q0, t0, [s * ds]])); out["S12_true"].append(np.concatenate([q, t, [s]]))
        out["intr"].append(np.concatenate([INTR_CAM1, INTR_CAM2])); out["fix_scale"].append(np.uint8(fs[f]))
        for key, val in (("P1", P1n), ("P2", P2n), ("obs1", obs1), ("obs2", obs2), ("info12", info12), ("info21", info21), ("is_outlier", bad)):
            out[key].append(val)
    widths = dict(S12=8, S12_true=8, intr=8, P1=3, P2=3, obs1=2, obs2=2, info12=4, info21=4)
    res = {}
    for key in ("S12", "S12_true", "intr"):
        res[key] = np.array(out[key], np.float64).reshape(-1, widths[key])
    res["fix_scale"] = np.array(out["fix_scale"], np.uint8).reshape(-1)
    for key in ("P1", "P2", "obs1", "obs2", "info12", "info21"):
        res[key] = (np.concatenate(out[key]) if out[key] else np.zeros((0, widths[key]))).reshape(-1, widths[key]).astype(np.float64)
    res["is_outlier"] = (np.concatenate(out["is_outlier"]) if out["is_outlier"] else np.zeros(0, bool)).astype(bool)
    ptr = np.zeros(n_pairs + 1, np.int32)
    ptr[1:] = np.cumsum(counts)
    res["match_ptr"] = ptr
    return res


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
