"""Seeded synthetic batches for the motion-only pose optimisation (capi.PoseBatch / cs_pose_optimize_batch).

KITTI-shaped frames: 1241 x 376 images, the odometry sequences' rectified intrinsics (fx = fy = 718.856, cx = 607.1928, cy = 185.2157,
bf = 386.1448), map points 4 .. 60 m in front of the camera, ORB-style information matrices (1 / 1.2^(2 level), level 0 .. 7).
"""
from __future__ import annotations

import numpy as np

IMG_W, IMG_H = 1241, 376
KITTI_INTR5 = np.array([718.856, 718.856, 607.1928, 185.2157, 386.1448])


def _quat_mul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz])


def _quat_rot(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _axis_angle_quat(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.array([0, 0, 0, 1.0])
    return np.concatenate([np.sin(th / 2) * w / th, [np.cos(th / 2)]])


def synth_pose_batch(n_frames, n_obs, stereo_share=0.0, outlier_share=0.1, seed=0, pose_sigma=(0.01, 0.05), pixel_sigma=1.0):
    """n_frames frames; n_obs = observations per frame: an int, a (lo, hi) tuple drawn per frame, or a list / array of n_frames counts.

    Per frame: a true world-to-camera pose, map points seen by it, measurements with pixel noise (sigma = pixel_sigma * 1.2^level),
    a share of gross outliers (measurement replaced by a random pixel), and an initial pose = the truth perturbed by a rotation of
    ~pose_sigma[0] rad and a translation of ~pose_sigma[1] m.  Returns a dict of flat arrays in the C ABI's layout: Tcw (n, 7) initial
    poses, Tcw_true, intr (n, 5), obs_ptr (n + 1, int32), Xw (N, 3), meas (N, 3), info (N, 9), is_stereo (N, uint8), is_outlier (N, bool).
    """
    rng = np.random.default_rng(seed)
    if np.isscalar(n_obs):
        counts = np.full(n_frames, int(n_obs))
    elif isinstance(n_obs, tuple) and len(n_obs) == 2:
        counts = rng.integers(int(n_obs[0]), int(n_obs[1]) + 1, n_frames)
    else:
        counts = np.asarray(n_obs, np.int64)
        assert len(counts) == n_frames
    fx, fy, cx, cy, bf = KITTI_INTR5
    Tcw, Ttrue, Xs, Ms, Ws, Ss, Os = [], [], [], [], [], [], []
    for f in range(n_frames):
        n = int(counts[f])
        q = _axis_angle_quat(rng.normal(0, 0.3, 3))
        t = rng.normal(0, 20.0, 3)
        R = _quat_rot(q)
        u, v = rng.uniform(20, IMG_W - 20, n), rng.uniform(20, IMG_H - 20, n)
        z = rng.uniform(4.0, 60.0, n)
        pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
        Xw = (pc - t) @ R                                   # R^T (pc - t)
        level = rng.integers(0, 8, n)
        sig = pixel_sigma * 1.2 ** level
        stereo = rng.random(n) < stereo_share
        meas = np.stack([u + rng.normal(0, 1, n) * sig, v + rng.normal(0, 1, n) * sig, u - bf / z + rng.normal(0, 1, n) * sig], 1)
        out = rng.random(n) < outlier_share
        k = int(out.sum())
        meas[out, 0], meas[out, 1] = rng.uniform(0, IMG_W, k), rng.uniform(0, IMG_H, k)
        meas[out, 2] = meas[out, 0] - bf / rng.uniform(4.0, 60.0, k)
        meas[~stereo, 2] = 0.0
        info = np.zeros((n, 9))
        inv = 1.0 / (1.2 ** (2 * level))
        info[:, 0] = info[:, 4] = inv
        info[stereo, 8] = inv[stereo]
        dq = _axis_angle_quat(rng.normal(0, pose_sigma[0], 3))
        q0 = _quat_mul(dq, q)
        if q0[3] < 0:
            q0 = -q0
        q0 /= np.linalg.norm(q0)
        t0 = _quat_rot(dq) @ t + rng.normal(0, pose_sigma[1], 3)
        Ttrue.append(np.concatenate([t, q if q[3] >= 0 else -q])); Tcw.append(np.concatenate([t0, q0]))
        Xs.append(Xw); Ms.append(meas); Ws.append(info); Ss.append(stereo.astype(np.uint8)); Os.append(out)
    cat = lambda a, w: (np.concatenate(a) if a else np.zeros((0,) + w)).reshape((-1,) + w)
    obs_ptr = np.zeros(n_frames + 1, np.int32)
    obs_ptr[1:] = np.cumsum(counts)
    return dict(Tcw=np.array(Tcw).reshape(-1, 7), Tcw_true=np.array(Ttrue).reshape(-1, 7), intr=np.tile(KITTI_INTR5, (n_frames, 1)), obs_ptr=obs_ptr,
                Xw=cat(Xs, (3,)), meas=cat(Ms, (3,)), info=cat(Ws, (9,)), is_stereo=cat(Ss, ()).astype(np.uint8), is_outlier=cat(Os, ()).astype(bool))


def take_frames(batch, idx):
    """The frames `idx` of a batch, in that order, as a batch of their own."""
    idx = [int(i) for i in idx]
    ptr = batch["obs_ptr"]
    sl = [np.arange(ptr[i], ptr[i + 1]) for i in idx]
    sel = np.concatenate(sl).astype(np.int64) if sl else np.zeros(0, np.int64)
    obs_ptr = np.zeros(len(idx) + 1, np.int32)
    obs_ptr[1:] = np.cumsum([len(s) for s in sl])
    out = {k: batch[k][idx] for k in ("Tcw", "Tcw_true", "intr")}
    out.update({k: batch[k][sel] for k in ("Xw", "meas", "info", "is_stereo", "is_outlier")})
    out["obs_ptr"] = obs_ptr
    return out


def concat_batches(batches):
    out = {k: np.concatenate([b[k] for b in batches]) for k in ("Tcw", "Tcw_true", "intr", "Xw", "meas", "info", "is_stereo", "is_outlier")}
    counts = np.concatenate([np.diff(b["obs_ptr"]) for b in batches])
    out["obs_ptr"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return out
