"""Seeded synthetic batches for the guided ORB matcher (capi.OrbSearch / cs_orb_search_jobs).

A batch is what ORBmatcher::Fuse and ORBmatcher::SearchBySim3 see: keyframes with KITTI-shaped cameras (1241 x 376, fx = fy = 718.856,
stereo baseline 0.537 m, scale factor 1.2, 8 levels) observing one shared point cloud, and jobs (a keyframe, a similarity, th,
max_hamming, flags) that each project some of the cloud's points into their keyframe.  A point has a 256-bit descriptor, a viewing
direction and a distance range [max_distance / 1.2^7, max_distance]; a keyframe's keypoint of a point lies at the noisy projection, at the
octave MapPoint::PredictScale predicts from the keyframe's distance (or one below it), with the point's descriptor.  Clutter keypoints
with random descriptors fill a keyframe up.  What a query meets depends on its family, a function of (frame, point) -- FAMILY_CYCLE:
  good      the point's descriptor with 0 .. 30 flipped bits: OK
  far       60 .. 90 flipped bits: TOO_FAR under TH_LOW = 50, OK under TH_HIGH = 100
  skip      the skip byte set: SKIPPED
  behind    a point behind the camera: BEHIND
  outside   a point in front whose projection misses the image: OUT_OF_IMAGE
  range     a distance range the keyframe's distance is outside of: OUT_OF_RANGE
  view      the viewing direction reversed: VIEW_ANGLE under CHECK_VIEW, OK otherwise
  level     the keypoint sits two octaves off the predicted level: NO_CANDIDATE
  reproj    the keypoint is 2.7 px (times its octave's scale) off the projection: inside the window, outside the chi2 gate:
            NO_CANDIDATE under CHECK_REPROJ, OK otherwise
  alone     the keyframe has no keypoint of the point: NO_CANDIDATE (unless clutter happens to fall into the window)

plant_job adds hand-placed cases (_plant) to one job (tests/orb_search_cases.py: the crowded batch): two candidates at EQUAL Hamming
distance in different cell columns, in different rows of one column, and within one cell -- the winner is the first in walk order, which
in the first two is the one with the LARGER index in the frame; within one cell the walk order is the index order itself -- and keypoints
whose rounded cell falls outside the grid (ORB-SLAM2 assigns cells by rounding to nearest, so a strip half a cell wide along the right and
bottom border is in no cell): such a keypoint carries exactly the query's descriptor and is matched by nobody."""
from __future__ import annotations

import numpy as np

from .synth_triangulate import CX, CY, FX, FY, HEIGHT, SCALE_FACTOR, STEREO_B, WIDTH, _pose7, _rot

N_LEVELS = 8
CHECK_VIEW, CHECK_REPROJ = 1, 2
FUSE, FUSE_SIM3, SEARCH_BY_SIM3 = CHECK_VIEW | CHECK_REPROJ, CHECK_VIEW, 0
TH_LOW, TH_HIGH = 50, 100
FAMILIES = ("good", "far", "skip", "behind", "outside", "range", "view", "level", "reproj", "alone", "planted")
FAMILY_CYCLE = ("good", "far", "good", "skip", "good", "behind", "good", "outside", "good", "range", "good", "view", "good", "level", "good", "reproj", "good", "alone")

FRAME_KEYS = ("cam", "bounds", "scale_factor", "n_levels")
KP_KEYS = ("kp", "octave", "desc", "kp_point")
JOB_KEYS = ("frame_of_job", "pose8", "th", "max_hamming", "flags")
QUERY_KEYS = ("X", "normal", "dist_range", "qdesc", "skip", "family", "truth", "point_of_query")


def level_table(scale_factor=SCALE_FACTOR, n_levels=N_LEVELS):
    s = [1.0]
    for _ in range(1, n_levels):
        s.append(s[-1] * scale_factor)
    return np.array(s)


def predict_level(max_distance, dist, scale):
    """The smallest l with scale[l] >= max_distance / dist, at most len(scale) - 1."""
    return int(np.sum(scale[:-1] < max_distance / dist))


def flip_bits(rng, desc32, k, avoid=()):
    """desc32 (32 bytes) with k bits flipped, none of them in `avoid`; -> (the new descriptor, the flipped bit positions)."""
    free = np.setdiff1d(np.arange(256), np.asarray(avoid, int))
    bits = rng.choice(free, int(k), replace=False)
    out = np.array(desc32, np.uint8, copy=True)
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out, bits


def _camera(rng, spread=1.0):
    """A camera near the origin that looks along +z: (Rwc, C)."""
    Rwc = _rot([0, 1, 0], rng.uniform(-0.08, 0.08)) @ _rot(rng.normal(size=3), rng.uniform(0, 0.04))
    return Rwc, rng.uniform(-1, 1, 3) * [spread, 0.1 * spread, 0.5 * spread]


def _back_project(Rwc, C, u, v, z):
    return C + Rwc @ (z * np.array([(u - CX) / FX, (v - CY) / FY, 1.0]))


def _to_camera(Rwc, C, X):
    return (np.asarray(X) - C) @ Rwc


def _keypoint(rng, u, v, z, stereo, noise_px):
    """u v ur with noise; ur = -1 without a right-image coordinate"""
    u, v = u + rng.normal(0, noise_px), v + rng.normal(0, noise_px)
    ur = -1.0
    if stereo and 0 < z < 40 * STEREO_B:
        r = u - FX * STEREO_B / z + rng.normal(0, noise_px)
        if r >= 0:
            ur = r
    return [u, v, ur]


def _cam_row(stereo):
    return [FX, FY, CX, CY, FX * STEREO_B if stereo else 0.0]


def frame_observing(points, pose7, seed=0, stereo=True, noise_px=0.4, desc=None, max_distance=None, keep=None):
    """A target keyframe built from given world points (n, 3): a keypoint at the noisy projection of every point in front of the camera and
    inside the image (and, with `keep`, only of those points), at the octave PredictScale gives for max_distance (n; without it a random
    one), with the point's descriptor desc (n, 32; without it a random one).  pose7: world-to-camera, x y z qx qy qz qw.
    -> a one-frame dict (kp_ptr, kp, octave, desc, cam, bounds, scale_factor, n_levels) with kp_point (per keypoint, the point's index) and
    kp_of_point (n, -1: not observed)."""
    rng = np.random.default_rng([int(seed), 0x0b5e])
    points = np.asarray(points, float).reshape(-1, 3)
    T = np.asarray(pose7, float)
    q = T[3:7] / np.linalg.norm(T[3:7])
    x, y, z, w = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    scale = level_table()
    kp, octave, dd, kp_point = [], [], [], []
    kp_of_point = np.full(len(points), -1, np.int64)
    for i, X in enumerate(points):
        if keep is not None and not keep[i]:
            continue
        pc = R @ X + T[:3]
        if pc[2] <= 0.1:
            continue
        u, v = FX * pc[0] / pc[2] + CX, FY * pc[1] / pc[2] + CY
        if not (2 <= u < WIDTH - 2 and 2 <= v < HEIGHT - 2):
            continue
        kp_of_point[i] = len(kp)
        kp.append(_keypoint(rng, u, v, pc[2], stereo, noise_px))
        octave.append(predict_level(max_distance[i], np.linalg.norm(pc), scale) if max_distance is not None else int(rng.integers(0, 4)))
        dd.append(desc[i] if desc is not None else rng.integers(0, 256, 32))
        kp_point.append(i)
    n = len(kp)
    return dict(kp_ptr=np.array([0, n], np.int32), kp=np.array(kp, float).reshape(n, 3), octave=np.array(octave, np.int32), desc=np.array(dd, np.uint8).reshape(n, 32),
                cam=np.array([_cam_row(stereo)]), bounds=np.array([[0.0, WIDTH, 0.0, HEIGHT]]), scale_factor=np.array([SCALE_FACTOR]), n_levels=np.array([N_LEVELS], np.int32),
                kp_point=np.array(kp_point, np.int64), kp_of_point=kp_of_point)


def synth_orb_search(frame_keypoints, jobs, seed=0, n_points=400, stereo=None, noise_px=0.4, grid=(64, 48), families=None, plant_job=None):
    """frame_keypoints: per frame the number of keypoints it is to have (observations of the cloud first, then clutter).  jobs: a list of
    dicts frame, count, flags, th, max_hamming (and optionally s, the similarity's scale: the job then searches the cloud scaled by 1 / s).
    stereo: per frame 0 / 1 (default f % 2 == 0).  plant_job: the job that gets the planted ties and off-grid keypoints (its frame too).
    -> dict of arrays: the frames (kp_ptr, kp, octave, desc, cam, bounds, scale_factor, n_levels), the jobs (frame_of_job, pose8, th,
    max_hamming, flags, query_ptr, X, normal, dist_range, qdesc, skip), and for tests grid, kp_point (per keypoint the cloud point, -1:
    clutter or planted), family, truth (per query the index in the frame of the point's own keypoint, -1: none), point_of_query, ties
    (rows: query, winner, loser, kind 0 columns / 1 rows / 2 one cell) and offgrid (rows: query, the off-grid keypoint, the decoy)."""
    rng = np.random.default_rng([int(seed), 0x0fb5])
    cycle = FAMILY_CYCLE if families is None else tuple(families)
    scale = level_table()
    n_frames = len(frame_keypoints)
    # the cloud, seen from a reference camera at the origin
    P = int(n_points)
    uv = np.stack([rng.uniform(20, WIDTH - 20, P), rng.uniform(15, HEIGHT - 15, P)], 1)
    depth = rng.uniform(5, 30, P)
    Xw = np.array([_back_project(np.eye(3), np.zeros(3), uv[i, 0], uv[i, 1], depth[i]) for i in range(P)]).reshape(P, 3)
    d_ref = np.linalg.norm(Xw, axis=1)
    normal = Xw / d_ref[:, None]
    max_d = d_ref * scale[rng.integers(0, 5, P)] * rng.uniform(0.86, 0.98, P)
    pdesc = rng.integers(0, 256, (P, 32)).astype(np.uint8)

    cams, frames = [], []
    for f in range(n_frames):
        st = bool(stereo[f]) if stereo is not None else f % 2 == 0
        Rwc, C = _camera(rng)
        cams.append((Rwc, C, st))
        rows = []                                                # [u v ur] octave desc point
        for p in range(P):
            if len(rows) >= -(-int(frame_keypoints[f]) * 3 // 4):      # three quarters, rounded up
                break
            fam = cycle[(p + 3 * f) % len(cycle)]
            if fam in ("alone", "behind", "outside"):
                continue
            pc = _to_camera(Rwc, C, Xw[p])
            u, v = FX * pc[0] / pc[2] + CX, FY * pc[1] / pc[2] + CY
            if not (2 <= u < WIDTH - 2 and 2 <= v < HEIGHT - 2):
                continue
            lvl = predict_level(max_d[p], np.linalg.norm(pc), scale)
            octv = lvl - 1 if (lvl > 0 and p % 3 == 0) else lvl
            k = _keypoint(rng, u, v, pc[2], st, noise_px)
            if fam == "level":
                octv = lvl + 1 if lvl + 1 < N_LEVELS else lvl - 2
            elif fam == "reproj":
                k = _keypoint(rng, u + 2.7 * scale[octv] * rng.choice([-1.0, 1.0]), v, pc[2], st, 0.0)
            rows.append((k, octv, pdesc[p], p))
        while len(rows) < int(frame_keypoints[f]):               # clutter
            rows.append(([rng.uniform(0, WIDTH), rng.uniform(0, HEIGHT), -1.0], int(rng.integers(0, N_LEVELS)), rng.integers(0, 256, 32).astype(np.uint8), -1))
        order = rng.permutation(len(rows))                       # (a keypoint's index says nothing about where it lies)
        frames.append([rows[i] for i in order])

    out = {k: [] for k in JOB_KEYS + QUERY_KEYS}
    counts, ties, offgrid = [], [], []
    for j, job in enumerate(jobs):
        f = int(job["frame"])
        Rwc, C, st = cams[f]
        s = float(job.get("s", 1.0))
        flags = int(job["flags"])
        pose7 = _pose7(Rwc, C)
        out["frame_of_job"].append(f); out["pose8"].append(np.concatenate([pose7, [s]])); out["th"].append(float(job["th"]))
        out["max_hamming"].append(int(job["max_hamming"])); out["flags"].append(flags)
        kp_of_point = {r[3]: i for i, r in enumerate(frames[f]) if r[3] >= 0}
        n_q = 0

        def add(X, nrm, dmax, qd, skip, fam, truth, p):
            # (with a similarity of scale s the job's map lives in a frame scaled by 1 / s: Xc = s R (X / s) + t)
            out["X"].append(np.asarray(X) / s); out["normal"].append(nrm); out["dist_range"].append([dmax / scale[-1], dmax]); out["qdesc"].append(qd)
            out["skip"].append(skip); out["family"].append(FAMILIES.index(fam)); out["truth"].append(truth); out["point_of_query"].append(p)

        if plant_job is not None and j == int(plant_job):
            n_q += _plant(rng, frames[f], cams[f], grid, float(job["th"]), scale, len(out["X"]), add, ties, offgrid)
        picks = rng.permutation(P)[:max(0, int(job["count"]) - n_q)]
        for p in picks:
            fam = cycle[(p + 3 * f) % len(cycle)]
            X, nrm, dmax, skip = Xw[p], normal[p], max_d[p], 0
            qd, _ = flip_bits(rng, pdesc[p], rng.integers(60, 91) if fam == "far" else rng.integers(0, 31))
            if fam == "skip":
                skip = 1
            elif fam == "behind":
                X = _back_project(Rwc, C, rng.uniform(100, WIDTH - 100), rng.uniform(50, HEIGHT - 50), -rng.uniform(2, 20))
            elif fam == "outside":
                side = rng.integers(0, 4)
                u = (-rng.uniform(5, 300), WIDTH + rng.uniform(5, 300), rng.uniform(0, WIDTH), rng.uniform(0, WIDTH))[side]
                v = (rng.uniform(0, HEIGHT), rng.uniform(0, HEIGHT), -rng.uniform(5, 200), HEIGHT + rng.uniform(5, 200))[side]
                X = _back_project(Rwc, C, u, v, rng.uniform(5, 30))
            elif fam == "range":
                dist = np.linalg.norm(_to_camera(Rwc, C, X))
                dmax = dist / rng.uniform(1.3, 2.0) if p % 2 else dist * scale[-1] / rng.uniform(0.4, 0.75)
            elif fam == "view":
                nrm = -nrm
            add(X, nrm, dmax, qd, skip, fam, kp_of_point.get(p, -1), p)
        counts.append(int(job["count"]) if int(job["count"]) >= n_q else n_q)
        assert len(out["X"]) == sum(counts)

    b = dict(grid=np.array(grid, np.int32))
    b["kp_ptr"] = np.concatenate([[0], np.cumsum([len(fr) for fr in frames])]).astype(np.int32)
    N = int(b["kp_ptr"][-1])
    b["kp"] = np.array([r[0] for fr in frames for r in fr], float).reshape(N, 3)
    b["octave"] = np.array([r[1] for fr in frames for r in fr], np.int32)
    b["desc"] = np.array([r[2] for fr in frames for r in fr], np.uint8).reshape(N, 32)
    b["kp_point"] = np.array([r[3] for fr in frames for r in fr], np.int64)
    b["cam"] = np.array([_cam_row(c[2]) for c in cams], float).reshape(n_frames, 5)
    b["bounds"] = np.tile([0.0, WIDTH, 0.0, HEIGHT], (n_frames, 1)).astype(float)
    b["scale_factor"], b["n_levels"] = np.full(n_frames, SCALE_FACTOR), np.full(n_frames, N_LEVELS, np.int32)
    Q, J = len(out["X"]), len(jobs)
    b["frame_of_job"], b["pose8"], b["th"] = np.array(out["frame_of_job"], np.int32), np.array(out["pose8"], float).reshape(J, 8), np.array(out["th"], float)
    b["max_hamming"], b["flags"] = np.array(out["max_hamming"], np.int32), np.array(out["flags"], np.int32)
    b["query_ptr"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    b["X"], b["normal"], b["dist_range"] = np.array(out["X"], float).reshape(Q, 3), np.array(out["normal"], float).reshape(Q, 3), np.array(out["dist_range"], float).reshape(Q, 2)
    b["qdesc"], b["skip"] = np.array(out["qdesc"], np.uint8).reshape(Q, 32), np.array(out["skip"], np.uint8)
    b["family"], b["truth"], b["point_of_query"] = np.array(out["family"], np.int32), np.array(out["truth"], np.int64), np.array(out["point_of_query"], np.int64)
    b["ties"], b["offgrid"] = np.array(ties, np.int64).reshape(-1, 4), np.array(offgrid, np.int64).reshape(-1, 3)
    b["cloud"] = dict(X=Xw, normal=normal, max_distance=max_d, desc=pdesc)
    b["frame_pose7"] = np.array([_pose7(c[0], c[1]) for c in cams], float).reshape(n_frames, 7)
    return b


def two_directions(frame_keypoints, seed=0, th=7.5, max_hamming=TH_HIGH, grid=(64, 48), flags=SEARCH_BY_SIM3):
    """ORBmatcher::SearchBySim3's two searches over two keyframes of one cloud: job 0 projects the points of keyframe 0's keypoints into
    keyframe 1 -- query i belongs to keypoint i of keyframe 0, and a keypoint without a point is a skipped query -- and job 1 the points of
    keyframe 1's keypoints into keyframe 0.  truth: the index in the searched keyframe of the point's keypoint there, -1: none."""
    assert len(frame_keypoints) == 2
    b = synth_orb_search(frame_keypoints, (), seed, grid=grid, stereo=(0, 0))
    rng = np.random.default_rng([int(seed), 0x2d1c])
    cloud, scale = b["cloud"], level_table()
    out = {k: [] for k in QUERY_KEYS}
    counts = []
    for src, dst in ((0, 1), (1, 0)):
        a, e = frame_slices(b, src)
        da, de = frame_slices(b, dst)
        there = {int(p): k for k, p in enumerate(b["kp_point"][da:de]) if p >= 0}
        for i in range(a, e):
            p = int(b["kp_point"][i])
            if p < 0:
                row = ([0.0, 0.0, 10.0], [0.0, 0.0, 1.0], [1.0, 2.0], b["desc"][i], 1, "skip", -1, -1)
            else:
                row = (cloud["X"][p], cloud["normal"][p], [cloud["max_distance"][p] / scale[-1], cloud["max_distance"][p]], flip_bits(rng, b["desc"][i], rng.integers(0, 11))[0], 0,
                       "good", there.get(p, -1), p)
            for k, v in zip(QUERY_KEYS, row):
                out[k].append(FAMILIES.index(v) if k == "family" else v)
        counts.append(e - a)
    Q = sum(counts)
    b["frame_of_job"], b["pose8"] = np.array([1, 0], np.int32), np.concatenate([b["frame_pose7"][[1, 0]], np.ones((2, 1))], axis=1)
    b["th"], b["max_hamming"], b["flags"] = np.full(2, float(th)), np.full(2, int(max_hamming), np.int32), np.full(2, int(flags), np.int32)
    b["query_ptr"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    b["X"], b["normal"], b["dist_range"] = np.array(out["X"], float).reshape(Q, 3), np.array(out["normal"], float).reshape(Q, 3), np.array(out["dist_range"], float).reshape(Q, 2)
    b["qdesc"], b["skip"] = np.array(out["qdesc"], np.uint8).reshape(Q, 32), np.array(out["skip"], np.uint8)
    b["family"], b["truth"], b["point_of_query"] = np.array(out["family"], np.int32), np.array(out["truth"], np.int64), np.array(out["point_of_query"], np.int64)
    return b


def _plant(rng, rows, cam, grid, th, scale, q0, add, ties, offgrid):
    """The planted queries of one job, with their keypoints appended to the frame's rows.  -> how many queries were added."""
    Rwc, C, st = cam
    cols, nrows = int(grid[0]), int(grid[1])
    cw, chh = WIDTH / cols, HEIGHT / nrows                     # a cell covers [(c - 0.5) cw, (c + 0.5) cw): cells are assigned by rounding to nearest
    L = 1
    radius = th * scale[L]
    assert cols >= 3 and nrows >= 3 and radius > 35 and radius < 0.45 * min(cw, chh)
    n = 0

    def query(u0, v0):
        X = _back_project(Rwc, C, u0, v0, 12.0)
        dist = np.linalg.norm(_to_camera(Rwc, C, X))
        qd = rng.integers(0, 256, 32).astype(np.uint8)
        add(X, (X - C) / np.linalg.norm(X - C), dist * scale[L] * 0.93, qd, 0, "planted", -1, -1)
        return qd

    def keypoint(u, v, d):
        rows.append(([u, v, -1.0], L, d, -1))
        return len(rows) - 1

    # equal distances: A is first in walk order and B was appended first (the smaller index) -- except within one cell
    for kind, (u0, v0, da, db) in enumerate((((2 - 0.5) * cw + 1.0, 1 * chh, (-12.0, 0.0), (12.0, 0.0)),        # two cell columns
                                             (2 * cw, (1 - 0.5) * chh + 1.0, (0.0, -12.0), (0.0, 12.0)),        # two rows of one column
                                             (1 * cw, 2 * chh, (-5.0, 0.0), (5.0, 0.0)))):                      # one cell
        qd = query(u0, v0)
        desc_a, bits = flip_bits(rng, qd, 12)
        desc_b, _ = flip_bits(rng, qd, 12, avoid=bits)
        if kind == 2:
            a = keypoint(u0 + da[0], v0 + da[1], desc_a); b = keypoint(u0 + db[0], v0 + db[1], desc_b)
        else:
            b = keypoint(u0 + db[0], v0 + db[1], desc_b); a = keypoint(u0 + da[0], v0 + da[1], desc_a)
        ties.append([q0 + n, a, b, kind])
        n += 1
    # off the grid: the keypoint with the query's own descriptor rounds to column `cols` (to row `nrows`); a decoy 20 bits away is in a cell
    for u0, v0, dt, dd in (((cols - 0.5) * cw + 20.0, 1 * chh, (2.0, 0.0), (-30.0, 0.0)), (1.5 * cw + 40.0, (nrows - 0.5) * chh + 17.0, (0.0, 2.0), (0.0, -30.0))):
        qd = query(u0, v0)
        t = keypoint(u0 + dt[0], v0 + dt[1], qd.copy())
        d = keypoint(u0 + dd[0], v0 + dd[1], flip_bits(rng, qd, 20)[0])
        offgrid.append([q0 + n, t, d])
        n += 1
    return n


def frame_slices(batch, f):
    a, b = int(batch["kp_ptr"][f]), int(batch["kp_ptr"][f + 1])
    return a, b


def take_jobs(batch, idx):
    """The jobs `idx` of a batch, in that order, over the same frames, as a batch of their own (ties and offgrid are dropped)."""
    idx = [int(i) for i in idx]
    ptr = batch["query_ptr"]
    sl = [np.arange(ptr[i], ptr[i + 1]) for i in idx]
    sel = np.concatenate(sl).astype(np.int64) if sl else np.zeros(0, np.int64)
    out = {k: batch[k] for k in FRAME_KEYS + KP_KEYS + ("kp_ptr", "grid")}
    out.update({k: batch[k][idx] for k in JOB_KEYS})
    out.update({k: batch[k][sel] for k in QUERY_KEYS})
    query_ptr = np.zeros(len(idx) + 1, np.int32)
    query_ptr[1:] = np.cumsum([len(s) for s in sl])
    out["query_ptr"] = query_ptr
    return out


def take_frames(batch, idx):
    """The frames `idx` of a batch with the jobs that search them (in their order, frame indices renumbered)."""
    idx = [int(i) for i in idx]
    new = {f: k for k, f in enumerate(idx)}
    jobs = [j for j, f in enumerate(batch["frame_of_job"]) if int(f) in new]
    out = take_jobs(batch, jobs)
    out["frame_of_job"] = np.array([new[int(f)] for f in out["frame_of_job"]], np.int32)
    sl = [np.arange(*frame_slices(batch, f)) for f in idx]
    sel = np.concatenate(sl).astype(np.int64) if sl else np.zeros(0, np.int64)
    out.update({k: batch[k][idx] for k in FRAME_KEYS})
    out.update({k: batch[k][sel] for k in KP_KEYS})
    out["kp_ptr"] = np.concatenate([[0], np.cumsum([len(s) for s in sl])]).astype(np.int32)
    return out


def concat(batches):
    """Frames after frames, jobs after jobs (all with one grid)."""
    assert all(np.array_equal(b["grid"], batches[0]["grid"]) for b in batches)
    out = {k: np.concatenate([b[k] for b in batches]) for k in FRAME_KEYS + KP_KEYS + JOB_KEYS + QUERY_KEYS if k != "frame_of_job"}
    first = np.cumsum([0] + [len(b["cam"]) for b in batches])
    out["frame_of_job"] = np.concatenate([b["frame_of_job"] + first[i] for i, b in enumerate(batches)]).astype(np.int32)
    out["kp_ptr"] = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(b["kp_ptr"]) for b in batches]))]).astype(np.int32)
    out["query_ptr"] = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(b["query_ptr"]) for b in batches]))]).astype(np.int32)
    out["grid"] = batches[0]["grid"]
    return out


def job_of_query(batch):
    return np.repeat(np.arange(len(batch["query_ptr"]) - 1), np.diff(batch["query_ptr"]))


def desc_words(desc32):
    """(n, 32) bytes -> (n, 8) little-endian words, as the kernel holds them."""
    return np.ascontiguousarray(np.asarray(desc32, np.uint8).reshape(-1, 32)).view("<u4").reshape(-1, 8)


def write_dump(path, batch, params):
    """The batch as the text dump tools/hostonly/orb_search_host_check.cpp reads (every double in %.17g).  params: min_dist_factor,
    max_dist_factor, view_cos, chi2_mono, chi2_stereo, grid_cols, grid_rows."""
    nf, N, nj, Q = len(batch["cam"]), int(batch["kp_ptr"][-1]), len(batch["frame_of_job"]), int(batch["query_ptr"][-1])
    g = lambda v: " ".join("%.17g" % float(x) for x in np.ravel(v))
    w = lambda v: " ".join("%d" % int(x) for x in np.ravel(v))
    kw, qw = desc_words(batch["desc"]), desc_words(batch["qdesc"])
    with open(path, "w") as f:
        f.write("%d %d %d %d\n%s %d %d\n" % (nf, N, nj, Q, g(params[:5]), int(params[5]), int(params[6])))
        for i in range(nf):
            f.write("%s %s %s %d %d %d\n" % (g(batch["cam"][i]), g(batch["bounds"][i]), g(batch["scale_factor"][i]), int(batch["n_levels"][i]), int(batch["kp_ptr"][i]), int(batch["kp_ptr"][i + 1])))
        for k in range(N):
            f.write("%s %d %s\n" % (g(batch["kp"][k]), int(batch["octave"][k]), w(kw[k])))
        for j in range(nj):
            f.write("%d %s %s %d %d %d %d\n" % (int(batch["frame_of_job"][j]), g(batch["pose8"][j]), g(batch["th"][j]), int(batch["max_hamming"][j]), int(batch["flags"][j]),
                                                int(batch["query_ptr"][j]), int(batch["query_ptr"][j + 1])))
        for q in range(Q):
            f.write("%s %s %s %d %s\n" % (g(batch["X"][q]), g(batch["normal"][q]), g(batch["dist_range"][q]), int(batch["skip"][q]), w(qw[q])))
