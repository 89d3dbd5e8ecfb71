"""Seeded synthetic batches for the two-view triangulation of new map points (capi.Triangulate / cs_triangulate_pairs).

A batch is what LocalMapping::CreateNewMapPoints sees after its matcher: pairs (current keyframe, neighbour) with KITTI-shaped cameras
(1241 x 376, fx = fy = 718.856, stereo baseline 0.537 m) and, per pair, matched keypoints.  Pairs come in the four sensor combinations
mono-mono, stereo-mono, mono-stereo, stereo-stereo (SENSORS, pair f has combination f % 4 unless told otherwise) and move sideways or
forward in turn ((f // 4) % 2): a forward pair sees less parallax between the keyframes than a stereo rig's own baseline gives, which is
when CreateNewMapPoints back-projects a stereo keypoint instead of triangulating.  Matches come in families, interleaved match by match
(FAMILY_CYCLE), so that any 64 consecutive matches hold several routes and statuses:
  good          a point 3 .. 20 m away, both keypoints with 0.5 px noise, the same octave
  distant       150 .. 400 m away: no parallax to speak of and, as in ORB-SLAM2, no stereo depth
  along         a mismatch ALONG the epipolar line: another depth on the same ray of camera 1, past the ray's vanishing point (a point
                behind the cameras), or, in a forward pair, a point between the two cameras (in front of 1, behind 2)
  off           a mismatch OFF the epipolar line by 7 px (octaves 3 and 1: the error gate of side 2 is the tighter one) or by 10 .. 40 px
  octave        a good match whose octaves are four levels apart
  close         1.5 .. 4 m away; close_spoiled: the same with a right-image coordinate that is 6 .. 15 px off

A stereo camera's keypoint has ur = u - bf / z + noise and depth = bf / (u - ur); past 40 baselines, or where ur would be negative, it
has neither (ur = depth = -1), and a mono camera's keypoints never have them.  median_depth2 is the median depth of the pair's points in
camera 2 for a mono-mono pair (the monocular rule) and -1 otherwise (the stereo rule)."""
from __future__ import annotations

import numpy as np

FX, FY, CX, CY, STEREO_B = 718.856, 718.856, 607.1928, 185.2157, 0.5371657
WIDTH, HEIGHT = 1241, 376
SCALE_FACTOR = 1.2
SENSORS = ((0, 0), (1, 0), (0, 1), (1, 1))      # (camera 1 is stereo, camera 2 is stereo)
FAMILIES = ("good", "distant", "along", "off", "octave", "close", "close_spoiled")
FAMILY_CYCLE = ("good", "distant", "good", "along", "good", "off", "good", "octave", "close", "close_spoiled")

PAIR_KEYS = ("Tcw1", "Tcw2", "cam1", "cam2", "median_depth2", "sensor", "forward")
MATCH_KEYS = ("kp1", "kp2", "family")


def _rot(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def _quat(R):
    """qx qy qz qw of a rotation matrix."""
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    x = np.sqrt(max(0.0, 1 + R[0, 0] - R[1, 1] - R[2, 2])) / 2
    y = np.sqrt(max(0.0, 1 - R[0, 0] + R[1, 1] - R[2, 2])) / 2
    z = np.sqrt(max(0.0, 1 - R[0, 0] - R[1, 1] + R[2, 2])) / 2
    return np.array([np.copysign(x, R[2, 1] - R[1, 2]), np.copysign(y, R[0, 2] - R[2, 0]), np.copysign(z, R[1, 0] - R[0, 1]), w])


def _pose7(Rwc, C):
    """World-to-camera, SE3Quat::toVector order, of a camera with orientation Rwc at C."""
    R = Rwc.T
    return np.concatenate([-R @ C, _quat(R)])


def _project(Rwc, C, X):
    pc = (X - C) @ Rwc
    return np.array([FX * pc[0] / pc[2] + CX, FY * pc[1] / pc[2] + CY]), pc[2]


def _keypoint(rng, uv, z, stereo, octave, noise_px, spoil=0.0):
    """u v ur depth sigma2 scale"""
    scale = SCALE_FACTOR ** octave
    u, v = uv + rng.normal(0, noise_px, 2)
    ur, depth = -1.0, -1.0
    if stereo and 0 < z < 40 * STEREO_B:
        r = u - FX * STEREO_B / z + rng.normal(0, noise_px)
        if r >= 0 and u - r > 0:
            ur, depth = r + spoil, FX * STEREO_B / (u - r)
    return [u, v, ur, depth, scale * scale, scale]


def synth_triangulate(n_pairs, n_matches, seed=0, sensors=None, forward=None, baselines=None, noise_px=0.5, families=None):
    """n_pairs pairs; n_matches: one count or one per pair.  sensors: per pair an index into SENSORS (default f % 4); forward: per pair 0 / 1
    (default (f // 4) % 2); baselines: per pair the distance between the keyframes (default 0.6 .. 1.5 m); families: the cycle of match
    families (default FAMILY_CYCLE).  -> dict of arrays: Tcw1, Tcw2 (n, 7), cam1, cam2 (n, 6), median_depth2 (n), match_ptr (n + 1),
    kp1, kp2 (N, 6), and for tests sensor, forward (n) and family (N, an index into FAMILIES)."""
    rng = np.random.default_rng([int(seed), 0x7219])
    counts = [int(n_matches)] * n_pairs if np.isscalar(n_matches) else [int(c) for c in n_matches]
    assert len(counts) == n_pairs
    cycle = FAMILY_CYCLE if families is None else tuple(families)
    out = {k: [] for k in PAIR_KEYS + MATCH_KEYS}
    for f in range(n_pairs):
        s = int(sensors[f]) if sensors is not None else f % 4
        fwd = int(forward[f]) if forward is not None else (f // 4) % 2
        st1, st2 = SENSORS[s]
        B = float(baselines[f]) if baselines is not None else rng.uniform(0.6, 1.5)
        Rwc1 = _rot([0, 1, 0], rng.uniform(-np.pi, np.pi)) @ _rot(rng.normal(size=3), rng.uniform(0, 0.05))
        C1 = rng.uniform(-50, 50, 3) * [1, 0.05, 1]
        d = np.array([rng.uniform(-0.2, 0.2), rng.uniform(-0.05, 0.05), 1.0]) if fwd else np.array([rng.choice([-1.0, 1.0]), rng.uniform(-0.05, 0.05), rng.uniform(-0.3, 0.3)])
        C2 = C1 + Rwc1 @ (B * d / np.linalg.norm(d))
        Rwc2 = Rwc1 @ _rot(rng.normal(size=3), rng.uniform(0, 0.06))
        depths2 = []
        for i in range(counts[f]):
            fam = cycle[i % len(cycle)]
            rep = i // len(cycle)
            uv1 = np.array([rng.uniform(50, WIDTH - 50), rng.uniform(30, HEIGHT - 30)])
            z1 = rng.uniform(150, 400) if fam == "distant" else rng.uniform(1.5, 4) if fam in ("close", "close_spoiled") else rng.uniform(3, 20)
            ray = Rwc1 @ np.array([(uv1[0] - CX) / FX, (uv1[1] - CY) / FY, 1.0])
            X = C1 + z1 * ray
            uv2, z2 = _project(Rwc2, C2, X)
            o1 = int(rng.integers(0, 4))
            o2 = o1
            spoil1 = spoil2 = 0.0
            if fam == "along":
                if rep % 3 == 2 and fwd:                          # between the cameras: in front of 1, behind 2
                    z1w = rng.uniform(0.2, 0.6) * B
                    uv2, z2 = _project(Rwc2, C2, C1 + z1w * ray)
                elif rep % 3 == 1:                                # past the vanishing point of camera 1's ray
                    inf = _project(Rwc2, np.zeros(3), ray)[0]
                    uv2 = inf + (inf - uv2) * rng.uniform(0.5, 3.0)
                else:                                             # another depth on the ray
                    uv2, z2 = _project(Rwc2, C2, C1 + z1 * rng.choice([rng.uniform(0.25, 0.6), rng.uniform(2, 5)]) * ray)
            elif fam == "off":
                e = _project(Rwc2, C2, C1 + 2 * z1 * ray)[0] - uv2
                perp = np.array([-e[1], e[0]]) / np.linalg.norm(e)
                if rep % 2 == 0:
                    o1, o2 = 3, 1
                    uv2 = uv2 + perp * 7.0 * rng.choice([-1.0, 1.0])
                else:
                    uv2 = uv2 + perp * rng.uniform(10, 40) * rng.choice([-1.0, 1.0])
            elif fam == "octave":
                o1, o2 = (0, 4) if rep % 2 == 0 else (4, 0)
            elif fam == "close_spoiled":
                if st1 and (rep % 2 == 0 or not st2):
                    spoil1 = rng.uniform(6, 15)
                else:
                    spoil2 = rng.uniform(6, 15)
            k1 = _keypoint(rng, uv1, z1, st1, o1, noise_px, spoil1)
            k2 = _keypoint(rng, uv2, z2, st2, o2, noise_px, spoil2)
            if fam == "close" and st1 and st2 and rep % 2 == 1:    # a stereo keyframe's keypoint without a depth: side 2's is what is left
                k1[2] = k1[3] = -1.0
            out["kp1"].append(k1); out["kp2"].append(k2); out["family"].append(FAMILIES.index(fam))
            depths2.append(z2)
        out["Tcw1"].append(_pose7(Rwc1, C1)); out["Tcw2"].append(_pose7(Rwc2, C2))
        out["cam1"].append([FX, FY, CX, CY, FX * STEREO_B if st1 else 0.0, STEREO_B if st1 else 0.0])
        out["cam2"].append([FX, FY, CX, CY, FX * STEREO_B if st2 else 0.0, STEREO_B if st2 else 0.0])
        pos = [z for z in depths2 if z > 0]
        out["median_depth2"].append(float(np.median(pos)) if (s == 0 and pos) else (10.0 if s == 0 else -1.0))
        out["sensor"].append(s); out["forward"].append(fwd)
    b = {k: np.array(out[k], float).reshape(n_pairs, -1) for k in ("Tcw1", "Tcw2", "cam1", "cam2")}
    b["median_depth2"] = np.array(out["median_depth2"], float)
    b["sensor"], b["forward"] = np.array(out["sensor"], np.int32), np.array(out["forward"], np.int32)
    b["kp1"], b["kp2"] = np.array(out["kp1"], float).reshape(-1, 6), np.array(out["kp2"], float).reshape(-1, 6)
    b["family"] = np.array(out["family"], np.int32)
    b["match_ptr"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    return b


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


def pair_of_match(batch):
    """(N) the pair each match belongs to."""
    return np.repeat(np.arange(len(batch["match_ptr"]) - 1), np.diff(batch["match_ptr"]))


def keep_accepted(batch, result):
    """What CreateNewMapPoints makes MapPoints of: the matches with status OK.  -> dict: index (into the batch's matches), pair, X (k, 3),
    normal (k, 3), min_distance, max_distance, kp1, kp2 (k, 6)."""
    ok = np.flatnonzero(np.asarray(result["status"]) == 0)
    return dict(index=ok, pair=pair_of_match(batch)[ok], X=np.asarray(result["X"])[ok], normal=np.asarray(result["normal"])[ok],
                min_distance=np.asarray(result["min_distance"])[ok], max_distance=np.asarray(result["max_distance"])[ok], kp1=batch["kp1"][ok], kp2=batch["kp2"][ok])


def write_dump(path, batch, params):
    """The batch as the text dump tools/hostonly/triangulate_host_check.cpp reads (every double in %.17g).  params: the six parameters in
    cs_triangulate_params' order."""
    n, N = len(batch["Tcw1"]), int(batch["match_ptr"][-1])
    g = lambda v: " ".join("%.17g" % float(x) for x in np.ravel(v))
    with open(path, "w") as f:
        f.write("%d %d\n%s\n" % (n, N, g(params)))
        for i in range(n):
            f.write("%s %s %s %s %s %d %d\n" % (g(batch["Tcw1"][i]), g(batch["Tcw2"][i]), g(batch["cam1"][i]), g(batch["cam2"][i]), g(batch["median_depth2"][i]),
                                                int(batch["match_ptr"][i]), int(batch["match_ptr"][i + 1])))
        for m in range(N):
            f.write("%s %s\n" % (g(batch["kp1"][m]), g(batch["kp2"][m])))
