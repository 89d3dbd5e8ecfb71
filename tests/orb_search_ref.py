"""The numpy statement of the guided ORB matcher (cube_slam_wu_amd/csrc/cs_orb_search.h, whose top comment it follows line by line), in
float64 or in long double: the same level table, the same grid, the same order of tests, every sum left to right, and the walk of step 7
as written -- cell columns outermost, cell rows inside, the keypoints of a cell in ascending index, a strict < for the best distance.
Steps 1 to 6 are vectorised over the queries of a batch; the walk is a loop over queries and cell columns.  Nothing here is fused.  run()
returns the inspection quantities beside the outcome, and every threshold comparison it made with the difference each one decided on.

Not recorded as comparisons: the floor and ceil of the window's cell bounds.  They decide nothing: a keypoint with |d| < radius lies in a
cell whose index is floor(y + 0.5) with y within rounding of the bounds' own arguments, half a cell away from where floor(y') or ceil(y')
could exclude it; the bounds only spare the walk the cells that hold no such keypoint.  The keypoints' own cells ARE recorded (they decide
the walk order and who is off the grid)."""
import numpy as np

OK, SKIPPED, BEHIND, OUT_OF_IMAGE, OUT_OF_RANGE, VIEW_ANGLE, NO_CANDIDATE, TOO_FAR = range(8)
STATUS_NAMES = ("OK", "SKIPPED", "BEHIND", "OUT_OF_IMAGE", "OUT_OF_RANGE", "VIEW_ANGLE", "NO_CANDIDATE", "TOO_FAR")
CHECK_VIEW, CHECK_REPROJ = 1, 2
LEVEL_NONE = 255
PARAM_KEYS = ("min_dist_factor", "max_dist_factor", "view_cos", "chi2_mono", "chi2_stereo", "grid_cols", "grid_rows")
INSPECT = ("u", "v", "ur", "dist", "radius")
INTEGER_OUT = ("status", "best_idx", "best_dist", "level", "n_window", "n_candidates")
_POP = np.array([bin(i).count("1") for i in range(256)], np.int64)


def params(**kw):
    p = dict(min_dist_factor=0.8, max_dist_factor=1.2, view_cos=0.5, chi2_mono=5.99, chi2_stereo=7.8, grid_cols=64, grid_rows=48)
    p.update(kw)
    return p


def rotation(pose8, dt):
    """R (n, 3, 3) of the quaternions of poses (n, 8): x y z qx qy qz qw s."""
    T = np.asarray(pose8, np.float64).astype(dt)
    n = np.sqrt(T[:, 3] * T[:, 3] + T[:, 4] * T[:, 4] + T[:, 5] * T[:, 5] + T[:, 6] * T[:, 6])
    x, y, z, w = T[:, 3] / n, T[:, 4] / n, T[:, 5] / n, T[:, 6] / n
    one, two = dt(1), dt(2)
    R = np.empty((len(T), 3, 3), dt)
    R[:, 0, 0] = one - two * (y * y + z * z); R[:, 0, 1] = two * (x * y - w * z); R[:, 0, 2] = two * (x * z + w * y)
    R[:, 1, 0] = two * (x * y + w * z); R[:, 1, 1] = one - two * (x * x + z * z); R[:, 1, 2] = two * (y * z - w * x)
    R[:, 2, 0] = two * (x * z - w * y); R[:, 2, 1] = two * (y * z + w * x); R[:, 2, 2] = one - two * (x * x + y * y)
    return R


def hamming(a32, b32):
    """a32 (32) against b32 (n, 32) bytes -> (n)"""
    return _POP[np.bitwise_xor(np.asarray(b32, np.uint8), np.asarray(a32, np.uint8)[None, :])].sum(axis=1)


def frame_tables(batch, prm, dt):
    """Per frame: the level table, the grid constants, every keypoint's cell (-1: in no cell) with the quantity that decided it, the sorted
    order and the cell starts."""
    cols, rows = int(prm["grid_cols"]), int(prm["grid_rows"])
    out = []
    for f in range(len(batch["cam"])):
        a, b = int(batch["kp_ptr"][f]), int(batch["kp_ptr"][f + 1])
        bounds = np.asarray(batch["bounds"][f], np.float64).astype(dt)
        sf, nl = dt(batch["scale_factor"][f]), int(batch["n_levels"][f])
        scale = [dt(1)]
        for _ in range(1, nl):
            scale.append(scale[-1] * sf)
        scale = np.array(scale, dt)
        inv_w, inv_h = dt(cols) / (bounds[1] - bounds[0]), dt(rows) / (bounds[3] - bounds[2])
        kp = np.asarray(batch["kp"][a:b], np.float64).astype(dt).reshape(b - a, 3)
        ax = (kp[:, 0] - bounds[0]) * inv_w + dt(0.5)
        ay = (kp[:, 1] - bounds[2]) * inv_h + dt(0.5)
        cx, cy = np.floor(ax), np.floor(ay)
        inside = (cx >= 0) & (cx <= cols - 1) & (cy >= 0) & (cy <= rows - 1)
        cell = np.where(inside, cx * rows + cy, -1).astype(np.int64)
        order = np.array([i for i in np.argsort(cell, kind="stable") if cell[i] >= 0], np.int64)
        start = np.searchsorted(cell[order], np.arange(cols * rows + 1), side="left")
        out.append(dict(first=a, kp=kp, octave=np.asarray(batch["octave"][a:b], np.int64), desc=np.asarray(batch["desc"][a:b], np.uint8).reshape(b - a, 32), bounds=bounds,
                        cam=np.asarray(batch["cam"][f], np.float64).astype(dt), scale=scale, inv_sigma2=dt(1) / (scale * scale), inv_w=inv_w, inv_h=inv_h, n_levels=nl,
                        cell=cell, cell_arg=(ax, ay), cell_floor=(cx, cy), order=order, start=start))
    return out


def _cell_range(x, radius, inv, n, dt):
    a, b = np.floor((x - radius) * inv), np.ceil((x + radius) * inv)
    top = dt(n - 1)
    c0 = a if a > 0 else dt(0)
    c1 = b if b < top else top
    lo = int(c0) if c0 <= top else n
    hi = int(c1) if c1 >= 0 else -1
    return lo, hi, lo < n and hi >= 0


def run(batch, prm=None, dt=np.float64):
    """-> dict over the batch's Q queries: status, best_idx, best_dist, level, n_window, n_candidates, u, v, ur, dist, radius, per job n_ok;
    `comparisons`: a list of (name, key (m, 2) int, diff (m)) -- every threshold comparison of the statement, for which (query, keypoint
    or level or -1) it was made, and lhs - rhs as it was computed; `cells`: per frame the keypoints' cells."""
    prm = params() if prm is None else prm
    dt = np.dtype(dt).type
    cols, rows = int(prm["grid_cols"]), int(prm["grid_rows"])
    FT = frame_tables(batch, prm, dt)
    ptr = np.asarray(batch["query_ptr"])
    nj, Q = len(ptr) - 1, int(ptr[-1])
    jq = np.repeat(np.arange(nj), np.diff(ptr))
    fj = np.asarray(batch["frame_of_job"], np.int64)
    pose = np.asarray(batch["pose8"], np.float64).astype(dt).reshape(nj, 8)
    R, t, s = rotation(batch["pose8"], dt)[jq], pose[jq, :3], pose[jq, 7]
    th, flags = np.asarray(batch["th"], np.float64).astype(dt)[jq], np.asarray(batch["flags"], np.int64)[jq]
    max_hamming = np.asarray(batch["max_hamming"], np.int64)[jq]
    fq = fj[jq]
    cam = np.array([FT[f]["cam"] for f in fq], dt).reshape(Q, 5)
    bounds = np.array([FT[f]["bounds"] for f in fq], dt).reshape(Q, 4)
    X = np.asarray(batch["X"], np.float64).astype(dt).reshape(Q, 3)
    nrm = np.asarray(batch["normal"], np.float64).astype(dt).reshape(Q, 3)
    dr = np.asarray(batch["dist_range"], np.float64).astype(dt).reshape(Q, 2)
    skip = np.asarray(batch["skip"]).astype(bool).reshape(Q)
    qdesc = np.asarray(batch["qdesc"], np.uint8).reshape(Q, 32)
    allq = np.arange(Q)
    comparisons = []

    def record(name, made, diff, second=-1):
        idx = np.flatnonzero(made)
        comparisons.append((name, np.stack([idx, np.full(len(idx), second)], 1), np.asarray(diff)[idx]))

    with np.errstate(all="ignore"):
        Xc = np.stack([s * (R[:, i, 0] * X[:, 0] + R[:, i, 1] * X[:, 1] + R[:, i, 2] * X[:, 2]) + t[:, i] for i in range(3)], axis=1)
        front = ~skip & (Xc[:, 2] > 0)
        record("Xc2 > 0", ~skip, Xc[:, 2])
        u = cam[:, 0] * Xc[:, 0] / Xc[:, 2] + cam[:, 2]
        v = cam[:, 1] * Xc[:, 1] / Xc[:, 2] + cam[:, 3]
        inside = front & (u >= bounds[:, 0]) & (u < bounds[:, 1]) & (v >= bounds[:, 2]) & (v < bounds[:, 3])
        for name, d in (("u >= min_x", u - bounds[:, 0]), ("u < max_x", u - bounds[:, 1]), ("v >= min_y", v - bounds[:, 2]), ("v < max_y", v - bounds[:, 3])):
            record(name, front, d)
        ur = u - cam[:, 4] / Xc[:, 2]
        dist = np.sqrt(Xc[:, 0] * Xc[:, 0] + Xc[:, 1] * Xc[:, 1] + Xc[:, 2] * Xc[:, 2])
        lo, hi = dist < dt(prm["min_dist_factor"]) * dr[:, 0], dist > dt(prm["max_dist_factor"]) * dr[:, 1]
        record("dist < min_dist_factor min_distance", inside, dist - dt(prm["min_dist_factor"]) * dr[:, 0])
        record("dist > max_dist_factor max_distance", inside & ~lo, dist - dt(prm["max_dist_factor"]) * dr[:, 1])
        in_range = inside & ~lo & ~hi
        Rn = np.stack([R[:, i, 0] * nrm[:, 0] + R[:, i, 1] * nrm[:, 1] + R[:, i, 2] * nrm[:, 2] for i in range(3)], axis=1)
        dot = Xc[:, 0] * Rn[:, 0] + Xc[:, 1] * Rn[:, 1] + Xc[:, 2] * Rn[:, 2]
        view = (flags & CHECK_VIEW) != 0
        bad_view = view & (dot < dt(prm["view_cos"]) * dist)
        record("Xc . R normal < view_cos dist", in_range & view, dot - dt(prm["view_cos"]) * dist)
        walk = in_range & ~bad_view
        ratio = dr[:, 1] / dist
    level = np.full(Q, LEVEL_NONE, np.int64)
    radius = np.zeros(Q, dt)
    for f in np.unique(fq[walk]):
        sel = walk & (fq == f)
        sc = FT[f]["scale"]
        lv = np.zeros(Q, np.int64)
        for l in range(FT[f]["n_levels"] - 1):
            with np.errstate(all="ignore"):
                lv += (sc[l] < ratio) & sel
            record("scale[l] < ratio", sel, sc[l] - ratio, l)
        level[sel] = lv[sel]
        radius[sel] = th[sel] * sc[lv[sel]]

    status = np.full(Q, OK, np.int64)
    for cond, code in ((bad_view & in_range, VIEW_ANGLE), (inside & (lo | hi), OUT_OF_RANGE), (front & ~inside, OUT_OF_IMAGE), (~skip & ~front, BEHIND), (skip, SKIPPED)):
        status[cond] = code
    best_idx, best_dist = np.full(Q, -1, np.int64), np.full(Q, -1, np.int64)
    n_window, n_candidates = np.zeros(Q, np.int64), np.zeros(Q, np.int64)
    kp_cmp = {"|du| < radius": ([], []), "|dv| < radius": ([], []), "e2 inv_sigma2 <= chi2": ([], [])}
    chi2_mono, chi2_stereo = dt(prm["chi2_mono"]), dt(prm["chi2_stereo"])
    for q in allq[walk]:
        F = FT[fq[q]]
        cx0, cx1, any_x = _cell_range(u[q] - F["bounds"][0], radius[q], F["inv_w"], cols, dt)
        cy0, cy1, any_y = _cell_range(v[q] - F["bounds"][2], radius[q], F["inv_h"], rows, dt)
        best, bd = -1, 257
        if any_x and any_y:
            for cx in range(cx0, cx1 + 1):
                ks = F["order"][F["start"][cx * rows + cy0]:F["start"][cx * rows + cy1 + 1]]      # one cell column of the window is one run
                if not len(ks):
                    continue
                kp, octv = F["kp"][ks], F["octave"][ks]
                du, dv = kp[:, 0] - u[q], kp[:, 1] - v[q]
                in_u = np.abs(du) < radius[q]
                in_w = in_u & (np.abs(dv) < radius[q])
                kp_cmp["|du| < radius"][0].append(np.stack([np.full(len(ks), q), ks], 1)); kp_cmp["|du| < radius"][1].append(np.abs(du) - radius[q])
                kp_cmp["|dv| < radius"][0].append(np.stack([np.full(in_u.sum(), q), ks[in_u]], 1)); kp_cmp["|dv| < radius"][1].append((np.abs(dv) - radius[q])[in_u])
                n_window[q] += int(in_w.sum())
                cand = in_w & (octv >= level[q] - 1) & (octv <= level[q])
                if flags[q] & CHECK_REPROJ:
                    stereo = kp[:, 2] >= 0
                    drr = ur[q] - kp[:, 2]
                    e2m = du * du + dv * dv
                    e2 = np.where(stereo, e2m + drr * drr, e2m)
                    d = e2 * F["inv_sigma2"][octv] - np.where(stereo, chi2_stereo, chi2_mono)
                    kp_cmp["e2 inv_sigma2 <= chi2"][0].append(np.stack([np.full(cand.sum(), q), ks[cand]], 1)); kp_cmp["e2 inv_sigma2 <= chi2"][1].append(d[cand])
                    cand = cand & (d <= 0)
                n_candidates[q] += int(cand.sum())
                if cand.any():
                    hd = hamming(qdesc[q], F["desc"][ks[cand]])
                    k = int(np.argmin(hd))                       # (the first of equals)
                    if hd[k] < bd:                               # (strict: of equals the first in walk order stays)
                        bd, best = int(hd[k]), int(ks[cand][k])
        if best < 0:
            status[q] = NO_CANDIDATE
        else:
            best_idx[q], best_dist[q] = best, bd
            status[q] = TOO_FAR if bd > max_hamming[q] else OK
    for name, (keys, diffs) in kp_cmp.items():
        comparisons.append((name, np.concatenate(keys) if keys else np.zeros((0, 2), np.int64), np.concatenate(diffs) if diffs else np.zeros(0, dt)))
    z = dt(0)
    computed = front                                               # u and v exist from step 3 on, ur and dist behind its test, the radius from step 6 on
    return dict(status=status, best_idx=best_idx, best_dist=best_dist, level=level, n_window=n_window, n_candidates=n_candidates,
                u=np.where(computed, u, z), v=np.where(computed, v, z), ur=np.where(inside, ur, z), dist=np.where(inside, dist, z), radius=np.where(walk, radius, z),
                n_ok=np.array([int((status[ptr[j]:ptr[j + 1]] == OK).sum()) for j in range(nj)], np.int64), comparisons=comparisons,
                cells=[F["cell"] for F in FT], cell_args=[F["cell_arg"] for F in FT], cell_floors=[F["cell_floor"] for F in FT], job_of_query=jq)


def mutual(best12, status12, best21, status21):
    """SearchBySim3's agreement: match12[i] = j iff i -> j is OK and j -> i is OK, otherwise -1."""
    out = np.full(len(best12), -1, np.int64)
    for i, j in enumerate(best12):
        if status12[i] == OK and 0 <= j < len(best21) and status21[j] == OK and best21[j] == i:
            out[i] = j
    return out


def brute_force_nearest(batch, q, radius, u, v):
    """Over ALL keypoints of query q's frame, on or off the grid, whatever their octave: the index (in the frame) of the nearest descriptor
    among those with |du| < radius and |dv| < radius, and its distance."""
    f = int(batch["frame_of_job"][np.searchsorted(batch["query_ptr"], q, side="right") - 1])
    a, b = int(batch["kp_ptr"][f]), int(batch["kp_ptr"][f + 1])
    kp = np.asarray(batch["kp"][a:b], np.float64)
    inw = np.flatnonzero((np.abs(kp[:, 0] - u) < radius) & (np.abs(kp[:, 1] - v) < radius))
    hd = hamming(batch["qdesc"][q], np.asarray(batch["desc"][a:b])[inw])
    k = int(np.argmin(hd))
    return int(inw[k]), int(hd[k])
