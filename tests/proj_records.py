"""Per-edge records for the mono and stereo projection edges (test infrastructure, not a test file; nothing of the product is imported).

ba_stereo_ref.make_family() gives every edge eye(2) / eye(3), one camera, one bf and one kernel width per class: a record read transposed, from
the neighbour's slot, from the other class's array or from the handle's uniform constants gives the right answer on it.  with_records() returns
the same graph -- vertices, tracks, edge order, starting state -- with every edge carrying a record of its own:

  information   mono s R(t) diag(1, r) R(t)^T, stereo s Q diag(1, r1, r2) Q^T; s = 1.2^(-2 level), level 0 .. 7 (the ORB pyramid), ratios in
                [2, 4] (condition number <= 4), the rotation drawn until the largest off-diagonal entry is >= 0.25 of the largest diagonal one
                (asserted: >= 0.2), symmetrised exactly
  intrinsics    one of three cameras (1-2 % apart, fx != fy in two of them); a stereo edge also one of three bf (10 % apart), drawn independently
  measurement   the edge's own projection of the camera-frame point at the starting state + the error the edge had there before, through
                Graph.errors(): the error vector at the start is unchanged (the family's measurements were drawn at the true state, which the
                dict does not carry; cameras 1-2 % apart move the 3-pixel starting offsets by < 0.1 pixel, inside the 0.5-pixel noise)
  kernel width  one of three per class around sqrt(5.991) / sqrt(7.815), in f["widths"] = (mono, stereo)

Modes (what the host's uniform bookkeeping may and may not take as one record per class):
  per_edge        everything per edge
  uniform_dense   one non-diagonal matrix per class, one camera and one bf for all edges
  mixed_a         mono information uniform, stereo information per edge; one camera; bf per edge
  mixed_b         information uniform in both classes, one camera, bf per edge: the 10-double stereo record is NOT uniform
  mixed_c         one camera per class, another one in each class; mono information per edge, stereo record uniform
The kernel widths differ between neighbours in every mode.
"""
import functools

import numpy as np

import ba_rounds_ref as rr
import ba_stereo_ref as ref

CAMERAS = np.array([[718.856, 718.856, 607.19, 185.22],          # ba_stereo_ref's
                    [726.0446, 711.6674, 613.2619, 183.3678],     # +1 % -1 % +1 % -1 %
                    [707.3543, 729.6388, 598.0822, 188.9244]])    # -1.6 % +1.5 % -1.5 % +2 %
BFS = np.array([386.1448, 351.3918, 424.7593])                    # -9 % +10 % (other baselines: 2 % moved H_pl by 1e-3 on 70 % of the edges only)
WIDTH_FACTORS = np.array([0.8, 1.0, 1.25])
MODES = ("per_edge", "uniform_dense", "mixed_a", "mixed_b", "mixed_c")
MIXED = MODES[2:]

FAMILIES = {
    "dense24": dict(seed=1),                                     # 24 cameras: dense reduced system, the long-track kernel
    "band60": dict(seed=2, long_track=False, n_cams=60),         # banded solve, fused Schur schedule
    "mono24": dict(seed=1, stereo_share=0.0),                    # the kernels' STEREO = false instantiations
}
RECORD_SEED = {"dense24": 11, "band60": 12, "mono24": 13}
# record seeds of the rounds cases: the first of 21, 22, ... at which ba_rounds_ref.assert_comparable holds (tests/test_proj_records_ref.py)
ROUNDS_RECORD_SEED = {"dense24": 21, "band60": 22, "mono24": 21}      # (band60 with 21: one edge 8.6e-5 from its threshold after round 1)


def _rot2(t):
    c, s = np.cos(t), np.sin(t)
    return np.stack([np.stack([c, -s], -1), np.stack([s, c], -1)], -2)


def _offdiag_ratio(M):
    d = M.shape[-1]
    off = np.abs(M * (1 - np.eye(d))).max((-1, -2))
    return off / np.abs(np.einsum("...ii->...i", M)).max(-1)


def dense_information(rng, n, dim, level=None):
    """(n, dim, dim) matrices of the module docstring, dim 2 or 3; level: per matrix, drawn 0 .. 7 when None."""
    level = rng.integers(0, 8, n) if level is None else np.broadcast_to(level, (n,))
    s = 1.2 ** (-2.0 * level)
    M = np.zeros((n, dim, dim))
    todo = np.ones(n, bool)
    while todo.any():
        k = int(todo.sum())
        if dim == 2:
            Q = _rot2(rng.choice([-1.0, 1.0], k) * (np.pi / 4 + rng.uniform(-0.2, 0.2, k)))
        else:
            Q = np.linalg.qr(rng.normal(size=(k, 3, 3)))[0]
        D = np.concatenate([np.ones((k, 1)), rng.uniform(2.0, 4.0, (k, dim - 1))], 1)
        A = s[todo, None, None] * np.einsum("nij,nj,nkj->nik", Q, D, Q)
        A = (A + np.swapaxes(A, 1, 2)) / 2
        ok = _offdiag_ratio(A) >= 0.25
        idx = np.nonzero(todo)[0]
        M[idx[ok]] = A[ok]
        todo[idx[ok]] = False
    return M


def assert_information(M):
    """The generator's own conditions on (n, d, d) matrices: symmetric bit for bit, far from diagonal, condition number <= 4."""
    assert np.array_equal(M, np.swapaxes(M, 1, 2))
    assert np.all(_offdiag_ratio(M) >= 0.2)
    w = np.linalg.eigvalsh(M)
    assert np.all(w[:, 0] > 0) and np.all(w[:, -1] / w[:, 0] <= 4.0 * (1 + 1e-12))


def with_records(f, seed, mode="per_edge"):
    """The make_family() / make_case() dict f with records of the given mode (module docstring).  Adds f["widths"] and f["mode"]."""
    assert mode in MODES
    rng = np.random.default_rng(seed)
    m, s = list(f["mono"]), list(f["stereo"])
    nm, ns = len(m[0]), len(s[0])
    # every draw is made in every mode, so a mode changes what an edge gets and nothing about its neighbours' draws
    info_m, info_s = dense_information(rng, nm, 2), dense_information(rng, ns, 3)
    uni_m, uni_s = dense_information(rng, 1, 2, level=2)[0], dense_information(rng, 1, 3, level=3)[0]
    cam_m, cam_s, bf_s = rng.integers(0, 3, nm), rng.integers(0, 3, ns), rng.integers(0, 3, ns)
    w_m, w_s = rng.integers(0, 3, nm), rng.integers(0, 3, ns)
    if mode in ("uniform_dense", "mixed_a", "mixed_b"):
        info_m = np.tile(uni_m, (nm, 1, 1))
    if mode in ("uniform_dense", "mixed_b", "mixed_c"):
        info_s = np.tile(uni_s, (ns, 1, 1))
    if mode in ("uniform_dense", "mixed_a", "mixed_b"):
        cam_m[:], cam_s[:] = 1, 1
    if mode == "mixed_c":
        cam_m[:], cam_s[:] = 1, 2
    if mode in ("uniform_dense", "mixed_c"):
        bf_s[:] = 2
    assert_information(info_m); assert_information(info_s)
    intr_m = CAMERAS[cam_m]
    intr_s = np.concatenate([CAMERAS[cam_s], BFS[bf_s][:, None]], 1)
    # the measurements: the error at the starting state stays what it was
    e0, _ = ref.graph_of(f).errors()
    z2, z3 = np.zeros((nm, 2)), np.zeros((ns, 3))
    G = ref.Graph(f["cams"], f["cam_fixed"], f["points"], f["pt_fixed"], (m[0], m[1], z2, info_m.reshape(nm, 4), intr_m, None) if nm else None,
                  (s[0], s[1], z3, info_s.reshape(ns, 9), intr_s, None) if ns else None)
    proj = -G.errors()[0]                          # measurement zero: error = -projection
    meas = proj + e0
    m[2], m[3], m[4] = meas[:nm, :2].copy(), info_m.reshape(nm, 4), intr_m
    s[2], s[3], s[4] = meas[nm:].copy(), info_s.reshape(ns, 9), intr_s
    out = dict(f, mono=tuple(m), stereo=tuple(s), mode=mode)
    out["widths"] = (rr.HUB[0] * WIDTH_FACTORS[w_m], rr.HUB[1] * WIDTH_FACTORS[w_s])
    return out


def splice(fa, fb, late_mono, late_stereo):
    """The graph whose edges are fa's where late_* is False, followed per class by fb's where it is True (an appended handle's edge order)."""
    def cat(ta, tb, late, wa, wb):
        return tuple(np.concatenate([np.asarray(a)[~late], np.asarray(b)[late]]) for a, b in zip(ta, tb)), np.concatenate([wa[~late], wb[late]])
    mono, wm = cat(fa["mono"], fb["mono"], late_mono, fa["widths"][0], fb["widths"][0])
    stereo, ws = cat(fa["stereo"], fb["stereo"], late_stereo, fa["widths"][1], fb["widths"][1])
    return dict(fa, mono=mono, stereo=stereo, widths=(wm, ws), mode="spliced")


@functools.lru_cache(maxsize=None)
def family(name, mode="per_edge"):
    """with_records() of FAMILIES[name], once per process and shared: read-only."""
    return with_records(ref.make_family(**FAMILIES[name]), RECORD_SEED[name], mode)


@functools.lru_cache(maxsize=None)
def append_case():
    """(uniform-dense graph, late mono edges, late stereo edges, spliced graph): the 24-camera graph whose edges of cameras 21 .. 23 arrive later
    and carry the per-edge records, the others the uniform-dense ones."""
    fu, fp = family("dense24", "uniform_dense"), family("dense24", "per_edge")
    late_m, late_s = fu["mono"][1] >= 21, fu["stereo"][1] >= 21
    return fu, late_m, late_s, splice(fu, fp, late_m, late_s)


@functools.lru_cache(maxsize=None)
def rounds_case(name, record_seed=None):
    """(ba_rounds_ref.make_case graph with per-edge records and widths, local_ba() of it), once per process and shared: read-only."""
    c = rr.CASES[name]
    f = with_records(rr.make_case(c["seed"], **c["kw"]), ROUNDS_RECORD_SEED[name] if record_seed is None else record_seed)
    return f, rr.local_ba(f, huber=f["widths"])


def huber_share(G):
    """Share of G's edges in the linear part of Huber's function at G's state."""
    return float((G.edge_chi2() > ref.f32(G.delta * G.delta)).mean())


# ---- the mistakes the records must expose (tests/test_proj_records_ref.py applies them to the reference)
def _diag_only(f):
    m, s = list(f["mono"]), list(f["stereo"])
    m[3] = m[3] * np.eye(2).ravel(); s[3] = s[3] * np.eye(3).ravel()
    return dict(f, mono=tuple(m), stereo=tuple(s))


def _successor(f):
    m, s = list(f["mono"]), list(f["stereo"])
    for t in (m, s):
        t[3], t[4] = np.roll(t[3], -1, 0), np.roll(t[4], -1, 0)
    return dict(f, mono=tuple(m), stereo=tuple(s), widths=tuple(np.roll(w, -1) for w in f["widths"]))


def _mono_index_in_stereo_array(f):
    s = list(f["stereo"])
    nm, ns = len(f["mono"][0]), len(s[0])
    assert nm % ns != 0
    k = (np.arange(ns) + nm) % ns
    s[3], s[4] = s[3][k], s[4][k]
    return dict(f, stereo=tuple(s))


def _one_bf(f):
    s = list(f["stereo"])
    s[4] = s[4].copy(); s[4][:, 4] = s[4][0, 4]
    return dict(f, stereo=tuple(s))


def _one_width(f):
    return dict(f, widths=tuple(np.full(len(w), w[0]) if len(w) else w for w in f["widths"]))


MISTAKES = {"diagonal-only information": _diag_only, "record of the successor": _successor, "mono index into the stereo array": _mono_index_in_stereo_array,
            "one bf for all": _one_bf, "one width for all": _one_width}


# ---- the pose-only batch
POSE_COUNTS = (0, 1, 3, 63, 64, 65, 128, 129)      # lane l owns observations l, l + 64, ...
POSE_SEED = 71                                     # the first of 71, 72, ... whose every frame meets tests/test_pose_only_gpu.py's conditions


def pose_batch(synth_pose, seed, start, n_random=40):
    """A synth_pose batch (the module is passed in: nothing of the product is imported here) of POSE_COUNTS + n_random counts up to 400, half
    of the observations stereo, with dense information per observation: a stereo one the 3 x 3 of dense_information, a mono one the 2 x 2 in
    entries 0 1 3 4 and zeros elsewhere."""
    rng = np.random.default_rng(seed)
    counts = list(POSE_COUNTS) + [int(c) for c in rng.integers(2, 401, n_random)]
    b = synth_pose.synth_pose_batch(len(counts), counts, 0.5, 0.1, seed, pose_sigma=start)
    st = b["is_stereo"].astype(bool)
    n = len(st)
    W = np.zeros((n, 3, 3))
    W[st] = dense_information(rng, int(st.sum()), 3)
    W[~st, :2, :2] = dense_information(rng, int((~st).sum()), 2)
    assert_information(W[st]); assert_information(W[~st, :2, :2])
    b["info"] = W.reshape(n, 9)
    return b
