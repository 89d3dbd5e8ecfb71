"""The graphs tests/test_pgo_ref.py and tests/test_pgo_gpu.py share, and their reference runs (tests/pgo_ref.py), each computed once.

Trajectory graphs (synth_pgo.ring, n = 16), with the iteration counts at which the float64 reference still decides every trial by more
than rounding (|rho| > 1e-6, asserted in test_pgo_ref.py) -- measured on the reference alone, float64 against long double:
  fixscale   fix_scale on every vertex, no scale noise, measurement noise 2e-3 rad / 1e-2 m, start drift 0.003 rad / 0.015 m per step (a
             larger drift makes the chi2 after the first step sensitive: 5e-6 .. 7e-6 between the two precisions at 0.01 rad / 0.05 m).
             rho per iteration 0.99, 5.7e-3, 2.9e-6, 1.5e-9 with the computed lambda, 0.99, 2.3e-3, 6e-9 with lambda 1e-16: 2 iterations.
  free       free scale, measurement noise 0.03 rad / 0.05 m / 0.02, start drift 0.01 rad / 0.05 m / 1 % per step.  rho 1.0, 0.61, 1.6e-4,
             1.1e-7 (computed) and 1.0, 0.64, 3.7e-5, 5.5e-9 (1e-16): 3 iterations.
  far        the same noise, start drift 0.12 rad / 0.4 m / 3 % per step.  rho 0.96, 1.0, 0.67, 4.6e-5 and 0.96, 1.0, 0.61, 3.2e-5: 4 iterations.
  rejected   `fixscale` without fix_scale: the second linearisation runs through sim3.h:192's branch (|sigma| >= eps, small rotation; 551
             of its 580 evaluations of log), H loses rank and the second iteration rejects five trials (rho -4.3, -3.4, -2.3, -0.52,
             -0.024) before it accepts one (0.063).  2 iterations, computed lambda.
  layout     n = 70, see layout_graph().
  <name>_w   the graph <name> with dense information on every edge (edge_information, INFO_SEED): fixscale_w (computed lambda, 2
             iterations), free_w (lambda 1e-16, 3), layout_w (both, 3).  Their optima lie 8e-3 .. 9e-2 from the unweighted ones.  Not
             used: free_w with the computed lambda (its third iteration evaluates log 31 times in sim3.h:192's branch and takes 5
             trials) and far_w (lambda 1e-16: chi2 differs by 5.03e-6 between the two precisions, above rule (d)'s 5e-6; computed
             lambda: 32 evaluations in that branch, 8 trials).
  mesh       121 keyframes on an 11 x 11 lattice, 320 weighted edges, see mesh_graph(): the one graph whose sparse plan keeps a dense
             tail.  2 iterations, both lambdas: trials [1, 1], rho 0.96.  (With vertex 0 alone fixed the gauge is nearly free and the
             two precisions disagree by 9e-6 after one iteration with lambda 1e-16, 2.4e-5 after two; hence the five fixed vertices.)"""
import functools

import numpy as np

from cube_slam_wu_amd import synth_pgo
import pgo_ref

RING = {
    "fixscale": dict(noise_rot=2e-3, noise_trans=1e-2, noise_scale=0.0, drift_rot=0.003, drift_trans=0.015, drift_scale=0.0, fix_scale=True),
    "free": dict(),
    "far": dict(drift_rot=0.12, drift_trans=0.4, drift_scale=0.03),
    "rejected": dict(noise_rot=2e-3, noise_trans=1e-2, noise_scale=0.0, drift_rot=0.003, drift_trans=0.015, drift_scale=0.0, fix_scale=False),
}
SEED = 2
# (graph, user lambda) -> iterations
TRAJECTORIES = {("fixscale", 0.0): 2, ("fixscale", 1e-16): 2, ("free", 0.0): 3, ("free", 1e-16): 3, ("far", 0.0): 4, ("far", 1e-16): 4}
REJECTED = ("rejected", 0.0, 2)
LAYOUT_ITERATIONS = 3
# the same graphs with edge_information(.., INFO_SEED) on every edge ("<name>_w"); (graph, user lambda) -> iterations.  Left out: free_w
# with the computed lambda (its third iteration runs through sim3.h:192's branch and rejects trials) and far_w (rule (d)).
INFO_SEED = 11
WEIGHTED_TRAJECTORIES = {("fixscale_w", 0.0): 2, ("free_w", 1e-16): 3}
WEIGHTED_LAYOUT = ("layout_w", LAYOUT_ITERATIONS)
BIGROT = ("bigrot", 1e-16, 2)      # not one of all_runs(): its second trial has rho 1.8e-7 (see test_pgo_ref.py)


def _noisy(rng, true, i, j, r, t, s):
    u = np.concatenate([r * rng.standard_normal(3), t * rng.standard_normal(3), [s * rng.standard_normal()]])
    return synth_pgo.mul(synth_pgo.exp(u), synth_pgo.mul(true[j], synth_pgo.inv(true[i])))


@functools.lru_cache(maxsize=None)
def layout_graph():
    """n = 70: an odd edge count, a hub of degree 40 (vertex 10), three fixed vertices (0, 33, 34: the ring edge 33 -> 34 joins two fixed
    ones), a vertex without edges (20), fix_scale on every third vertex."""
    n, hub, lonely = 70, 10, 20
    g = synth_pgo.ring(n, 7)
    rng = np.random.default_rng(77)
    true = g["sim8_true"]
    pairs, meas = [], []
    for i, j, m in zip(g["vi"], g["vj"], g["meas8"]):
        if lonely not in (i, j):
            pairs.append((int(i), int(j))); meas.append(m)

    def add(i, j):
        pairs.append((i, j)); meas.append(_noisy(rng, true, i, j, 0.03, 0.05, 0.02))

    add(lonely - 1, lonely + 1)
    have = {(min(p), max(p)) for p in pairs}
    degree = lambda v: sum(v in p for p in pairs)
    for v in range(n):
        if degree(hub) >= 40:
            break
        w = (hub + 5 + 3 * v) % n
        if w not in (hub, lonely) and (min(hub, w), max(hub, w)) not in have:
            have.add((min(hub, w), max(hub, w)))
            add(w, hub) if v % 2 else add(hub, w)
    assert degree(hub) == 40 and degree(lonely) == 0
    if len(pairs) % 2 == 0:
        add(40, 50)
    assert len(pairs) % 2 == 1 and len({(min(p), max(p)) for p in pairs}) == len(pairs)
    fixed = np.zeros(n, np.uint8)
    fixed[[0, 33, 34]] = 1
    fix_scale = (np.arange(n) % 3 == 0).astype(np.uint8)
    return dict(sim8=g["sim8"], fixed=fixed, fix_scale=fix_scale, vi=np.array([p[0] for p in pairs], np.int32), vj=np.array([p[1] for p in pairs], np.int32),
                meas8=np.stack(meas), info49=None)


@functools.lru_cache(maxsize=None)
def bigrot_graph():
    """Four fixed / free pairs whose free vertex starts 2.6 rad off about x, y, z and (1, 1, 1): the first step's exp(update) is the one
    place where Quaterniond(R) leaves its trace branch (cs_pgo_linearize_edges only ever sees exp of a 1e-9 step); a fifth pair 0.5 rad off."""
    rng = np.random.default_rng(9)
    sim8, vi, vj, meas, fixed = [], [], [], [], []
    for ax, th in (((1, 0, 0), 2.6), ((0, 1, 0), 2.6), ((0, 0, 1), 2.6), ((1, 1, 1), 2.6), ((1, -1, 0.5), 0.5)):
        Sa, Sb = _state(rng, 1.0), _state(rng, 1.3)
        off = np.concatenate([_axis_angle(ax, th), 0.1 * rng.standard_normal(3), [1.05]])
        vi.append(len(sim8)); sim8.append(Sa); fixed.append(1)
        vj.append(len(sim8)); sim8.append(synth_pgo.mul(off, Sb)); fixed.append(0)
        meas.append(synth_pgo.mul(Sb, synth_pgo.inv(Sa)))
    return dict(sim8=np.stack(sim8), fixed=np.array(fixed, np.uint8), fix_scale=np.zeros(len(sim8), np.uint8), vi=np.array(vi, np.int32), vj=np.array(vj, np.int32),
                meas8=np.stack(meas), info49=None)


def edge_information(n, seed, skew_every=0):
    """(n, 49): per edge Q diag(w) Q^T, Q from the QR of a seeded 7 x 7 normal matrix, w = 10 ** U(-1, 1.5) per axis, symmetrised exactly
    (0.5 (M + M^T)); another matrix for every edge.  skew_every = m > 0: every m-th edge (k % m == 1) also gets a seeded skew part of the
    matrix's own size -- an ASYMMETRIC Omega, for the per-edge products of test_edge_terms alone (cubeslam_hip.h: never a trajectory)."""
    rng = np.random.default_rng(seed)
    out = np.empty((n, 7, 7))
    for k in range(n):
        Q, _ = np.linalg.qr(rng.standard_normal((7, 7)))
        w = 10.0 ** rng.uniform(-1.0, 1.5, 7)
        M = (Q * w) @ Q.T
        out[k] = 0.5 * (M + M.T)
        if skew_every and k % skew_every == 1:
            A = rng.standard_normal((7, 7))
            out[k] += 0.25 * np.abs(w).max() * (A - A.T)
    return out.reshape(n, 49)


def _weighted(g, seed):
    return dict(g, info49=edge_information(len(g["vi"]), seed))


MESH_SIDE, MESH_SEED, MESH_INFO_SEED, MESH_ITERATIONS = 11, 3, 21, 2
MESH_FIXED = (0, MESH_SIDE - 1, MESH_SIDE * (MESH_SIDE - 1), MESH_SIDE * MESH_SIDE - 1, (MESH_SIDE * MESH_SIDE) // 2)


@functools.lru_cache(maxsize=None)
def mesh_graph():
    """An 11 x 11 lattice of keyframes (vertex y * 11 + x), 121 vertices and 320 edges: right and down (from the even-parity end of x + y
    to the odd one, so the orientation alternates) and along one diagonal; measurement noise 0.03 rad / 0.05 m / 0.02, the start the truth
    perturbed by 0.01 rad / 0.05 m / 1 % per vertex, fix_scale on v % 5 == 2, the four corners and the centre fixed (at the truth), dense
    information on every edge.  More than PGO_REDUCE_T = 256 edges and unknowns, and a graph whose elimination ends in a near-clique: the
    sparse plan keeps a dense tail (tests/test_pgo_plan_cpu.py asserts it from the host-only plan)."""
    w = MESH_SIDE
    n = w * w
    rng = np.random.default_rng(MESH_SEED)
    true = np.zeros((n, 8))
    for v in range(n):
        x, y = v % w, v // w
        Swc = synth_pgo.exp(np.concatenate([0.25 * rng.standard_normal(3) + [0.0, 0.0, 0.2 * (x - y)], np.zeros(4)]))
        Swc[4:7] = [1.5 * x, 1.5 * y, 0.3 * np.sin(0.7 * x + 0.4 * y)]
        true[v] = synth_pgo.inv(Swc)
    pairs = []
    for y in range(w):
        for x in range(w):
            v = y * w + x
            for dx, dy in ((1, 0), (0, 1)):
                if x + dx < w and y + dy < w:
                    u = (y + dy) * w + x + dx
                    pairs.append((v, u) if (x + y) % 2 == 0 else (u, v))
            if x + 1 < w and y + 1 < w:
                pairs.append((v, v + w + 1))
    assert len(pairs) == 320 and len({(min(p), max(p)) for p in pairs}) == 320
    meas = np.stack([_noisy(rng, true, i, j, 0.03, 0.05, 0.02) for i, j in pairs])
    fixed = np.zeros(n, np.uint8)
    fixed[list(MESH_FIXED)] = 1
    start = true.copy()
    for v in range(n):
        if not fixed[v]:
            u = np.concatenate([0.01 * rng.standard_normal(3), 0.05 * rng.standard_normal(3), [0.01 * rng.standard_normal()]])
            start[v] = synth_pgo.mul(synth_pgo.exp(u), true[v])
    fix_scale = (np.arange(n) % 5 == 2).astype(np.uint8)
    return dict(sim8=start, fixed=fixed, fix_scale=fix_scale, vi=np.array([p[0] for p in pairs], np.int32), vj=np.array([p[1] for p in pairs], np.int32),
                meas8=meas, info49=edge_information(len(pairs), MESH_INFO_SEED))


@functools.lru_cache(maxsize=None)
def graph(name):
    if name.endswith("_w"):                     # the same graph with dense information on every edge
        return _weighted(graph(name[:-2]), INFO_SEED)
    if name == "mesh":
        return mesh_graph()
    return layout_graph() if name == "layout" else (bigrot_graph() if name == "bigrot" else synth_pgo.ring(16, SEED, **RING[name]))


def make_ref(g, dtype=np.float64, lam=0.0):
    G = pgo_ref.Graph(g["sim8"], g["fixed"], g["fix_scale"], g["vi"], g["vj"], g["meas8"], g.get("info49"), dtype=dtype)
    G.user_lambda_init = lam
    return G


@functools.lru_cache(maxsize=None)
def ref_run(name, lam, iterations, long_double=False):
    """The reference after optimize(iterations): the Graph, with .done."""
    G = make_ref(graph(name), np.longdouble if long_double else np.float64, lam)
    G.done = G.optimize(iterations)
    return G


def weighted_runs():
    """(weighted graph, user lambda, iterations) of every run with dense information that has an unweighted twin."""
    return [(k[0], k[1], it) for k, it in WEIGHTED_TRAJECTORIES.items()] + [(WEIGHTED_LAYOUT[0], lam, WEIGHTED_LAYOUT[1]) for lam in (0.0, 1e-16)]


def mesh_runs():
    return [("mesh", 0.0, MESH_ITERATIONS), ("mesh", 1e-16, MESH_ITERATIONS)]


def all_runs():
    return ([(k[0], k[1], it) for k, it in TRAJECTORIES.items()] + [REJECTED, ("layout", 0.0, LAYOUT_ITERATIONS), ("layout", 1e-16, LAYOUT_ITERATIONS)] +
            weighted_runs() + mesh_runs())


@functools.lru_cache(maxsize=None)
def mesh_factorisation_deviation():
    """The mesh's state after ONE iteration's step (computed lambda), from three float64 factorisations of the reference's H + lambda I:
    pgo_ref.cholesky_solve, numpy's LAPACK solve, and cholesky_solve of the system in reversed vertex order.  Returns the larger state
    deviation of the last two from the first: what factorisation rounding alone does to the states, the yardstick of the back ends' test."""
    G = make_ref(mesh_graph())
    H, b, _ = G.build_system()
    A = H + 1e-5 * np.abs(np.diag(H)).max() * np.eye(G.n)
    rev = np.arange(G.n).reshape(-1, 7)[::-1].ravel()
    x_rev = np.zeros(G.n)
    x_rev[rev] = pgo_ref.cholesky_solve(A[np.ix_(rev, rev)], b[rev])
    start, states = G.est.copy(), []
    for x in (pgo_ref.cholesky_solve(A, b), np.linalg.solve(A, b), x_rev):
        G.est = start.copy()
        G.update(x)
        states.append(G.est.copy())
    return max(pgo_ref.state_deviation(states[1], states[0]), pgo_ref.state_deviation(states[2], states[0]))


# ---- hand-placed edges for the block test ------------------------------------------------------------------------------------------
def _axis_angle(axis, th):
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    return np.concatenate([np.sin(0.5 * th) * a, [np.cos(0.5 * th)]])


def _state(rng, scale):
    return np.concatenate([_axis_angle(rng.standard_normal(3), rng.uniform(0.2, 2.5)), rng.uniform(-3, 3, 3), [scale]])


@functools.lru_cache(maxsize=None)
def edge_block_case():
    """One pair of vertices per edge; the measurement is chosen so that the edge's error C S_i S_j^-1 is a given Sim(3).
    Returns the graph and, per edge, its group: 'quirk' (sim3.h:192's branch: W nearly rank one), 'near_pi' (the error's rotation 1e-3
    short of pi: log divides by sqrt(1 - d^2) ~ 1e-3, and a central difference over 2e-9 of that is rounding noise of order one in
    any precision) or 'regular'.  A tolerance derived from the reference's own deviation is derived per group."""
    rng = np.random.default_rng(5)
    gen = (1.0, -0.7, 0.4)
    # (axis, angle, sigma): the four branches of log -- |sigma| < 1e-5 or not, d > 1 - 1e-5 (angle < 4.47e-3) or not
    targets = [((1, 0, 0), 0.0, 0.0)]                                                              # replaced by the exactly zero error below
    targets += [(gen, th, sg) for th in (0.0, 1e-6, 2e-3, 4e-3) for sg in (0.0, 3e-6)]             # small sigma, small rotation
    targets += [(gen, th, sg) for th in (5e-3, 0.3, 1.5, 2.5) for sg in (0.0, -3e-6)]              # small sigma, rotation
    targets += [(gen, th, sg) for th in (0.0, 1e-4, 3e-3) for sg in (2e-5, -1e-3, 0.05, 0.5)]      # sigma, small rotation: the kept branch
    targets += [(gen, th, sg) for th in (5e-3, 0.3, 2.5) for sg in (2e-5, -0.05, 0.5)]             # sigma, rotation
    targets += [(ax, np.pi - 1e-3, sg) for ax in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)) for sg in (0.0, 0.1)]   # near pi, about each axis
    sim8, vi, vj, meas, group = [], [], [], [], []
    fixed, fix_scale = [], []
    scales = (0.2, 3.0, 1.0)
    for k, (ax, th, sg) in enumerate(targets):
        if k == 0:
            Si = Sj = C = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])
        else:
            Si, Sj = _state(rng, scales[k % 3]), _state(rng, scales[(k // 3) % 3])
            E = np.concatenate([_axis_angle(ax, th), rng.uniform(-1, 1, 3), [np.exp(sg)]])
            C = pgo_ref.sim3_mul(E, pgo_ref.sim3_mul(Sj, pgo_ref.sim3_inv(Si)))
        vi.append(len(sim8)); sim8.append(Si)
        vj.append(len(sim8)); sim8.append(Sj)
        meas.append(C)
        group.append("quirk" if abs(sg) >= 1e-5 and th < 4.47e-3 else ("near_pi" if th > 3.0 else "regular"))
        # flags: a fix_scale vertex on either side, a fixed vertex on either side, both fixed
        fix_scale += [1 if k % 5 == 1 else 0, 1 if k % 5 == 2 else 0]
        fixed += [1 if k % 7 == 3 else 0, 1 if k % 7 == 4 else 0]
    fixed[2 * 17], fixed[2 * 17 + 1] = 1, 1                                                            # an edge between two fixed vertices
    return dict(sim8=np.stack(sim8), fixed=np.array(fixed, np.uint8), fix_scale=np.array(fix_scale, np.uint8), vi=np.array(vi, np.int32), vj=np.array(vj, np.int32),
                meas8=np.stack(meas), info49=None), np.array(group)


@functools.lru_cache(maxsize=None)
def edge_terms_case():
    """edge_block_case()'s 46 edges with dense information, every second matrix (odd k) ASYMMETRIC: for the per-edge products of
    cs_pgo_edge_terms alone, where a transposed read of info49 shows.  Never optimised."""
    g, _ = edge_block_case()
    return dict(g, info49=edge_information(len(g["vi"]), 31, skew_every=2))


def edge_terms_expected(info49, e, Ji, Jj):
    """base_binary_edge.hpp:55-120 in long double from GIVEN e, J_i, J_j: J_i^T Omega J_i, J_i^T Omega J_j, J_j^T Omega J_j, -J_i^T Omega e,
    -J_j^T Omega e, e^T Omega e -- and for each the entrywise bound 32 * 2^-53 * (|.|^T |Omega| |.|): two nested 7-term sums in a fixed
    order carry at most 14 roundings per entry.  Returns {name: (value, bound)}."""
    L = np.longdouble
    W, e, Ji, Jj = np.asarray(info49, L).reshape(-1, 7, 7), np.asarray(e, L), np.asarray(Ji, L), np.asarray(Jj, L)
    u = L(32.0) * L(2.0) ** -53
    out = {}
    for name, a, b, sign in (("Hii", Ji, Ji, 1), ("Hij", Ji, Jj, 1), ("Hjj", Jj, Jj, 1), ("bi", Ji, e[:, :, None], -1), ("bj", Jj, e[:, :, None], -1),
                             ("chi2", e[:, :, None], e[:, :, None], 1)):
        val = sign * np.einsum("kra,krc,kcb->kab", a, W, b)
        bound = u * np.einsum("kra,krc,kcb->kab", np.abs(a), np.abs(W), np.abs(b))
        out[name] = (val.reshape(len(W), -1) if name in ("bi", "bj") else (val[:, 0, 0] if name == "chi2" else val),
                     bound.reshape(len(W), -1) if name in ("bi", "bj") else (bound[:, 0, 0] if name == "chi2" else bound))
    return out


@functools.lru_cache(maxsize=None)
def edge_block_refs():
    """(err, Ji, Jj) of the hand-placed edges in float64 and in long double."""
    g, _ = edge_block_case()
    return make_ref(g, np.float64).linearize_edges(), make_ref(g, np.longdouble).linearize_edges()


def block_deviation(a, b):
    """Per edge: the largest difference of a block, relative to the block's largest entry in b (1 where the block is zero)."""
    a, b = np.asarray(a, np.longdouble).reshape(len(a), -1), np.asarray(b, np.longdouble).reshape(len(b), -1)
    scale = np.abs(b).max(-1)
    return (np.abs(a - b).max(-1) / np.where(scale > 0, scale, 1)).astype(float)
