"""ORB-SLAM2's LocalBundleAdjustment as rounds over tests/ba_stereo_ref.Graph (test infrastructure, not a test file; nothing of the product is
imported).

The reference has no edge level.  "Level 1" is restated as *the same vertices, the edge left out*: a round is Graph.optimize() on the sub-graph
of the kept edges, the classification between the rounds is `e->chi2() > 5.991 (mono) / 7.815 (stereo) || !isDepthPositive()` through
Graph.edge_chi2() and Graph.errors()[1][:, 2] > 0, `setRobustKernel(0)` is a sub-graph built without deltas, and the next round starts from the
state the last one reached.  Every classification is taken at the returned state (g2o's e->chi2() after optimize() is the last trial's, which is
the returned state whenever that trial was accepted -- asserted here through the trial counts of the cases).

Cases (the device tests and the CPU test share them, computed once per process): the injection recipe puts N(0, 12) pixels on 5 % of the
measurements of ba_stereo_ref.make_family(), Huber deltas sqrt(5.991) / sqrt(7.815) in the first round.
"""
import functools

import numpy as np

import ba_stereo_ref as ref

TH = (5.991, 7.815)
HUB = (np.sqrt(TH[0]), np.sqrt(TH[1]))
LOCAL_BA = ((5, True, (TH[0], TH[1], 1, 1)), (10, False, (TH[0], TH[1], 1, 0)))      # cs_ba_optimize_rounds' schedule of LocalBundleAdjustment
MARGIN = 1e-3            # no edge closer than this (relative) to its threshold at a classification the device is compared at

CASES = {
    "dense24": dict(seed=1, kw={}),                                              # 24 cameras: dense reduced system, the long-track kernel
    "band60": dict(seed=2, kw=dict(long_track=False, n_cams=60)),                # banded solve, fused linearisation from the second iteration on
    "mono24": dict(seed=1, kw=dict(stereo_share=0.0)),                           # no stereo edge: the kernels' STEREO = false instantiations
}


def make_case(seed, **kw):
    """make_family(seed, **kw) with gross errors injected: the issue's recipe, in its order."""
    f = ref.make_family(seed=seed, **kw)
    rng = np.random.default_rng(1000 + seed)
    m, s = list(f["mono"]), list(f["stereo"])
    m[2], s[2] = m[2].copy(), s[2].copy()
    om = rng.random(len(m[0])) < 0.05
    os_ = rng.random(len(s[0])) < 0.05
    m[2][om] += rng.normal(0, 12, (om.sum(), 2))
    s[2][os_] += rng.normal(0, 12, (os_.sum(), 3))
    f["mono"], f["stereo"] = tuple(m), tuple(s)
    return f


def subgraph(f, cams, points, keep_mono=None, keep_stereo=None, huber=None):
    """Graph of f's vertices at the given estimates with the kept edges only (keep_* = boolean per edge of the class, None = all); huber = (delta
    mono, delta stereo) or None (no kernels); a delta is one number for the class or an array with every edge's own (kept or not)."""
    def sub(t, keep, delta):
        keep = np.ones(len(t[0]), bool) if keep is None else np.asarray(keep, bool)
        if not keep.any():
            return None
        if delta is not None and np.ndim(delta) == 1:
            assert len(delta) == len(keep)
            delta = np.asarray(delta, float)[keep]
        return tuple(np.asarray(a)[keep] for a in t[:5]) + (np.full(int(keep.sum()), delta if delta is not None else 0.0),)
    return ref.Graph(cams, f["cam_fixed"], points, f["pt_fixed"], sub(f["mono"], keep_mono, huber[0] if huber else None),
                     sub(f["stereo"], keep_stereo, huber[1] if huber else None))


def classify(G, th=TH, depth_positive=True):
    """(outlier per edge of G, plain chi2, smallest |chi2 / threshold - 1|) at G's state."""
    chi = G.edge_chi2()
    t = np.where(G.stereo, th[1], th[0])
    out = chi > t
    if depth_positive:
        out = out | ~(G.errors()[1][:, 2] > 0)
    return out, chi, float(np.abs(chi / t - 1).min())


def local_ba(f, iters=(5, 10), huber=HUB):
    """The two rounds and the two classifications of LocalBundleAdjustment on f.  Returns a dict: per round `done`, `hist` (chi2, lambda, trials),
    `rho` (every trial's gain ratio); `out1` / `out2` = outliers after round 1 / at the end over ALL edges (mono first), `margin1` / `margin2`,
    `state1` / `state2` = (cams7, points) after each round, `n_mono`.  huber: the first round's deltas, as subgraph() takes them."""
    nm = len(f["mono"][0])
    G1 = ref.graph_of(f, huber=huber)
    d1 = G1.optimize(iters[0])
    out1, _, margin1 = classify(G1)
    cams1, _, X1 = G1.state()
    G2 = subgraph(f, cams1, X1, ~out1[:nm], ~out1[nm:])
    d2 = G2.optimize(iters[1])
    cams2, _, X2 = G2.state()
    # the final classification tests every edge again (sticky = 0): the full graph at the final state
    out2, chi2_all, margin2 = classify(subgraph(f, cams2, X2))
    kept = ~out1
    return dict(n_mono=nm, done=(d1, d2), hist=(G1.history(), G2.history()), rho=(list(G1.rho_log), list(G2.rho_log)), out1=out1, out2=out2,
                margin1=margin1, margin2=margin2, state1=(cams1, X1), state2=(cams2, X2), final_outliers_among_kept=int(out2[kept].sum()),
                active1=(np.bincount(G1.e_pt[kept], minlength=G1.npt), np.bincount(G1.e_cam[kept], minlength=G1.nc)), e_pt=G1.e_pt)


@functools.lru_cache(maxsize=None)
def case(name):
    """(family dict with the injected errors, local_ba() of it) of CASES[name], computed once per process and shared: treat both as read-only."""
    c = CASES[name]
    f = make_case(c["seed"], **c["kw"])
    return f, local_ba(f)


def assert_comparable(r):
    """The conditions under which the device may be held to the reference's decisions: no edge within MARGIN of its threshold at either
    classification, every gain ratio clear of zero."""
    assert r["margin1"] > MARGIN and r["margin2"] > MARGIN, (r["margin1"], r["margin2"])
    assert all(abs(x) > 1e-6 for x in r["rho"][0] + r["rho"][1])
