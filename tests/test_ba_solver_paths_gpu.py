"""Every factorisation of the reduced pose system against an exact float64 solve of the system the device factorised (tests/ba_numpy_ref.py).

The paths (csrc/ba_host.cpp: the choice in the structure phase; csrc/ba_lm.cpp: the solves in solve_device): the persistent banded Cholesky in its nested,
two-front and one-sided orders; block cyclic reduction (bcr_kernels.hip); the general sparse Cholesky (ba_sparse.h + sparse_kernels.hip)
with the default dense tail, a small one and none; dense rocSOLVER.  Per case, at lambda 1e-3 and 30:
  (a) cs_ba_get_reduced_system equals the numpy reduced matrix permuted to solver order (1e-12 of max |S|);
  (b) the reduced part of cs_ba_solve has a normwise backward error <= 1e-13 on the device's own S;
  (c) the whole increment (cameras, eliminated cuboids, landmarks) equals the numpy solve (1e-9 of max |x|);
  (d) 1e-3, 30, 1e-3 on one handle with no reduced_system() in between: the third increment is bit-identical to the first (the sparse
      path clears only its pattern of S after the first trial);
  (e) around lambda* (the most negative damping at which the whole damped system is positive definite) the device reports positive
      definite at lambda* + m and not at lambda* - m, and solves normally afterwards -- on the path (a)-(d) ran on;
  (f) the new sparse cases run the same 5 LM iterations as the same graph forced to dense.
Several switches are read once per process (CS_BAND_BCR, CS_BAND_TWO_FRONTS, CS_BAND_ONE_SIDED), so every switch set runs in a child
process of its own that writes an .npz under build_tmp/; the numpy checks run here.

Measured on one MI355X (2-norm condition number of S, backward error of (b), forward error of (c) relative to max |x|; lambda = 1e-3 /
lambda = 30; the test writes them to build_tmp/solver_paths_report.json):
  band_chain_cub   cond 6.6e8 / 7.5e5   backward 2.1e-17 / 1.6e-17   forward 1.7e-11 / 8.9e-14
  band_loop        cond 2.7e8 / 6.8e5   backward 2.3e-17 / 1.6e-17   forward 4.9e-11 / 6.3e-14
  bcr132 .. 1194   cond 8.1e7 .. 9.2e8  backward <= 3.2e-17          forward <= 2.4e-11
  bcr_cub          cond 1.9e8 / 7.9e5   backward 3.2e-17 / 2.5e-17   forward 3.9e-12 / 3.3e-14
  sparse_*         cond 2.5e7 .. 2.0e9  backward <= 3.1e-17          forward <= 6.4e-11 (chain300: 6.1e-11, mesh24: 2.4e-11)
  dense_chain      cond 1.7e8 / 3.6e5   backward 1.9e-17 / 2.6e-17   forward 1.5e-11 / 7.7e-14
  dense_mesh       cond 9.2e8 / 4.7e5   backward 3.3e-17 / 3.8e-17   forward 2.4e-10 / 6.3e-13
The two-front and one-sided band orders give the nested order's figures to two digits.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ba_numpy_ref as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))
LAMS = (1e-3, 30.0)


# ---- graphs (deterministic: the child builds the handle, this process rebuilds the same dict for the reference) ----------------------
def _merge(a, b):
    """Two problems side by side with no shared landmark and no edge between them (b's indices shifted behind a's)."""
    nc, no, np_ = len(a["cams"]), len(a["cuboids"]), len(a["points"])
    out = {}
    for k in ("cams", "cam_fixed", "cuboids", "cub_fixed", "points", "pt_fixed", "e_uv", "e_info", "e_intr", "e_huber", "ce_meas", "ce_info",
              "oe_meas", "oe_info", "pe_meas", "pe_info", "pe_K"):
        out[k] = np.concatenate([a[k], b[k]])
    for k, off in (("e_pt", np_), ("e_cam", nc), ("ce_cam", nc), ("ce_cub", no), ("oe_i", nc), ("oe_j", nc), ("pe_cam", nc), ("pe_cub", no)):
        out[k] = np.concatenate([a[k], b[k] + off]).astype(np.int32)
    return out


def graph(name):
    from cube_slam_wu_amd import synth_ba as S
    if name == "chain150_cub":
        return S.make_problem(150, 6000, 24, seed=21)
    if name == "loop150":
        return S.make_problem(150, 6000, 24, seed=22, loop=True)
    if name.startswith("chain") and name[5:].isdigit():         # chainN: N cameras (N - 1 free), no cuboid (an eliminated one would couple 20 cameras)
        n = int(name[5:])
        return S.make_problem(n, 40 * n, 0, seed=n)
    if name == "chain40_cub_narrow":                            # cuboids seen from 6 cameras each: a band of < 128 with 9-wide columns in it
        return S.make_problem(40, 1600, 6, seed=40, obs_per_cuboid=6)
    if name == "chain60_cub":
        return S.make_problem(60, 2400, 8, seed=60)
    if name == "mesh16":
        return S.make_mesh_problem(16, 16, 20000)
    if name == "mesh16_fixed":
        pr = S.make_mesh_problem(16, 16, 20000)
        pr["cam_fixed"] = pr["cam_fixed"].copy()
        pr["cam_fixed"][[37, 101, 150, 190, 222]] = 1
        return pr
    if name == "forest":
        return _merge(S.make_mesh_problem(8, 8, 4000, seed=1), S.make_mesh_problem(10, 10, 6000, seed=2))
    if name == "mesh24":
        return S.make_mesh_problem(24, 24, 20000)
    if name == "mesh8":
        return S.make_mesh_problem(8, 8, 3000)
    raise KeyError(name)


# ---- cases: name -> (graph, per-handle environment, expected path, checks) -------------------------------------------------------------
# expected: (path, bcr, exact n_red or None, cuboids eliminated or None, extra); per-handle switches (read at handle creation or in the
# structure phase) are set around the handle; per-process switches pick the child.
KEEP = {"CS_BA_KEEP_CUBOIDS": "1"}
SPARSE = {"CS_BA_SPARSE": "1"}
DENSE = {"CS_BA_FORCE_DENSE": "1"}
CHILDREN = {
    "band": ({"CS_BAND_BCR": "0"}, ["band_chain_cub", "band_loop"]),
    "two_fronts": ({"CS_BAND_BCR": "0", "CS_BAND_TWO_FRONTS": "1"}, ["band_chain_cub", "band_loop"]),
    "one_sided": ({"CS_BAND_BCR": "0", "CS_BAND_ONE_SIDED": "1"}, ["band_chain_cub", "band_loop"]),
    "bcr": ({"CS_BAND_BCR": "2"}, ["bcr132", "bcr258", "bcr384", "bcr1194", "bcr_cub"]),
    # (CS_BA_PROF: the structure phase prints its sparse plan -- the dense tail's size is read from that line, _structure())
    "sparse": ({"CS_BA_PROF": "1"}, ["sparse_mesh", "sparse_mesh_fixed", "sparse_forest", "sparse_no_tail", "sparse_tail200", "sparse_9wide", "sparse_chain300",
                    "sparse_mesh24", "dense_chain", "dense_mesh"]),
}
CASES = {
    "band_chain_cub": dict(graph="chain150_cub", env=KEEP, path="band", bcr=False, elim=False),
    "band_loop": dict(graph="loop150", env={}, path="band", bcr=False),
    "bcr132": dict(graph="chain23", env={}, path="band", bcr=True, n_red=132, levels=2),
    "bcr258": dict(graph="chain44", env={}, path="band", bcr=True, n_red=258, levels=2),
    "bcr384": dict(graph="chain65", env={}, path="band", bcr=True, n_red=384, levels=2),
    "bcr1194": dict(graph="chain200", env={}, path="band", bcr=True, n_red=1194, levels=4),
    "bcr_cub": dict(graph="chain40_cub_narrow", env=KEEP, path="band", bcr=True, elim=False),
    # tail: the dense tail's unknowns as a (lo, hi) range.  ba_sparse.h:sparse_plan_build keeps a tail only where it spans at least 24
    # elimination positions (a shorter one costs rocSOLVER's launches without shortening the level chain), i.e. >= 144 unknowns of
    # 6-wide cameras: a cap below that is no tail at all.  On mesh16 the default cap gives 474 unknowns, a cap of 200 gives 198.
    "sparse_mesh": dict(graph="mesh16", env=SPARSE, path="sparse", tail=(201, 9000)),
    "sparse_mesh_fixed": dict(graph="mesh16_fixed", env=SPARSE, path="sparse"),
    "sparse_forest": dict(graph="forest", env=SPARSE, path="sparse"),
    "sparse_no_tail": dict(graph="mesh16", env={**SPARSE, "CS_BA_SPARSE_NO_TAIL": "1"}, path="sparse", lm=True, tail=(0, 0)),
    "sparse_tail200": dict(graph="mesh16", env={**SPARSE, "CS_BA_SPARSE_TAIL_MAX": "200"}, path="sparse", tail=(144, 200)),
    "sparse_9wide": dict(graph="chain60_cub", env={**SPARSE, **KEEP}, path="sparse", elim=False, lm=True),
    "sparse_chain300": dict(graph="chain300", env=SPARSE, path="sparse", wrap=True, lm=True),
    "sparse_mesh24": dict(graph="mesh24", env=SPARSE, path="sparse", wrap=True, lm=True),
    "dense_chain": dict(graph="chain60_cub", env=DENSE, path="dense", cuboids_first=True),
    "dense_mesh": dict(graph="mesh8", env=DENSE, path="dense"),
}


# ---- child ------------------------------------------------------------------------------------------------------------------------------
def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _handle(pr, cuboids_first):
    from cube_slam_wu_amd import capi
    G = capi.ba_from_dict(pr, cuboids_first=cuboids_first)
    G.compute_errors()
    return G


def _structure(pr, cf):
    """A handle with its structure phase done and its system built -> (handle, system, dense tail unknowns of its sparse plan, -1 without
    a plan).  The tail's size is in the line the structure phase prints under CS_BA_PROF (stderr of this process, taken from fd 2)."""
    import re
    import tempfile
    with tempfile.TemporaryFile() as tmp:
        sys.stderr.flush()
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            G = _handle(pr, cf)
            system = G.build_system()
            G.solver_path()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
            tmp.seek(0)
            text = tmp.read().decode(errors="replace")
            sys.stderr.write(text)
    m = re.findall(r"sparse plan: .* a dense tail of (\d+) unknowns", text)
    return G, system, int(m[-1]) if m else -1


def _margin(lam_star, S):
    return max(0.05 * abs(lam_star), 1e3 * len(S) * np.finfo(float).eps * np.abs(S).sum(1).max())


def _pd_graph(pr):
    """The graph for (e) where a landmark sets lambda*.  g2o inverts the landmark blocks by cofactors without a test (block_solver.hpp)
    and checks only the reduced system, so lambda* - m must leave every H_ll + lambda I positive definite.  On the meshes the reduced
    system sets lambda*; along a chain the weakest landmark does (a far point's depth, seen from a short baseline: lambda* lies just
    above -min eig H_ll), and fixing the weakest few only hands the part to the next.  There every landmark is fixed: the projections
    still build H_pp, the reduced system is the pose system alone, and lambda* is its own."""
    pr2 = dict(pr)
    pr2["pt_fixed"] = np.ones(len(pr["points"]), np.int32)
    return pr2


def _run_case(name, out):
    c = CASES[name]
    cf = bool(c.get("cuboids_first", False))
    pr = graph(c["graph"])
    G, system, n_tail = _structure(pr, cf)
    out[name + "/n_tail"] = np.array(n_tail)
    out[name + "/path"] = np.array(G.solver_path(detail=True), dtype=object).astype(str)
    out[name + "/band_order"] = np.array(G.band_order(), dtype=np.int64)
    out[name + "/reduced_size"] = np.array(G.reduced_size(), dtype=np.int64)
    import torch
    out[name + "/cus"] = np.array(torch.cuda.get_device_properties(0).multi_processor_count)
    for k, v in zip(("Hpp", "Hll", "Hpl", "b"), system):
        out["%s/%s" % (name, k)] = v
    for lam in LAMS:
        S, r, cc, oc = G.reduced_system(lam)
        out["%s/S_%g" % (name, lam)], out["%s/r_%g" % (name, lam)] = S, r
    out[name + "/cam_col"], out[name + "/cub_col"] = cc, oc
    seq = []
    for lam in (1e-3, 30.0, 1e-3):        # (d): no reduced_system() in between
        ok, x = G.solve(lam)
        seq.append((ok, x))
    out[name + "/x_ok"] = np.array([s[0] for s in seq])
    out[name + "/x_seq"] = np.stack([s[1] for s in seq])
    F = ref.Reference(system, pr, cf)
    lam_star, lam_lm = F.lambda_star()
    if lam_star - _margin(lam_star, F.schur(1e-3)[0]) <= lam_lm:
        # (e) on the graph with every landmark fixed (_pd_graph): a handle of its own, whose path is recorded like the case's
        G.close()
        pr = _pd_graph(pr)
        G, system, n_tail = _structure(pr, cf)
        F = ref.Reference(system, pr, cf)
        lam_star = F.lambda_star()[0]
        out[name + "/pd_path"] = np.array(G.solver_path(detail=True), dtype=object).astype(str)
        out[name + "/pd_band_order"] = np.array(G.band_order(), dtype=np.int64)
        out[name + "/pd_reduced_size"] = np.array(G.reduced_size(), dtype=np.int64)
        out[name + "/pd_n_tail"] = np.array(n_tail)
        out[name + "/pd_pt_fixed"] = pr["pt_fixed"]
        for k, v in zip(("Hpp", "Hll", "Hpl", "b"), system):
            out["%s/pd_%s" % (name, k)] = v
    m = _margin(lam_star, F.schur(1e-3)[0])
    out[name + "/pd_lams"] = np.array([lam_star, m])
    out[name + "/pd"] = np.array([G.solve(lam_star + m)[0], G.solve(lam_star - m)[0], G.solve(1e-3)[0]])
    G.close()
    if c.get("lm"):
        runs = []
        for env in (c["env"], DENSE):
            def run():
                H = _handle(pr, cf)
                p = H.solver_path()
                n = H.optimize(5)
                chi, lam, tr = H.history()
                H.close()
                return p, n, chi.copy(), tr.copy()
            runs.append(_with_env(env, run))
        out[name + "/lm_paths"] = np.array([r[0] for r in runs])
        out[name + "/lm_n"] = np.array([r[1] for r in runs])
        out[name + "/lm_chi"] = np.stack([r[2] for r in runs])
        out[name + "/lm_tr"] = np.stack([r[3] for r in runs])


def child_main(group, path):
    """The group's cases in turn.  The first case that raises ends the process (a HIP error or a wait time-out surfaces as an exception
    of the C ABI wrapper): what was recorded so far is saved, the exception propagates and the process exits non-zero."""
    out = {}
    try:
        for name in CHILDREN[group][1]:
            _with_env(CASES[name]["env"], lambda: _run_case(name, out))
            print("case %s done" % name, flush=True)
    finally:
        np.savez(path, **out)


# ---- parent -------------------------------------------------------------------------------------------------------------------------------
_results = {}
_stopped = []      # a child that died by a signal or ran out of time: no further child is started on the device


def _child(group):
    assert not _stopped, "an earlier child ended abnormally (%s): no further child is started" % _stopped[0]
    if group not in _results:
        f = os.path.join(ROOT, "build_tmp", "solver_paths_%s.npz" % group)
        os.makedirs(os.path.dirname(f), exist_ok=True)
        if os.path.exists(f):
            os.remove(f)
        code = "import sys; sys.path[:0] = [%r, %r]; import test_ba_solver_paths_gpu as T; T.child_main(%r, %r)" % (ROOT, TESTS, group, f)
        env = {**os.environ, **CHILDREN[group][0]}
        try:
            r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600, env=env)
        except subprocess.TimeoutExpired:
            _stopped.append("%s: time-out" % group)
            raise
        if r.returncode < 0 or r.returncode in (134, 139):
            _stopped.append("%s: exit %d" % (group, r.returncode))
        if r.returncode != 0:
            _results[group] = "child %s failed (%d):\n%s\n%s" % (group, r.returncode, r.stdout[-3000:], r.stderr[-3000:])
        else:
            _results[group] = dict(np.load(f, allow_pickle=False))
    assert not isinstance(_results[group], str), _results[group]
    return _results[group]


def _report(name, **kv):
    f = os.path.join(ROOT, "build_tmp", "solver_paths_report.json")
    rep = json.load(open(f)) if os.path.exists(f) else {}
    rep[name] = {k: (float(v) if np.ndim(v) == 0 else [float(u) for u in v]) for k, v in kv.items()}
    json.dump(rep, open(f, "w"), indent=1, sort_keys=True)


def _assert_path(name, c, pr, g, pre):
    """The handle (pre "": the case's own; "pd_": the one (e) ran on) took the path the case is about."""
    path, bw, fill = [str(v) for v in g(pre + "path")]
    bcr, levels = [int(v) for v in g(pre + "band_order")]
    n_red, elim = [int(v) for v in g(pre + "reduced_size")]
    n_tail = int(g(pre + "n_tail"))
    assert path == c["path"], (name, pre, path, c["path"])
    assert bool(bcr) == bool(c.get("bcr", False)), (name, pre, bcr)
    if "n_red" in c:
        assert n_red == c["n_red"], (name, pre, n_red)
    if "levels" in c:
        assert levels == c["levels"], (name, pre, levels)
    if "elim" in c:
        assert elim == c["elim"], (name, pre, elim)
    if c.get("bcr"):
        assert int(bw) <= 128, (name, pre, bw)
    if "tail" in c:
        assert c["tail"][0] <= n_tail <= c["tail"][1], (name, pre, "dense tail of %d unknowns" % n_tail, c["tail"])
    if path == "sparse":
        assert n_tail >= 0, (name, pre, "no sparse plan line")
    if not c.get("elim", True):
        assert len(pr["cuboids"]) > 0 and n_red > 6 * int((np.asarray(pr["cam_fixed"]) == 0).sum()), "no 9-wide column in the reduced system"
    if c.get("wrap"):
        # more free vertices than the factorisation's grid: sparse_grids() sizes it min(N, occupancy x CUs), and the panel's LDS
        # (sparse_lds_bytes: ~134 KB of the 160 KB per CU, sparse_kernels.hip) makes the occupancy 1 -- so the grid is the CU count and
        # some workgroup takes a second column (idx += gridDim.x).  A smaller panel cap would need this bound times the occupancy.
        n_free = int((np.asarray(pr["cam_fixed"]) == 0).sum()) + (0 if elim else int((np.asarray(pr["cub_fixed"]) == 0).sum()))
        assert n_free > int(g("cus")), (name, pre, n_free, int(g("cus")))
    return n_red, elim


def _check(group, name):
    d = _child(group)
    c = CASES[name]
    g = lambda k: d["%s/%s" % (name, k)]
    cf = bool(c.get("cuboids_first", False))
    pr = graph(c["graph"])
    n_red, elim = _assert_path(name, c, pr, g, "")
    F = ref.Reference((g("Hpp"), g("Hll"), g("Hpl"), g("b")), pr, cf)
    perm, _ = ref.solver_permutation(pr, g("cam_col"), g("cub_col"), n_red, cf)
    xs, oks = g("x_seq"), g("x_ok")
    assert oks.all(), (name, oks)
    rep = {}
    for i, lam in enumerate(LAMS):
        S, r = g("S_%g" % lam), g("r_%g" % lam)
        # (a) assembly: every entry, the band's outside included
        S_ref, r_ref = F.reduced(lam, perm)
        dS = np.abs(S - S_ref).max() / np.abs(S_ref).max()
        dr = np.abs(r - r_ref).max() / np.abs(r_ref).max()
        assert dS <= 1e-12, (name, lam, "reduced system", dS)
        assert dr <= 1e-12, (name, lam, "reduced rhs", dr)
        # (b) factorisation: backward error of the device's increment on the device's own S
        x = xs[i]
        xr = x[perm]
        be = np.abs(S @ xr - r).max() / (np.abs(S).sum(1).max() * np.abs(xr).max() + np.abs(r).max())
        assert be <= 1e-13, (name, lam, "backward error", be)
        # (c) the whole increment
        ok, x_ref = F.solve(lam)
        assert ok
        fe = np.abs(x - x_ref).max() / np.abs(x_ref).max()
        assert fe <= 1e-9, (name, lam, "forward error", fe)
        ev = np.linalg.eigvalsh(S_ref)
        rep.update({"cond_%g" % lam: ev[-1] / ev[0], "backward_%g" % lam: be, "forward_%g" % lam: fe, "dS_%g" % lam: dS})
    # (d) the re-solve after a pattern-only clear: bit-identical
    assert np.array_equal(xs[2], xs[0]), (name, "re-solve", np.abs(xs[2] - xs[0]).max())
    # (e) definiteness around lambda*
    F_e = F
    if name + "/pd_pt_fixed" in d:      # (every landmark fixed: _pd_graph) -- on the same path as (a)-(d), asserted the same way
        pr_e = dict(pr)
        pr_e["pt_fixed"] = g("pd_pt_fixed")
        assert (pr_e["pt_fixed"] == 1).all()
        # (the case's expectations hold for it, and it factorises the same way: band order and levels; the loop's cuboids may be
        # eliminated there and kept in the case -- the landmarks' coupling decided that -- so n_red is pinned only where the case pins it)
        _assert_path(name, c, pr_e, g, "pd_")
        assert np.array_equal(g("pd_band_order"), g("band_order")), (name, g("pd_band_order"), g("band_order"))
        F_e = ref.Reference((g("pd_Hpp"), g("pd_Hll"), g("pd_Hpl"), g("pd_b")), pr_e, cf)
    lam_star, m = g("pd_lams")
    pd_plus, pd_minus, pd_after = [bool(v) for v in g("pd")]
    assert m == _margin(lam_star, F_e.schur(1e-3)[0])
    assert F_e.positive_definite(lam_star + m) and not F_e.positive_definite(lam_star - m), (name, "lambda* is not the threshold")
    assert F_e.landmarks_pd(lam_star - m), (name, "a landmark block sets lambda*")
    assert pd_plus, (name, "not positive definite at lambda* + m", lam_star, m)
    assert not pd_minus, (name, "positive definite at lambda* - m", lam_star, m)
    assert pd_after, (name, "no normal solve after the indefinite one")
    rep.update({"lambda_star": lam_star, "margin": m})
    # (f) LM against the same graph forced to dense
    if c.get("lm"):
        paths = [str(p) for p in g("lm_paths")]
        assert paths == [c["path"], "dense"], (name, paths)
        n = g("lm_n")
        assert n[0] == n[1] == 5
        chi, tr = g("lm_chi"), g("lm_tr")
        assert np.array_equal(tr[0], tr[1]), (name, tr)
        assert np.abs(chi[0] - chi[1]).max() <= 1e-9 * np.abs(chi[1]).max(), (name, chi)
    _report(name, **rep)


@pytest.mark.parametrize("name", CHILDREN["band"][1])
def test_band_nested(name):
    _check("band", name)


@pytest.mark.parametrize("name", CHILDREN["two_fronts"][1])
def test_band_two_fronts(name):
    _check("two_fronts", name)


@pytest.mark.parametrize("name", CHILDREN["one_sided"][1])
def test_band_one_sided(name):
    _check("one_sided", name)


@pytest.mark.parametrize("name", CHILDREN["bcr"][1])
def test_block_cyclic_reduction(name):
    _check("bcr", name)


@pytest.mark.parametrize("name", CHILDREN["sparse"][1])
def test_sparse_and_dense(name):
    _check("sparse", name)
