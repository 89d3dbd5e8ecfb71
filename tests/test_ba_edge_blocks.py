"""The CPU oracle's cuboid, box and odometry edge blocks against the exact-quotient fixture tests/golden/ba_edge_blocks.npz.

The fixture (tools/make_edge_golden.py: a 60-digit mpmath restatement from the reference's sources, nothing of oracle/ or csrc/ in its
mathematics) gives per edge the error e and the exact central-difference quotient J; tests/edge_blocks_ref.py forms the blocks
(J^T W J, -J^T W e, W = rho' Omega) in float64 and wires the edges into a disjoint graph (every block of H_pp is one edge's) and into
shared graphs (blocks are sums over edges).  Every deviation is max|B - B_ref| / max|B_ref| of THAT block, never of the whole matrix.

Bounds are measured, not chosen: the generator stored the oracle's worst deviation per class, family and block kind (oracle_dev/...).
Here the oracle must reproduce them within a factor 2 (same code: a change that doubles its noise is a finding), none may exceed 1e-5,
and the shared graphs must stay within 8 x the summed allowances (edge_blocks_ref.check_system).  chi2 per class against sum rho(e^T Omega e).

The guards show that the fixture can fail: what a plausible mistake (a diagonal-only information matrix, H_ab read with the wrong leading
dimension, the runner-up yaw candidate, a fixed end that is not zero) would change, in units of the blocks themselves.  The log_small
family is different on purpose: at 1e-3 and 3e-3 rad the acos formula and the small-angle formula of SE3Quat::log agree to within the
tolerance, so that family tests that the branch EXISTS and is taken without harm (no 0/0, no loss of digits in theta / sqrt(1 - d^2)),
not which of the two values is returned; log_acos / moderate / large hold the acos formula's value, and a branch threshold moved far
enough (d > 0.9) is caught by `moderate`.
"""
import importlib.util
import os

import numpy as np
import pytest

import edge_blocks_ref as EB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 8.0                       # the device's margin over the oracle's measured noise (see test_ba_edge_blocks_gpu.py)


@pytest.fixture(scope="module")
def fx():
    return EB.load()


def _oracle_system(pr, cuboids_first):
    P = EB.oracle_problem(pr, cuboids_first)
    chi = P.compute_errors()[0]
    Hpp, _, _, b = P.build_system()
    P.close()
    return chi, Hpp, b


def test_fixture_families_and_conditions(fx):
    """What the issue fixes about the inputs, re-checked from the stored values: family sizes, dense symmetric information, the leads,
    both sides of log's branch, fixed ends, kernels; and no stored oracle deviation above 1e-5."""
    assert os.path.getsize(EB.FIXTURE) < 400 * 1024
    thr = EB.clear_lead_threshold()
    fam = fx["cub/family"].astype(str)
    for i in range(4):
        m = fam == "cand%d" % i
        assert m.sum() >= 6 and (fx["cub/win"][m] == i).all() and (fx["cub/lead"][m] > 1e-2).all()
    tie = fam == "near_tie"
    assert tie.sum() >= 8 and (fx["cub/lead"][tie] >= 1e-5).all() and (fx["cub/lead"][tie] <= 5e-4).all() and (fx["cub/lead"][tie] < thr).all()
    assert (fx["cub/lead"][~tie] > thr).all()
    assert sorted(set(fx["cub/win"][tie])) == [0, 1, 2, 3]
    assert (fx["box/lead_px"] > 1e-3).all() and (fx["box/family"].astype(str) == "off_image").sum() >= 6
    for cls in ("cub", "odo"):
        f, ang = fx[cls + "/family"].astype(str), fx[cls + "/angle"]
        assert (f == "log_small").sum() >= 4 and (f == "log_acos").sum() >= 4
        assert (ang[f == "log_small"] < 3.5e-3).all() and (ang[f == "log_acos"] > 5.5e-3).all()      # d > 0.99999 <=> angle < 4.47e-3
    f, ang = fx["odo/family"].astype(str), fx["odo/angle"]
    assert ((ang[f == "moderate"] >= 0.1) & (ang[f == "moderate"] <= 1.0)).all() and ((ang[f == "large"] >= 2.0) & (ang[f == "large"] <= 2.6)).all()
    assert (fx["odo/a"] > fx["odo/b"]).sum() >= 8
    for cls in EB.CLASSES:
        D = EB.DIMS[cls][0]
        n = len(fx[cls + "/a"])
        info = fx[cls + "/info"].reshape(n, D, D)
        assert np.array_equal(info, info.transpose(0, 2, 1)) and (np.linalg.cond(info) <= 1e3).all()
        off = np.abs(info[:, ~np.eye(D, dtype=bool)]).reshape(n, -1).max(1)
        assert (off > 0.05 * np.abs(np.einsum("kii->ki", info)).max(1)).all(), "an information matrix is (nearly) diagonal"
        assert fx[cls + "/fixed_a"].sum() == 2 and fx[cls + "/fixed_b"].sum() == 2 and not (fx[cls + "/fixed_a"] & fx[cls + "/fixed_b"]).any()
        kinds = fx[cls + "/rk_kind"]
        assert abs((kinds > 0).mean() - 0.25) < 0.05 and set(kinds[kinds > 0]) == {EB.RK_HUBER, EB.RK_CAUCHY, EB.RK_TUKEY, EB.RK_DCS}
        w = np.array([EB.robustify(int(kinds[k]), float(fx[cls + "/rk_delta"][k]), float(fx[cls + "/e"][k] @ info[k] @ fx[cls + "/e"][k]))[1] for k in range(n)])
        assert 0.3 <= (w[kinds > 0] < 1).mean() <= 0.8, "about half of the kernels in the outlier regime"
    devs = {k: float(v) for k, v in fx.items() if k.startswith("oracle_dev/")}
    assert len(devs) == 5 * (8 + 2 + 4) + 3
    assert all(0 < v <= 1e-5 for k, v in devs.items() if not k.endswith("chi2")), "a family is badly conditioned"


@pytest.mark.parametrize("cuboids_first", [False, True])
def test_oracle_disjoint_graph_per_edge(fx, cuboids_first):
    """Every edge on vertices of its own: each block of the oracle's H_pp and each segment of b against that edge's reference block.  The
    oracle reproduces the deviations the generator stored within a factor 2; no edge is skipped."""
    pr, ends = EB.layout(fx, EB.CLASSES, shared=False)
    chi, H, b = _oracle_system(pr, cuboids_first)
    devs = EB.edge_devs(fx, pr, ends, H, b, cuboids_first)
    assert sum(len(d) for d in devs.values()) == sum(len(fx[c + "/a"]) for c in EB.CLASSES)
    tab = EB.family_table(fx, devs)
    for cls in tab:
        for fam in tab[cls]:
            for kd, v in tab[cls][fam].items():
                stored = EB.oracle_dev(fx, cls, fam, kd)
                print("%s %-10s %-4s oracle %.3g stored %.3g" % (cls, fam, kd, v, stored))
                assert v <= 2 * stored, (cls, fam, kd, v, stored)
    EB.check_system(fx, pr, ends, H, b, cuboids_first, factor=2.0, what="oracle, disjoint")
    want = EB.chi2_ref(fx, EB.CLASSES)
    assert abs(chi - want) <= 1e-11 * want


@pytest.mark.parametrize("classes", [("cub",), ("box",), ("odo",), EB.CLASSES], ids=["cub", "box", "odo", "all"])
@pytest.mark.parametrize("cuboids_first", [False, True])
def test_oracle_shared_graphs(fx, classes, cuboids_first):
    """Vertices shared between edges: the oracle's blocks against the SUMS of the per-edge reference blocks (every entry within 8 x the sum
    of its parts' allowances, untouched entries exactly zero), chi2 per class against sum rho(e^T Omega e)."""
    pr, ends = EB.layout(fx, classes, shared=True)
    assert len(pr["cams"]) <= len(fx["cams"]) and len(pr["cuboids"]) <= len(fx["cuboids"])
    chi, H, b = _oracle_system(pr, cuboids_first)
    worst = EB.check_system(fx, pr, ends, H, b, cuboids_first, factor=FACTOR, what="oracle, shared " + "+".join(classes))
    print("worst deviation / allowance:", worst)
    want = EB.chi2_ref(fx, classes)
    dev = abs(chi - want) / want
    if len(classes) == 1:
        stored = float(fx["oracle_dev/%s/chi2" % classes[0]])
        print("chi2 deviation %.3g, stored %.3g" % (dev, stored))
        assert stored <= 1e-11
    assert dev <= 1e-11


def test_oracle_chi2_per_class_reproduces_stored(fx):
    for cls in EB.CLASSES:
        pr, _ = EB.layout(fx, (cls,), shared=False)
        chi = _oracle_system(pr, False)[0]
        want = EB.chi2_ref(fx, (cls,))
        assert abs(chi - want) / want <= max(2 * float(fx["oracle_dev/%s/chi2" % cls]), 4 * np.finfo(float).eps)


# ---- guards: the fixture can fail -------------------------------------------------------------------------------------------------------
def _all_edges(fx):
    return [(cls, k) for cls in EB.CLASSES for k in range(len(fx[cls + "/a"]))]


def test_guard_diagonal_information_changes_the_blocks(fx):
    """Reading only the diagonal of Omega changes >= 90 % of the reference blocks by more than 1e-2 of themselves."""
    changed = total = 0
    for cls, k in _all_edges(fx):
        D = EB.DIMS[cls][0]
        info = fx[cls + "/info"][k].reshape(D, D)
        Bref, _ = EB.fixture_edge_blocks(fx, cls, k)
        Bd, _ = EB.fixture_edge_blocks(fx, cls, k, info=np.diag(np.diag(info)))
        for r, d in zip(Bref, Bd):
            if np.any(r):
                total += 1
                changed += EB.rel_dev(d, r) > 1e-2
    assert total > 500 and changed >= 0.9 * total, (changed, total)


def test_guard_transposed_cross_block_changes_it(fx):
    """H_ab written with rows and columns in each other's place (the same numbers under the other leading dimension; for the 6 x 6 odometry
    block: the transpose) differs from H_ab by more than 1e-2 of it, for every edge that has one."""
    n = 0
    for cls, k in _all_edges(fx):
        _, NA, NB = EB.DIMS[cls]
        Hab = EB.fixture_edge_blocks(fx, cls, k)[0][2]
        if np.any(Hab):
            n += 1
            assert EB.rel_dev(np.ascontiguousarray(Hab.T).reshape(NA, NB), Hab) > 1e-2, (cls, k)
    assert n > 100


def test_guard_runner_up_candidate_changes_the_blocks(fx):
    """cand* and near_tie edges: the blocks of the runner-up yaw candidate (its e and J, also exact) differ from the winner's by more than
    1e-2 -- a wrong winner, or a perturbed evaluation that switches candidate, cannot hide inside the tolerance."""
    fam = fx["cub/family"].astype(str)
    n = 0
    for k in np.nonzero(np.char.startswith(fam, "cand") | (fam == "near_tie"))[0]:
        info = fx["cub/info"][k].reshape(9, 9)        # (without the kernel's weight: a Tukey outlier's blocks are zero for either candidate)
        fa, fb = bool(fx["cub/fixed_a"][k]), bool(fx["cub/fixed_b"][k])
        Bref = EB.edge_blocks(fx["cub/e"][k], fx["cub/J"][k], info, 6, 1.0, fa, fb)
        Br = EB.edge_blocks(fx["cub/e_runner"][k], fx["cub/J_runner"][k], info, 6, 1.0, fa, fb)
        for kd, r, d in zip(EB.KINDS, Bref, Br):
            assert np.any(r) and EB.rel_dev(d, r) > 1e-2, (k, kd, EB.rel_dev(d, r))
        n += 1
    assert n >= 32


def test_guard_log_small_formulas_agree_within_tolerance(fx):
    """log_small tests the branch's existence, not its value: the blocks from the acos formula (e_alt, J_alt: the same edges evaluated at 60
    digits with the other formula) lie within the device's tolerance (8 x oracle_dev) of the small-angle formula's."""
    n = 0
    for cls in ("cub", "odo"):
        for k in np.nonzero(fx[cls + "/family"].astype(str) == "log_small")[0]:
            Bref, _ = EB.fixture_edge_blocks(fx, cls, k)
            Ba, _ = EB.fixture_edge_blocks(fx, cls, k, e=fx[cls + "/e_alt"][k], J=fx[cls + "/J_alt"][k])
            for kd, r, a in zip(EB.KINDS, Bref, Ba):
                d = EB.rel_dev(a, r)
                print("%s %d %-4s formulas differ by %.3g, tolerance %.3g" % (cls, k, kd, d, FACTOR * EB.oracle_dev(fx, cls, "log_small", kd)))
                assert d < FACTOR * EB.oracle_dev(fx, cls, "log_small", kd), (cls, k, kd)
            n += 1
    assert n >= 8


def test_guard_fixed_ends(fx):
    """A fixed end gives exactly zero blocks on its side and leaves the free side's block bit for bit unchanged."""
    n = 0
    for cls, k in _all_edges(fx):
        fa, fb = bool(fx[cls + "/fixed_a"][k]), bool(fx[cls + "/fixed_b"][k])
        if not (fa or fb):
            continue
        D, NA, _ = EB.DIMS[cls]
        B, _ = EB.fixture_edge_blocks(fx, cls, k)
        info = fx[cls + "/info"][k].reshape(D, D)
        w = EB.robustify(int(fx[cls + "/rk_kind"][k]), float(fx[cls + "/rk_delta"][k]), float(fx[cls + "/e"][k] @ info @ fx[cls + "/e"][k]))[1]
        F = EB.edge_blocks(fx[cls + "/e"][k], fx[cls + "/J"][k], info, NA, w)
        Haa, Hbb, Hab, ba, bb = B
        assert not np.any(Hab)
        if fa:
            assert not np.any(Haa) and not np.any(ba) and np.array_equal(Hbb, F[1]) and np.array_equal(bb, F[4]) and np.any(Hbb)
        else:
            assert not np.any(Hbb) and not np.any(bb) and np.array_equal(Haa, F[0]) and np.array_equal(ba, F[3]) and np.any(Haa)
        n += 1
    assert n == 12


# ---- fixture and generator cannot drift apart -------------------------------------------------------------------------------------------
def test_generator_regenerates_stored_edges(fx):
    """Three edges per class evaluated again with mpmath from the stored inputs equal the stored e and J to 1e-15 relative."""
    pytest.importorskip("mpmath")
    spec = importlib.util.spec_from_file_location("make_edge_golden", os.path.join(ROOT, "tools", "make_edge_golden.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    for cls in EB.CLASSES:
        n = len(fx[cls + "/a"])
        for k in (0, n // 2, n - 1):
            e, J, info = gen.evaluate_edge(fx, cls, k)
            assert np.abs(e - fx[cls + "/e"][k]).max() <= 1e-15 * np.abs(e).max()
            assert np.abs(J - fx[cls + "/J"][k]).max() <= 1e-15 * np.abs(J).max()
            if cls == "cub":
                assert info["win"] == fx["cub/win"][k] and abs(info["lead"] - fx["cub/lead"][k]) <= 1e-15 * abs(info["lead"])
