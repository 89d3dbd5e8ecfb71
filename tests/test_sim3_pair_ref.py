"""The Sim(3) pair alignment WITHOUT a GPU: (a) the conditions under which the float64 numpy statement (tests/sim3_pair_ref.py) may be
compared with anything, for every pair of every batch tests/test_sim3_pair_gpu.py runs (tests/sim3_pair_cases.py), none dropped;
(b) cube_slam_wu_amd/csrc/cs_sim3_pair.h -- the per-pair routine the kernel runs -- built with g++ into
tools/hostonly/sim3_pair_host_check.cpp, run over the dumped batches and held to the reference; (c) the same program under the address and
undefined-behaviour sanitizers, stand-alone.

Why the conditions: both edges' Jacobians are central differences over 2e-9, so H carries a relative rounding noise of ~1e-7 in any
precision.  A trial whose rho is within that noise of 0, or a match whose chi2 is within it of th2, is decided by rounding: float64 and
long double -- and a device whose libm differs by an ulp -- may then run different trials or classify differently, and nothing can be
compared.  Measured here (float64 against long double; printed by the tests):
  main batch, 96 pairs, schedule (3, 2):  same trials, min |rho| 4.6e-3, smallest margin |chi2 / th2 - 1| 1.6e-4, states within 4.4e-7
  the three parameter variants:           same trials, min |rho| 6.2e-4, margins >= 1.6e-3, states within 4.2e-8
  default schedule (5, then 10 or 5):     LM reaches the rounding floor (|rho| down to 2.5e-13) and the trial counts differ between the
                                          precisions; inlier sets identical, margin 1.2e-4, states within 1.2e-7
  dense batch, 24 pairs, schedule (3, 2): same trials, min |rho| 0.12, smallest margin 2.8e-4, states within 1.1e-7
The dense batch and the dense edge batch (tests/sim3_pair_cases.py) give every pair its own two cameras with fx != fy and every edge its
own dense 2 x 2 information: the generator's batches share one camera pair with fx == fy and weigh every edge by a scalar.
A clean pair (no match removed after round one) solves the same problem again in round two, so the variant with clean pairs runs a first
round of 2 iterations: its second round then still has something to gain (|rho| >= 6.2e-4) and is held to the same conditions as the rest.

Contract of (b), as of the GPU tests: iterations_done and inlier flags identical, states and chi2 within 1e-5 relative; the edge blocks
within 100 x (errors, floor 1e-13) and 10 x (Jacobians) of the reference's own float64-against-long-double deviation."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from cube_slam_wu_amd import synth_sim3_pairs as sp
import sim3_pair_cases as pc
import sim3_pair_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "hostonly", "sim3_pair_host_check.cpp")


@pytest.mark.parametrize("name", ["main", "dense"] + list(pc.VARIANTS))
def test_reference_is_comparable_at_the_short_schedule(name):
    k = pc.comparable(name)
    print(name, k)
    assert k["same_trials"] and k["same_inliers"]
    assert k["min_abs_rho"] > 1e-6 and k["min_margin"] > 1e-6 and k["state_dev"] < 1e-6


def test_variant_batch_has_clean_pairs_and_pairs_that_lose_matches():
    res = pc.run("clean_and_outlier_counts")
    its = [tuple(r["iterations"]) for r in res]
    clean = [r["n_inliers"] == len(r["inlier"]) for r in res]
    assert (2, 1) in its and (2, 2) in its and sum(clean) == 4
    assert all(it == ((2, 1) if c else (2, 2)) for it, c, r in zip(its, clean, res) if r["n_inliers"] > 0)


def test_dense_batch_tells_its_fields_apart_and_still_runs_second_rounds():
    b, plain = pc.dense_batch(), sp.synth_sim3_pairs(24, np.diff(pc.dense_batch()["match_ptr"]), 0.1, pc.DENSE_SEED, pc.START)
    assert set(np.diff(b["match_ptr"]).tolist()) == set(pc.COUNTS) and len(b["S12"]) == 24
    assert np.all(plain["intr"] == np.concatenate([sp.INTR_CAM1, sp.INTR_CAM2]))      # what the builders start from
    K = b["intr"]
    assert np.all(np.abs(K[:, [1, 5]] / K[:, [0, 4]] - 1) >= 0.02) and all(len(np.unique(K[:, k])) == 24 for k in range(8))
    for key in ("info12", "info21"):
        W = b[key].reshape(-1, 2, 2)
        ev = np.linalg.eigvalsh(W)
        assert np.all(W[:, 0, 1] == W[:, 1, 0]) and np.all(W[:, 0, 1] != 0) and ev.min() > 0
        assert np.all(ev[:, 1] / ev[:, 0] <= 5 * (1 + 1e-12)) and (ev[:, 1] / ev[:, 0]).max() > 2.5
    assert not np.array_equal(b["info12"], b["info21"])
    # the keypoints moved with the cameras: the errors at the true state are what they were, to within what 2 cm of noise on a point 3 m
    # away make of a focal length changed by up to 11 % (80 px * 0.015 = 1.2 px)
    for f in (0, 7, 23):
        e0, e1 = ref.errors(ref.pair_of(plain, f), plain["S12_true"][f]), ref.errors(ref.pair_of(b, f), b["S12_true"][f])
        assert np.allclose(e0[0], e1[0], rtol=0, atol=1.5) and np.allclose(e0[1], e1[1], rtol=0, atol=1.5)
    res = pc.run("dense")
    second = sum(r["iterations"][1] > 0 for r in res)
    print("pairs that run a second round: %d of 24" % second)
    assert 2 * second >= len(res) and any(r["n_inliers"] == 0 for r in res)
    e = pc.dense_edge_batch()
    assert np.array_equal(np.diff(e["match_ptr"]), [12, 12, 12, 12]) and len(np.unique(e["intr"])) == 32
    (e64, j64), (p64, q64) = pc.edge_blocks(False, True), pc.edge_blocks()
    assert np.all(e64 != p64) and np.all(np.abs(j64 - q64).reshape(48, -1).max(-1) > 0.1)


def test_reference_at_the_default_schedule_agrees_where_rounding_cannot_decide():
    k = pc.comparable("default")
    print("default", k)
    assert k["same_inliers"] and k["min_margin"] > 1e-6 and k["state_dev"] < 1e-6


def test_reference_edge_blocks_have_an_exactly_zero_scale_column_under_fix_scale():
    b = pc.edge_batch()
    (e64, j64), (eld, jld) = pc.edge_blocks(), pc.edge_blocks(True)
    fs = np.repeat(b["fix_scale"].astype(bool), np.diff(b["match_ptr"]))
    assert fs.sum() == 12 and np.all(j64[fs][..., 6] == 0) and np.all(jld[fs][..., 6] == 0)
    # (a free scale moves e21 only: exp(sigma e_6) * S scales S.map(P) as a whole, which project() does not see)
    assert np.all(j64[~fs][:, 1, :, 6] != 0)
    print("reference's own deviation: err %.3g, jac %.3g" % (ref.block_deviation(e64, eld).max(), ref.block_deviation(j64, jld).max()))


# ---------------------------------------------------------------- (b), (c): the host build of cs_sim3_pair.h
def _dump(path, batch, prm):
    n, N = len(batch["S12"]), int(batch["match_ptr"][-1])
    g = lambda v: " ".join("%.17g" % float(x) for x in np.ravel(v))
    with open(path, "w") as f:
        f.write("%d %d\n" % (n, N))
        f.write("%d %d %d %d %d %.17g %.17g\n" % (prm["iterations_first"], prm["iterations_more_clean"], prm["iterations_more_outliers"], prm["robust_second_round"],
                                                 prm["min_inliers"], prm["th2"], prm["huber_delta"]))
        for i in range(n):
            f.write("%s %s %d %d %d\n" % (g(batch["S12"][i]), g(batch["intr"][i]), int(batch["fix_scale"][i]), int(batch["match_ptr"][i]), int(batch["match_ptr"][i + 1])))
        for m in range(N):
            f.write("%s\n" % g(np.concatenate([batch["P1"][m], batch["P2"][m], batch["obs1"][m], batch["obs2"][m], batch["info12"][m], batch["info21"][m]])))


def _parse_opt(text, batch):
    S, its, chi, n_in, inl = [], [], [], [], []
    for line in text.splitlines():
        w = line.split()
        if w and w[0] == "pair":
            its.append([int(w[2]), int(w[3])]); n_in.append(int(w[4])); chi.append([float(w[5]), float(w[6])]); S.append([float(x) for x in w[7:15]])
        elif w and w[0] == "inl":
            inl.append(np.array([int(c) for c in (w[2] if len(w) > 2 else "")], np.uint8))
    return dict(S12=np.array(S).reshape(-1, 8), iterations=np.array(its).reshape(-1, 2), chi2=np.array(chi).reshape(-1, 2), n_inliers=np.array(n_in),
                inlier=np.concatenate(inl) if inl else np.zeros(0, np.uint8))


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("sim3_pair_dumps")
    out = {}
    for name in ["main", "default", "dense"] + list(pc.VARIANTS):
        batch = pc.main_batch() if name == "main" else pc.default_batch() if name == "default" else pc.dense_batch() if name == "dense" else pc.variant_pairs(name)
        prm = ref.params(**(pc.SHORT if name == "main" else {} if name == "default" else pc.DENSE if name == "dense" else pc.VARIANTS[name]))
        out[name] = str(d / (name + ".txt"))
        _dump(out[name], batch, prm)
    out["edge"] = str(d / "edge.txt")
    _dump(out["edge"], pc.edge_batch(), ref.params())
    out["dense_edge"] = str(d / "dense_edge.txt")
    _dump(out["dense_edge"], pc.dense_edge_batch(), ref.params())
    return out


def _build(exe, extra):
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall"] + extra + [SRC, "-o", str(exe)])


def _run(exe, mode, dump):
    out = subprocess.run([str(exe), mode, dump], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().splitlines()[-1] == "sim3_pair_host_check: ok"
    return out.stdout


def test_host_build_of_the_shared_header_against_the_reference(tmp_path, dumps):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "sim3_pair_host_check"
    _build(exe, ["-O2"])
    for name in ["main", "dense"] + list(pc.VARIANTS):
        pc.compare_with_reference(_parse_opt(_run(exe, "opt", dumps[name]), None), pc.run(name), "host " + name)
    # the default schedule: LM reaches the rounding floor, iteration counts cannot be compared (see the head of this file)
    pc.compare_with_reference(_parse_opt(_run(exe, "opt", dumps["default"]), None), pc.run("default"), "host default", iterations=False)
    # the edge blocks, of the generator's batch and of the one with per-pair, per-camera intrinsics
    for dense in (False, True):
        rows = np.array([[float(x) for x in line.split()[2:]] for line in _run(exe, "lin", dumps["dense_edge" if dense else "edge"]).splitlines() if line.startswith("lin ")])
        err, jac = rows[:, :4], rows[:, 4:].reshape(-1, 2, 2, 7)
        (e64, j64), (eld, jld) = pc.edge_blocks(False, dense), pc.edge_blocks(True, dense)
        fs = np.repeat(pc.edge_batch()["fix_scale"].astype(bool), np.diff(pc.edge_batch()["match_ptr"]))
        assert np.all(jac[fs][..., 6] == 0)
        for nm, got, r64, rld, factor, floor in (("err", err, e64, eld, 100, 1e-13), ("jac", jac, j64, jld, 10, 0.0)):
            ref_dev, dev = ref.block_deviation(r64, rld).max(), ref.block_deviation(got, r64).max()
            tol = max(factor * ref_dev, floor)
            print("%s%s: host %.3g, reference's own %.3g, tolerance %.3g" % (nm, " (distinct intrinsics)" if dense else "", dev, ref_dev, tol))
            assert dev <= tol, (nm, dense, dev, tol)


def test_host_build_runs_clean_under_asan_and_ubsan_stand_alone(tmp_path, dumps):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "sim3_pair_host_check_san"
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    plain = _parse_opt(_run(exe, "opt", dumps["main"]), None)
    pc.compare_with_reference(plain, pc.run("main"), "host main, sanitized")
    pc.compare_with_reference(_parse_opt(_run(exe, "opt", dumps["dense"]), None), pc.run("dense"), "host dense, sanitized")
    _run(exe, "lin", dumps["edge"])
    _run(exe, "lin", dumps["dense_edge"])
