"""The Sim(3) RANSAC WITHOUT a GPU: (a) the conditions under which the float64 numpy statement (tests/sim3_ransac_ref.py) may be compared
with anything, for every hypothesis it evaluates on every pair of every batch tests/test_sim3_ransac_gpu.py runs
(tests/sim3_ransac_cases.py), none dropped; (b) that the hard batch holds the selection cases it is there for; (c) the closed-form draws
of cs_sim3_ransac_triplets against draws from real lists; (d) cube_slam_wu_amd/csrc/cs_sim3_ransac.h -- the routines the kernel runs --
built with g++ into tools/hostonly/sim3_ransac_host_check.cpp, run over the dumped batches and held to the reference; (e) the same
program under the address and undefined-behaviour sanitizers, stand-alone.

Why the conditions: a match whose squared error is within rounding of its threshold is classified by rounding, and a count, a winner and
everything after it may then differ between two correct evaluations.  So for every hypothesis evaluated and every match, float64 and long
double must classify alike and |err64 - errld| <= |err64 - threshold| / 100.  Measured here (printed by the tests):
  easy batch        0 flips, worst |err64 - errld| / |err64 - threshold| 6.4e-11, smallest margin |err / threshold - 1| 2.6e-3
  hard batch        0 flips, worst 3.0e-11, smallest margin 1.1e-2; winners at hypotheses 45, 220, 9, 107; exhausted at 149 and at 300
  variants          0 flips, worst 4.0e-12, smallest margin 2.3e-2
  degenerate batch  0 flips, worst 3.3e-12, smallest margin 4.7e-2
The reference's own float64-against-long-double deviation of a handed-out S12 is at most 4.9e-15 of its largest entry.

Contract of (d), as of the GPU tests: found, hyp, iterations, n_inliers and the flags identical; S12 within max(100 x the reference's own
float64-against-long-double deviation of that pair's S12, 1e-13), relative to the pair's largest entry."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from cube_slam_wu_amd import capi
from cube_slam_wu_amd import synth_sim3_ransac as sr
import sim3_ransac_cases as pc
import sim3_ransac_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "hostonly", "sim3_ransac_host_check.cpp")


@pytest.mark.parametrize("name", pc.NAMES)
def test_reference_is_comparable(name):
    res = pc.run(name)
    flips, differ = sum(r["flips"] for r in res), sum(r["refusals_differ"] for r in res)
    worst, margin, dev = max(r["worst_ratio"] for r in res), min(r["min_margin"] for r in res), max(r["dev"] for r in res)
    print("%s: %d hypotheses evaluated, %d flips, %d refusals that differ, worst |err64 - errld| / |err64 - threshold| %.3g, smallest margin %.3g, S12 deviation %.3g"
          % (name, sum(len(r["counts"]) for r in res), flips, differ, worst, margin, dev))
    assert flips == 0 and differ == 0
    assert worst <= 1.0 / 100


def test_easy_batch_runs_what_it_should():
    b, res = pc.easy_batch(), pc.run("easy")
    counts = np.diff(b["match_ptr"]).tolist()
    assert counts == list(pc.EASY_COUNTS) and {pc.CHUNK - 1, pc.CHUNK, pc.CHUNK + 1, 2 * pc.CHUNK + 1} <= set(counts)
    assert np.array_equal(b["fix_scale"], np.arange(len(counts)) % 2) and not b["is_mismatch"].any()
    for n, r in zip(counts, res):
        if n < 20:      # not run at min_inliers = 20
            assert (r["found"], r["hyp"], r["iterations"], r["n_inliers"]) == (0, -1, 0, 0) and not r["inlier"].any() and np.array_equal(r["S12"], ref.IDENTITY)
    assert res[2]["max_its"] == 1 and sum(r["found"] for r in res) >= 8


def test_hard_batch_holds_its_selection_cases():
    b, res = pc.hard_batch(), pc.run("hard")
    assert np.diff(b["match_ptr"]).tolist() == list(pc.HARD_COUNTS)
    print([(r["found"], r["hyp"], r["iterations"], r["n_inliers"]) for r in res])
    assert any(r["found"] and 64 <= r["hyp"] < 128 for r in res)
    assert any(r["found"] and r["hyp"] >= 128 for r in res)
    assert any(not r["found"] and r["iterations"] == 300 for r in res)                       # a partial last block: 300 = 4 x 64 + 44
    assert not res[0]["found"] and res[0]["iterations"] == 149                               # 64 matches: the eps rule
    tie = False
    for r in res:
        c = np.array(r["counts"])
        if not r["found"] and (c == c.max()).sum() >= 2:
            assert r["hyp"] == np.flatnonzero(c == c.max())[-1] and r["n_inliers"] == c.max()
            tie = True
    assert tie
    for name, m in pc.VARIANTS.items():
        for r, full in zip(pc.run(name), res):
            assert r["iterations"] == (full["iterations"] if full["found"] and full["iterations"] <= m else min(m, full["max_its"]))


def test_degenerate_batch_is_what_it_says():
    b, res = pc.degenerate_batch(), pc.run("degenerate")
    ptr = b["match_ptr"]
    assert np.diff(ptr).tolist() == [40, 0, 65, 3, 3, 40]
    assert (res[1]["found"], res[1]["hyp"], res[1]["iterations"]) == (0, -1, 0)
    assert (res[3]["found"], res[3]["hyp"], res[3]["n_inliers"]) == (0, -1, 0) and res[3]["iterations"] == res[3]["max_its"] > 1
    assert all(c == -1 for c in res[3]["counts"]) and np.array_equal(res[3]["S12"], ref.IDENTITY)
    assert (res[4]["found"], res[4]["hyp"], res[4]["n_inliers"]) == (1, 0, 3)
    assert res[5]["found"] and np.all(np.isfinite(res[5]["S12"])) and not res[5]["inlier"][7] and not res[5]["inlier"][11]
    assert res[0]["found"] and res[2]["found"] and res[2]["S12"][7] == 1.0


def test_budget_follows_the_eps_rule():
    assert ref.budget(64, 0.99, 20, 300) == 149 and ref.budget(19, 0.99, 20, 300) == 0 and ref.budget(20, 0.99, 20, 300) == 1
    assert ref.budget(2, 0.99, 0, 300) == 0 and ref.budget(3, 0.99, 0, 300) == 300 and ref.budget(10 ** 6, 0.99, 1, 1024) == 1024
    assert ref.budget(257, 0.99, 20, 300) == 300 and ref.budget(21, 0.99, 20, 300) == 3


def test_closed_form_draws_equal_the_draws_from_lists():
    for n in list(range(3, 71)) + [1000, 100000]:
        seed = ref.splitmix64(n) | 1
        got = capi.sim3_ransac_triplets(seed, n, 300)
        want = np.array([ref.draw(seed, h, n) for h in range(300)])
        assert np.array_equal(got, want), n
        assert got.min() >= 0 and got.max() < n
        assert np.all(got[:, 0] != got[:, 1]) and np.all(got[:, 0] != got[:, 2]) and np.all(got[:, 1] != got[:, 2])
    assert capi.lib().cs_sim3_ransac_triplets(1, 2, 1, capi._ip(np.zeros(3, np.int32))) == -1      # CS_ERR_INVALID_ARG


# ---------------------------------------------------------------- (d), (e): the host build of cs_sim3_ransac.h
def _dump(path, batch, prm):
    sr.write_dump(path, batch, prm["probability"], prm["min_inliers"], prm["max_iterations"])


def _parse_run(text):
    rows, inl = [], []
    for line in text.splitlines():
        w = line.split()
        if w and w[0] == "pair":
            rows.append([float(x) for x in w[2:]])
        elif w and w[0] == "inl":
            inl.append(np.array([int(c) for c in (w[2] if len(w) > 2 else "")], np.uint8))
    rows = np.array(rows).reshape(-1, 12)
    return dict(found=rows[:, 0].astype(int), hyp=rows[:, 1].astype(int), iterations=rows[:, 2].astype(int), n_inliers=rows[:, 3].astype(int), S12=rows[:, 4:],
                inlier=np.concatenate(inl) if inl else np.zeros(0, np.uint8))


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("sim3_ransac_dumps")
    out = {}
    for name in pc.NAMES:
        out[name] = str(d / (name + ".txt"))
        _dump(out[name], pc.batch_of(name), pc.params_of(name))
    return out


def _build(exe, extra):
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall"] + extra + [SRC, "-o", str(exe)])


def _run(exe, args):
    out = subprocess.run([str(exe)] + args, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().splitlines()[-1] == "sim3_ransac_host_check: ok"
    return out.stdout


def _check(exe, dumps, names, what):
    for name in names:
        got = _parse_run(_run(exe, ["run", dumps[name]]))
        pc.compare_with_reference(got, pc.run(name), "%s %s" % (what, name))
        ptr = pc.batch_of(name)["match_ptr"]
        assert got["n_inliers"].tolist() == [int(got["inlier"][ptr[f]:ptr[f + 1]].sum()) for f in range(len(ptr) - 1)]


def test_host_build_of_the_shared_header_against_the_reference(tmp_path, dumps):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "sim3_ransac_host_check"
    _build(exe, ["-O2"])
    _check(exe, dumps, pc.NAMES, "host")
    rows = np.array([[float(x) for x in line.split()[1:]] for line in _run(exe, ["hyp", str(pc.HYPOTHESES_COUNT), dumps["hard"]]).splitlines() if line.startswith("hyp ")])
    rows = rows[rows[:, 0] == pc.HYPOTHESES_PAIR]
    assert np.array_equal(rows[:, 1], np.arange(pc.HYPOTHESES_COUNT))
    pc.compare_hypotheses(rows[:, 2].astype(int), rows[:, 3:], "host, every hypothesis of hard pair %d" % pc.HYPOTHESES_PAIR)


def test_host_build_runs_clean_under_asan_and_ubsan_stand_alone(tmp_path, dumps):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "sim3_ransac_host_check_san"
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    _check(exe, dumps, ("easy", "hard", "degenerate"), "host, sanitized")
    _run(exe, ["hyp", "70", dumps["degenerate"]])
