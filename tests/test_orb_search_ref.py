"""The guided ORB matcher WITHOUT a GPU: (a) the conditions under which the float64 numpy statement (tests/orb_search_ref.py) may be
compared with anything, for EVERY query of every batch tests/test_orb_search_gpu.py runs (tests/orb_search_cases.py), none dropped; (b)
that the batches hold what they are there for -- the counts around the 64-query chunk, every status in the crowded batch, the planted
Hamming ties, the keypoints that are off the grid; (c) cube_slam_wu_amd/csrc/cs_orb_search.h -- the routines the kernel runs, behind the
grid build the C ABI does -- built with g++ into tools/hostonly/orb_search_host_check.cpp, run over the dumped batches and held to the
reference; (d) the same program under the address and undefined-behaviour sanitizers, stand-alone; (e) cs_orb_search_jobs without a
device, and cs_orb_search_mutual, which needs none.

Why the conditions: a quantity within rounding of the threshold it is compared with is decided by rounding, and a status, a candidate set
and a best index may then differ between two correct evaluations.  So for every query float64 and long double must give the same status,
best_idx, best_dist, level, n_window and n_candidates, must have made the same comparisons, and for every comparison made
|d64 - dld| <= |d64| / 100, d = lhs - rhs; a keypoint's cell is held to the same with d = the distance of floor's argument to the nearer
integer.  Measured here (printed by the tests):
  easy     596 queries,  8889 comparisons, 0 flips, worst |d64 - dld| / |d64| 1.0e-11, smallest |d64| 1.1e-5 (scale[l] < ratio), inspection outputs' own deviation 2.9e-15
  crowded  400 queries, 29755 comparisons, 0 flips, worst 3.9e-11, smallest |d64| 1.4e-3 (scale[l] < ratio), inspection outputs' own deviation 1.5e-15
  single     1 query,      20 comparisons, 0 flips, worst 2.8e-15, inspection outputs' own deviation 1.2e-16
  two_way  400 queries, 29925 comparisons, 0 flips, worst 7.0e-12, smallest |d64| 1.0e-3 (a keypoint's cell)

Contract of (c): every integer output identical, and u, v, ur, dist, radius the reference's float64 BITS (the g++ build and numpy do the
same IEEE operations in the same order)."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from cube_slam_wu_amd import capi
from cube_slam_wu_amd import synth_orb_search as so
import orb_search_cases as pc
import orb_search_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "hostonly", "orb_search_host_check.cpp")
ALL = pc.NAMES + ("two_way",)


@pytest.mark.parametrize("name", ALL)
def test_reference_is_comparable(name):
    res = pc.run(name)
    print("%s: %d queries, %d comparisons, %d flips, worst |d64 - dld| / |d64| %.3g, smallest |d64| %.3g (%s), inspection outputs' own deviation %.3g"
          % (name, len(res["status"]), res["n_comparisons"], res["flips"], res["worst_ratio"], res["min_gap"][0], res["min_gap"][1], res["dev"].max()))
    assert res["flips"] == 0                               # the cap on dropped queries is zero: every query of the batch is held to this
    assert res["worst_ratio"] <= 1.0 / 100


def test_easy_batch_runs_what_it_should():
    b, res = pc.easy_batch(), pc.run("easy")
    counts = np.diff(b["query_ptr"]).tolist()
    assert counts == list(pc.EASY_COUNTS) and {0, 1, pc.CHUNK - 1, pc.CHUNK, pc.CHUNK + 1, 2 * pc.CHUNK + 1} <= set(counts)
    assert np.diff(b["kp_ptr"]).tolist() == list(pc.EASY_FRAME_KEYPOINTS) and {0, 1, 65} <= set(pc.EASY_FRAME_KEYPOINTS)
    assert set(b["flags"].tolist()) == {so.FUSE, so.FUSE_SIM3, so.SEARCH_BY_SIM3} and set(b["pose8"][:, 7].tolist()) > {1.0}
    assert np.all(b["grid"] == (64, 48))
    stereo_kp = b["kp"][:, 2] >= 0
    assert stereo_kp.sum() > 50 and (~stereo_kp).sum() > 50             # keypoints with and without a right-image coordinate
    jq = res["job_of_query"]
    assert np.all(res["status"][(jq == 6) & (b["skip"] == 0)] != ref.OK) and res["n_window"][jq == 6].sum() == 0      # the frame without keypoints
    assert res["n_ok"][[2, 3, 4, 5, 8, 9]].min() >= 5 and (res["status"] == ref.OK).sum() > 150
    ok = res["status"] == ref.OK
    mine = ok & (b["truth"] >= 0)
    assert np.array_equal(res["best_idx"][mine], b["truth"][mine]) and mine.sum() > 140      # what is matched at all is matched to the point's own keypoint
    assert np.all(res["level"][np.isin(res["status"], (ref.SKIPPED, ref.BEHIND, ref.OUT_OF_IMAGE, ref.OUT_OF_RANGE, ref.VIEW_ANGLE))] == ref.LEVEL_NONE)
    assert np.all(res["level"][np.isin(res["status"], (ref.OK, ref.NO_CANDIDATE, ref.TOO_FAR))] < so.N_LEVELS)
    assert set(np.unique(res["level"][ok]).tolist()) >= {0, 1, 2, 3}


def test_crowded_batch_holds_every_status_and_wide_windows():
    b, res = pc.crowded_batch(), pc.run("crowded")
    assert np.all(b["grid"] == pc.CROWDED_GRID)
    print("crowded: statuses %s, keypoints in a window on average %.2f, at most %d; candidates at most %d" % (np.bincount(res["status"], minlength=8).tolist(), res["n_window"].mean(),
                                                                                                             res["n_window"].max(), res["n_candidates"].max()))
    assert set(np.unique(res["status"]).tolist()) == set(range(8))      # every status occurs
    assert res["n_window"].max() >= 10 and res["n_candidates"].max() >= 4
    counts = np.bincount(res["cells"][0][res["cells"][0] >= 0], minlength=12)
    assert np.median(counts) >= 8 and counts.max() >= 20                # cells hold many keypoints
    assert (res["cells"][0] < 0).sum() >= 10                            # and a strip along the right and bottom border holds keypoints that are in no cell
    jq = res["job_of_query"]
    for j in range(len(pc.CROWDED_JOBS)):                               # one wave holds several statuses at once
        a = int(b["query_ptr"][j])
        assert len(np.unique(res["status"][a:a + pc.CHUNK])) >= 5, j
    assert not np.any((res["status"] == ref.VIEW_ANGLE) & (b["flags"][jq] == so.SEARCH_BY_SIM3))


def test_planted_ties_resolve_to_the_walk_order_winner():
    """Two candidates at the SAME Hamming distance 12: in different cell columns and in different rows of one column the winner, the first
    in walk order, is the keypoint with the LARGER index in the frame (an `argmin over the index` would take the other one); within one
    cell the walk order IS the index order, so there the smaller index wins -- that case holds a `<=` in place of the strict `<` apart."""
    b, res = pc.crowded_batch(), pc.run("crowded")
    assert b["ties"][:, 3].tolist() == [0, 1, 2]
    cell = res["cells"][0]
    rows = pc.CROWDED_GRID[1]
    for q, win, lose, kind in b["ties"]:
        assert res["status"][q] == ref.OK and res["best_dist"][q] == 12 and res["n_candidates"][q] >= 2
        assert ref.hamming(b["qdesc"][q], b["desc"][[win, lose]]).tolist() == [12, 12]
        assert res["best_idx"][q] == win, (kind, res["best_idx"][q])
        cw, cl = divmod(int(cell[win]), rows), divmod(int(cell[lose]), rows)
        if kind == 0:
            assert cw[0] + 1 == cl[0] and cw[1] == cl[1] and win > lose
        elif kind == 1:
            assert cw[0] == cl[0] and cw[1] + 1 == cl[1] and win > lose
        else:
            assert cw == cl and win < lose


def test_off_grid_keypoints_are_matched_by_nobody():
    """A keypoint whose rounded cell is column `cols` or row `rows` is in no cell: it carries exactly the query's descriptor, lies inside the
    query's window, and the match goes to a decoy 20 bits away."""
    b, res = pc.crowded_batch(), pc.run("crowded")
    cols, rows = pc.CROWDED_GRID
    assert len(b["offgrid"]) == 2
    for (q, off, decoy), axis in zip(b["offgrid"], (0, 1)):
        assert res["cells"][0][off] == -1 and res["cell_floors"][0][axis][off] == (cols, rows)[axis]
        assert ref.brute_force_nearest(b, q, res["radius"][q], res["u"][q], res["v"][q]) == (off, 0)      # the nearest descriptor inside the window
        assert res["status"][q] == ref.OK and res["best_idx"][q] == decoy and res["best_dist"][q] == 20
    off_grid = np.flatnonzero(res["cells"][0] < 0)
    assert not np.isin(res["best_idx"][res["best_idx"] >= 0], off_grid).any()      # by nobody, in any job over the frame


def test_two_way_batch_and_mutual_matches():
    b, res = pc.two_way_batch(), pc.run("two_way")
    ptr = b["query_ptr"]
    assert np.diff(ptr).tolist() == np.diff(b["kp_ptr"]).tolist()
    best12, st12, best21, st21 = res["best_idx"][:ptr[1]], res["status"][:ptr[1]], res["best_idx"][ptr[1]:], res["status"][ptr[1]:]
    want = ref.mutual(best12, st12, best21, st21)
    got = capi.orb_search_mutual(best12, st12, best21, st21)            # plain host code: runs without a device
    assert np.array_equal(got, want)
    one_way = (st12 == ref.OK).sum()
    print("two_way: %d OK from keyframe 0, %d from keyframe 1, %d mutual" % (one_way, (st21 == ref.OK).sum(), (want >= 0).sum()))
    assert 40 < (want >= 0).sum() < one_way                             # at least one one-directional OK is rejected
    both = np.flatnonzero(want >= 0)
    assert np.array_equal(want[both], b["truth"][:ptr[1]][both])        # what both directions agree on is the point's own pair of keypoints
    L = capi.lib()
    n = C.c_int(5)
    out = np.full(3, 7, np.int32)
    i3, u3 = np.zeros(3, np.int32), np.zeros(3, np.uint8)
    assert L.cs_orb_search_mutual(3, None, capi._u8p(u3), 3, capi._ip(i3), capi._u8p(u3), capi._ip(out), C.byref(n)) == -1
    assert L.cs_orb_search_mutual(-1, capi._ip(i3), capi._u8p(u3), 3, capi._ip(i3), capi._u8p(u3), capi._ip(out), C.byref(n)) == -1
    assert np.all(out == 7) and n.value == 5
    assert L.cs_orb_search_mutual(3, capi._ip(np.array([0, 5, -1], np.int32)), capi._u8p(u3), 1, capi._ip(i3), capi._u8p(u3), capi._ip(out), C.byref(n)) == 0
    assert out.tolist() == [0, -1, -1] and n.value == 1                 # an index outside 0 .. n2 - 1 is no match


# ---------------------------------------------------------------- (c), (d): the host build of cs_orb_search.h
def _params_list(prm):
    return [prm[k] for k in ref.PARAM_KEYS]


def _parse_run(text):
    rows, jobs, frames = [], [], []
    for line in text.splitlines():
        w = line.split()
        if w and w[0] == "q":
            rows.append([float(x) for x in w[1:]])
        elif w and w[0] == "job":
            jobs.append([int(x) for x in w[1:]])
        elif w and w[0] == "frame":
            frames.append([int(x) for x in w[1:]])
    rows, jobs, frames = np.array(rows).reshape(-1, 12), np.array(jobs, np.int64).reshape(-1, 2), np.array(frames, np.int64).reshape(-1, 2)
    assert np.array_equal(rows[:, 0], np.arange(len(rows))) and np.array_equal(jobs[:, 0], np.arange(len(jobs)))
    return dict(status=rows[:, 1].astype(int), best_idx=rows[:, 2].astype(int), best_dist=rows[:, 3].astype(int), level=rows[:, 4].astype(int), n_window=rows[:, 5].astype(int),
                n_candidates=rows[:, 6].astype(int), insp5=rows[:, 7:12], n_ok=jobs[:, 1], n_in_a_cell=frames[:, 1])


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    d = tmp_path_factory.mktemp("orb_search_dumps")
    out = {}
    for name in ALL:
        out[name] = str(d / (name + ".txt"))
        so.write_dump(out[name], pc.batch_of(name), _params_list(pc.params_of(name)))
    return out


def _build(exe, extra):
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall"] + extra + [SRC, "-o", str(exe)])


def _run(exe, args):
    out = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert out.stdout.strip().splitlines()[-1] == "orb_search_host_check: ok"
    return out.stdout


def _check(exe, dumps, what):
    for name in ALL:
        got = _parse_run(_run(exe, ["run", dumps[name]]))
        res = pc.run(name)
        pc.compare_with_reference(got, res, "%s %s" % (what, name), inspect=True, exact=True)
        assert got["n_in_a_cell"].tolist() == [int((c >= 0).sum()) for c in res["cells"]]


def test_host_build_of_the_shared_header_against_the_reference(tmp_path, dumps):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "orb_search_host_check"
    _build(exe, ["-O2"])
    _check(exe, dumps, "host")
    assert "ms per pass over 3 jobs, 400 queries" in _run(exe, ["time", "2", dumps["crowded"]])


def test_host_build_runs_clean_under_asan_and_ubsan_stand_alone(tmp_path, dumps):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "orb_search_host_check_san"
    _build(exe, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    _check(exe, dumps, "host, sanitized")


def test_refuses_to_run_without_a_device():
    L = capi.lib()
    if L.cs_device_count() > 0:
        return
    b = pc.single_batch()
    nf, N, keep_f, fargs = capi._orb_frame_inputs(b)
    nj, Q, keep_j, jargs = capi._orb_job_inputs(b)
    p = capi.orb_search_default_params()
    st, lv, bi, bd, ok = np.full(Q, 9, np.uint8), np.full(Q, 9, np.uint8), np.full(Q, 77, np.int32), np.full(Q, 77, np.int32), np.full(nj, 77, np.int32)
    rc = L.cs_orb_search_jobs(0, C.byref(p), nf, *fargs, nj, *jargs, capi._u8p(st), capi._ip(bi), capi._ip(bd), capi._u8p(lv), capi._ip(ok))
    assert rc == -3                                        # CS_ERR_NO_DEVICE: no CPU fallback
    assert "no CPU fallback" in capi.last_error()
    assert np.all(st == 9) and np.all(bi == 77) and np.all(ok == 77)
    h = C.c_void_p()
    assert L.cs_orb_search_create(0, C.byref(h)) == -3 and not h


def test_default_params_are_fuse():
    p = capi.orb_search_default_params()
    assert [getattr(p, k) for k in ref.PARAM_KEYS] == [ref.params()[k] for k in ref.PARAM_KEYS]
    with pytest.raises(KeyError):
        capi.orb_search_default_params(no_such_field=1)
    assert capi.ORB_STATUS == {k: i for i, k in enumerate(ref.STATUS_NAMES)}
    assert capi.ORB_FLAGS == dict(CHECK_VIEW=ref.CHECK_VIEW, CHECK_REPROJ=ref.CHECK_REPROJ)
    assert (so.FUSE, so.FUSE_SIM3, so.SEARCH_BY_SIM3) == (3, 1, 0)
