"""What the cases of line_setup_cases.py promise, from its float64 statement of merge_break_lines alone (no device): the segments inside
every ROI, the size class that picks the kernel instance, the number of merges, for the boundary cases the (as, bs, last) triple of
every round, and that every ROI stays below the merge count at which host (500 rounds) and device (as many as it has rows) part."""
import numpy as np
import pytest

import line_setup_cases as lsc

CASES = lsc.all_cases()


@pytest.fixture(scope="module")
def statements():
    return {c["name"]: lsc.statement(c) for c in CASES}


def test_case_names_are_unique_and_inputs_fit():
    assert len({c["name"] for c in CASES}) == len(CASES)
    for c in CASES:
        assert len(c["lines"]) <= lsc.LS_CAP and len(c["rois"]) == len(c["yt"]) > 0 and np.isfinite(c["lines"]).all(), c["name"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_case_keeps_its_promise(case, statements):
    st = statements[case["name"]]
    P = case["promise"]
    assert [n for n, _, _ in st] == list(P["n_in"])
    for n_in, rows, rounds in st:
        assert len(rounds) < lsc.MAX_MERGES
    if not case["clear"]:
        return      # (on the thresholds the statement's decisions are not the library's)
    assert [len(rounds) for _, _, rounds in st] == list(P["merges"])
    if case["rounds"] is not None:
        assert [rounds for _, _, rounds in st] == case["rounds"]
    if "m" in P:
        assert [len(rows) for _, rows, _ in st] == P["m"]
    for k in P.get("skipped", []):
        assert 0 in tuple(case["yt"][k]) and len(st[k][1]) == 0


def test_the_cases_cover_what_they_are_for():
    by = {c["name"]: c for c in CASES}
    counts = by["counts"]
    assert counts["promise"]["n_in"][:13] == [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512]
    # every class in one call -> both lists non-empty; more listed jobs of one class than the grid of 1 024
    assert {lsc.size_class(n) for n in counts["promise"]["n_in"]} == {"small", "mid", "big"}
    many = by["many-jobs"]["promise"]["n_in"]
    assert sum(lsc.size_class(n) == "mid" for n in many) > 1024 and {lsc.size_class(n) for n in many} == {"small", "mid", "big"}
    assert [lsc.size_class(n) for n in by["chains"]["promise"]["n_in"]] == ["small", "mid", "big"]
    assert [lsc.size_class(n) for n in by["interleaved"]["promise"]["n_in"]] == ["small", "mid", "big"]
    # the word-boundary positions, on the register instance and on the 256-row one
    for N, cls in ((100, "small"), (200, "mid")):
        trip = {name[len("boundary-%d-" % N):]: c["rounds"][0] for name, c in by.items() if name.startswith("boundary-%d-" % N)}
        assert lsc.size_class(N) == cls and len(trip) == 10
        a, b, last = trip["as<64<=bs"][0]
        assert a < 64 <= b < last
        a, b, last = trip["both>=64"][0]
        assert 64 <= a < b < last
        a, b, last = trip["bs==last"][0]
        assert b == last
        assert trip["bs==63"][0][1] == 63 and trip["bs==62"][0][1] == 62 and trip["bs==63"][0][2] >= 64
        assert trip["moved,partner-behind-62"][1][:2] == (62, 63) and trip["moved,partner-behind-63"][1][:2] == (63, 80)
    assert by["boundary-65-total-onto-word"]["rounds"][0][0][2] == 64 and by["boundary-193-total-onto-word"]["rounds"][0][0][2] == 192
    a, b, last = by["boundary-512-last-word"]["rounds"][0][0]
    assert 448 <= a < b < last == 511
    # a row in front of `as` that becomes a partner of the merged row
    for N in (100, 200):
        (a1, b1, _), (a2, b2, _) = by["late-partner-%d" % N]["rounds"][0]
        assert a2 < a1 == b2
    # outside segments between the inside ones: in every 64-lane chunk of the input a row's place differs from its input position
    c = by["interleaved"]
    mask = lsc.inside(c["lines"], c["rois"][2])
    place = np.cumsum(mask) - 1
    for base in range(0, 512, 64):
        sel = np.arange(base, base + 64)[mask[base:base + 64]]
        assert len(sel) and (place[sel] != sel).all() and not mask[base:base + 64].all()
    # the threshold cases reach every instance
    assert {lsc.size_class(c["promise"]["n_in"][0]) for c in CASES if not c["clear"]} == {"small", "mid", "big"}
    assert any(c["len_thre"] == 0 for c in CASES)


def test_statement_on_a_hand_example():
    """Three collinear pieces and one far away: two merges, in the reference's order, the last row moving into the freed place."""
    L = [[0, 0, 40, 0], [200, 50, 240, 50], [45, 0, 85, 0], [90, 0, 130, 0]]
    rows, rounds = lsc.merge_break_lines(L)
    assert rounds == [(0, 2, 3), (0, 2, 2)]
    assert rows.tolist() == [[0, 0, 130, 0], [200, 50, 240, 50]]
    rows, _ = lsc.merge_break_lines([[0, 0, 10, 0], [100, 100, 140, 100]])
    assert rows.tolist() == [[100, 100, 140, 100]]      # the length threshold
    rows, _ = lsc.merge_break_lines([[0, 0, 10, 0], [100, 100, 140, 100]], len_thre=0)
    assert len(rows) == 2
