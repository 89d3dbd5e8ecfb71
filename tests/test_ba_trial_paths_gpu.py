"""The one switch of cs_ba_optimize's trial flow that no other test flips: the stage split (cs_ba_set_stage_timing).

With the split on, every phase of a trial is bracketed by events on the stream, and two things the default flow does are off: the next
iteration's linearisation is not speculated behind the trial, and the banded solve's prologue kernel is not moved to the side stream inside the
reduce (csrc/ba_trial_plan.h: can_spec, pro_in_reduce).  Both claim "the same bits either way".  This module holds them to it.

Graphs (the smallest that reach each path, as in test_ba_after_optimize_gpu.py):
  fused     make_problem(40, 2500, 8, seed=3)     stream flow, fused linearisation, cuboid elimination
  rejected  the same, set_lm_params(1e-8, 10)     rejected trials: pop + re-linearisation (a trial count above 1)
  band132   make_problem(23, 920, 0, seed=23)     no cuboid, 132 unknowns: the smallest banded system
  dense     make_problem(12, 400, 2, seed=5)      dense solve: the synchronising flow
Per graph two fresh handles, one with stage_timing(True), optimize(4) each:
  * history() and state() are np.array_equal;
  * with the split on, timing()'s linearize / reduce / factor / backsub fields are > 0;
  * with the split off, the reduce / factor / backsub fields are 0 on the banded graphs (no phase mark was recorded);
  * band_ld and the Schur layout are the case's, so that no case passes beside its path.
"""
import numpy as np
import pytest

from cube_slam_wu_amd import capi, synth_ba

pytestmark = pytest.mark.gpu

CASES = {
    "fused": dict(graph=(40, 2500, 8, 3), fused=True, band=True),
    "rejected": dict(graph=(40, 2500, 8, 3), fused=True, band=True, lm=(1e-8, 10)),
    "band132": dict(graph=(23, 920, 0, 23), band=True, n_red=132),
    "dense": dict(graph=(12, 400, 2, 5), band=False),
}
SPLIT_FIELDS = ("linearize_ms", "reduce_ms", "factor_ms", "backsub_ms")

_graphs, _runs = {}, {}


def _graph(key):
    if key not in _graphs:
        nc, npt, no, seed = key
        _graphs[key] = synth_ba.make_problem(nc, npt, no, seed=seed)
    return _graphs[key]


def _optimize(pr, c, split):
    H = capi.ba_from_dict(pr)
    if "lm" in c:
        H.set_lm_params(*c["lm"])
    if split:
        H.stage_timing(True)
    r = {"schur_layout": H.schur_layout(), "solver_layout": H.solver_layout(), "reduced_size": H.reduced_size(), "band_order": H.band_order()}
    r["done"] = H.optimize(4)
    r["history"] = tuple(np.array(h) for h in H.history())
    r["state"] = H.state()
    r["timing"] = H.timing()
    H.close()
    return r


def _run(name):
    if name not in _runs:
        c = CASES[name]
        pr = _graph(c["graph"])
        _runs[name] = (_optimize(pr, c, False), _optimize(pr, c, True))
    return _runs[name]


case = pytest.mark.parametrize("name", list(CASES))


@case
def test_the_case_took_its_path(name):
    c = CASES[name]
    for r in _run(name):
        band_ld = r["solver_layout"][0]
        assert (band_ld > 0) if c["band"] else (band_ld == 0), r["solver_layout"]
        if "fused" in c:
            assert r["schur_layout"][0] == c["fused"], r["schur_layout"]
        if "n_red" in c:
            assert r["reduced_size"][0] == c["n_red"], r["reduced_size"]
        print(name, "Schur layout", r["schur_layout"], "band_ld", band_ld, "reduced", r["reduced_size"], "block cyclic reduction", r["band_order"])
        assert r["done"] >= 2
        if name == "rejected":
            assert r["history"][2].max() > 1, r["history"][2]


@case
def test_the_stage_split_changes_no_bit(name):
    off, on = _run(name)
    print(name, "trials", off["history"][2], on["history"][2], "chi2", off["history"][0], on["history"][0])
    assert off["done"] == on["done"]
    for k, (a, b) in enumerate(zip(off["history"], on["history"])):
        assert np.array_equal(a, b), ("history", k, a, b)
    for k, (a, b) in enumerate(zip(off["state"], on["state"])):
        assert np.array_equal(a, b), ("state", k, np.abs(a - b).max())
    assert off["timing"]["n_solves"] == on["timing"]["n_solves"] == int(off["history"][2].sum())


@case
def test_the_split_is_filled_only_when_asked_for(name):
    off, on = _run(name)
    print(name, "off", {k: off["timing"][k] for k in SPLIT_FIELDS}, "on", {k: on["timing"][k] for k in SPLIT_FIELDS})
    for k in SPLIT_FIELDS:
        assert on["timing"][k] > 0, (k, on["timing"])
    if CASES[name]["band"]:
        for k in ("reduce_ms", "factor_ms", "backsub_ms"):
            assert off["timing"][k] == 0, (k, off["timing"])
