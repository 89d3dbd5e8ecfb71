"""The vanishing-point support on the device (cs_check_vp_support: vp_support_multi called directly -- the staged wavefront form <2, true> on pairs of
points, the unstaged forms <2, false> and <1, false>) against the reference's loop on the host (cs_atan2 for every segment, the unwrap, strict
first-occurrence extremes): the two bounding segment angles of every point, bit for bit, on the cases of vp_support_cases.py -- table sizes around
the 64-segment chunk, the first inlier in the second and third chunk, and the adversarial families listed there.  The points that keep clear of
every threshold by 1e-6 rad are also held to the float64 numpy statement of the reference there."""
import numpy as np
import pytest

import vp_support_cases as vsc
from cube_slam_wu_amd import capi

pytestmark = pytest.mark.gpu

CASES = vsc.all_cases()
FORMS = {0: "staged_pairs", 1: "unstaged_pairs", 2: "unstaged_single"}
_STATEMENTS = {}


def _statement(case, swapped):
    key = (case["name"], swapped)
    if key not in _STATEMENTS:
        _STATEMENTS[key] = vsc.statement(case, swapped)
    return _STATEMENTS[key]


@pytest.mark.parametrize("form", sorted(FORMS), ids=lambda f: FORMS[f])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_device_bounds_equal_host_bounds(case, form):
    n_clear = 0
    for swapped in (False, True):
        dev, host = capi.check_vp_support(case["mx"], case["my"], case["la"], case["vpx"], case["vpy"], case["thre"], swapped=swapped, form=form)
        bad = np.nonzero((dev.view(np.uint64) != host.view(np.uint64)).any(axis=1))[0]
        assert len(bad) == 0, (swapped, bad[:8], dev[bad[:4]], host[bad[:4]])
        want, clear = _statement(case, swapped)
        assert np.array_equal(dev[clear], want[clear], equal_nan=True), swapped
        assert np.array_equal(np.isnan(host[:, 0]), np.isnan(host[:, 1]))
        n_clear += int(clear.sum())
    if case["name"].startswith(("size_", "first_inlier", "no_inlier", "one_inlier", "collinear")):
        assert n_clear > 0      # (the statement has points to speak about in the families that are not built on a threshold)


def test_arguments_are_checked():
    c = CASES[3]
    with pytest.raises(RuntimeError, match="form must be"):
        capi.check_vp_support(c["mx"], c["my"], c["la"], c["vpx"], c["vpy"], c["thre"], form=3)
    dev, host = capi.check_vp_support(c["mx"], c["my"], c["la"], [], [], c["thre"])
    assert dev.shape == host.shape == (0, 2)
