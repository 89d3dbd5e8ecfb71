"""The vanishing-point support procedure (cube_slam_wu_amd/csrc/cs_vp_support.h: the three-way cross/dot classification and the order of the inliers
from cross products) WITHOUT a GPU: tools/hostonly/vp_support_check.cpp is built against the header with the host compiler, under the address and
undefined-behaviour sanitizers, and run.  It holds the procedure's (arg-max, arg-min) indices to those of the reference's loop with cs_atan2 on 2
million seeded random tables and on the adversarial families (far vanishing points, collinear and duplicated mid points, both edges of the
undecided band, vanishing points to the right of everything, on a mid point, non-finite, no inlier / one inlier), and caps the share of
segments that the classification leaves undecided on the random tables at 1e-3.  The program walks the segments as the unstaged kernel form does,
with glibc's cosf / sinf for the direction: the staged form's control flow (the two bit masks, the loop that settles the undecided survivors,
the switched-off lanes of pass 2) is NOT covered here -- tests/test_vp_support_gpu.py holds it to the host's loop on the device.
And the GPU test's cases (vp_support_cases.py) are what their names say, by the float64 statement there."""
import os
import shutil
import subprocess

import numpy as np

import vp_support_cases as vsc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cross_product_order_equals_the_reference_loop_stand_alone(tmp_path):
    assert shutil.which("g++") is not None, "g++ is part of the project's tool chain"
    exe = tmp_path / "vp_support_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "hostonly", "vp_support_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    lines = out.stdout.strip().splitlines()
    assert lines[-1] == "vp_support_check: ok"
    assert lines[0].split()[:3] == ["random", "tables", "2000000"]


def _first_inliers(case):
    mx, my, la = case["mx"], case["my"], case["la"]
    first, count = [], []
    for vx, vy in zip(case["vpx"], case["vpy"]):
        d = np.abs(la - vsc.direction(mx, my, vx, vy))
        inl = np.nonzero(np.minimum(d, np.pi - d) < case["thre"])[0]
        first.append(inl[0] if len(inl) else -1)
        count.append(len(inl))
    return np.array(first), np.array(count)


def test_gpu_cases_are_what_they_say():
    cases = {c["name"]: c for c in vsc.all_cases()}
    assert [len(cases["size_%d" % m]["mx"]) for m in vsc.SIZES] == list(vsc.SIZES)
    assert all(len(c["vpx"]) <= vsc.N_POINTS for c in cases.values())
    for at in (64, 100, 128, 129):
        first, _ = _first_inliers(cases["first_inlier_at_%d" % at])
        assert np.all((first == -1) | (first >= at)) and np.sum(first >= at) > 100
        assert at < 128 or np.sum(first >= 128) > 100
    assert np.all(_first_inliers(cases["no_inlier"])[1] == 0)
    first, count = _first_inliers(cases["one_inlier"])
    assert np.all(count == 1) and np.all(first == 41)
    # the statement finds points that keep clear of every threshold in the families that are not built on one, and none of the far points
    for name in ("size_63", "size_130", "collinear_one_side", "first_inlier_at_128"):
        assert vsc.statement(cases[name])[1].sum() > 0, name
    out, clear = vsc.statement(cases["duplicates"])
    assert not np.all(np.isnan(out))
