"""The projection edge of the bundle adjustment (cube_slam_wu_amd/csrc/ba_proj_edge.h) WITHOUT a GPU and without the library:
tools/hostonly/ba_proj_edge_check.cpp is built with the host compiler against the header and the stand-in for the HIP runtime
(tools/hostonly/hip_standin, first on the include path), with -ffp-contract=off like the library and under the address and
undefined-behaviour sanitizers, and run.  Over 4200 random edges (points in front of, near and behind the camera; full information; every
robust kind and width, width 0 included; the classes' kernels switched off; level-1 edges, some at depth exactly 0) it holds
  * ProjLinT<2> and the 2-row products, byte for byte, to the expressions the four kernels spelled inline before the header existed,
    restated once in the program;
  * ProjLinT<3> and the 3-row products, byte for byte, to the proj_linearize_any / lin3_* they replace;
  * a mono edge through the 3-row form to the 2-row values (equal as doubles), and every product of a level-1 edge to zero;
  * the table view's accessors and proj_edge_chi to what the chi2 sites spelled.
That the kernels call these functions and agree with each other on the device is the GPU suite's business (test_ba_gpu.py,
test_ba_stereo_gpu.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_projection_edge_forms_hold_the_parent_expressions_stand_alone(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "ba_proj_edge_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "tools", "hostonly", "hip_standin"),
                           os.path.join(ROOT, "tools", "hostonly", "ba_proj_edge_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "ba_proj_edge_check: ok"
