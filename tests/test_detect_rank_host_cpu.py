"""The detector host's shared rules (cube_slam_wu_amd/csrc/detect_rank_host.h) WITHOUT a GPU: tools/hostonly/detect_rank_host_check.cpp is built
against the header with the host compiler, under the address and undefined-behaviour sanitizers, and run.  It holds
  * decode_slot to the slot numbering slot = slot_off + ((rp*Y + yaw)*T + top)*2 + (config-1) for every (rp, yaw, top, config) of a job with
    RP = 3, Y = 5, T = 4 and a non-zero slot_off;
  * exact_rank_box -- the one copy of the exact final ranking all four sweep paths call -- to its properties (min(KMAX, proposals) winners, comb
    non-decreasing, no flagged candidate, every winner in its height sample's keep list, the last kept slot of the last height sample or -1) for
    V = 0, V <= 4, V = 30 with all-equal distance keys, a height sample with every candidate flagged, KMAX above the number of proposals and three
    height samples, with and without precomputed keep / score lists;
  * the camera cache (detect_cam_host.h): rot_to_euler(euler_to_rot(r, p, y)) = (r, p, y) over a grid that takes the positive-trace branch and each
    of the three largest-diagonal branches of the quaternion step; make_cam's KinvR against K R^-1 in long double and its ground-plane row; the
    roll/pitch sample poses, roll-major, each storing its sample angles (25 for a camera whose lists close at +6 degrees, 20 for a forward-looking
    one whose roll list rounds past it -- the count linespace's loop gives, restated);
  * host_corners16 to build_corners on the vanishing points restated in the program, bit for bit, with at least one accepted proposal;
  * the record writers (write_exact_winners with corners from a callback and from corners_at, write_device_records) to writing the records and count of rec(f, box, r) / count(f, box)
    of a 2-frame, 3-box, KMAX = 2 output and no element beside them; rank_weights / rank_params to the detector's parameters.
That the four callers then write the same bytes is tests/test_detect_gpu.py's business."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INC = "/opt/rocm/include"


def test_slot_decode_and_exact_ranking_properties_stand_alone(tmp_path):
    if shutil.which("g++") is None or not os.path.exists(os.path.join(HIP_INC, "hip", "hip_runtime.h")):
        pytest.skip("needs g++ and the HIP headers")
    exe = tmp_path / "detect_rank_host_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INC, os.path.join(ROOT, "tools", "hostonly", "detect_rank_host_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "detect_rank_host_check: ok"
