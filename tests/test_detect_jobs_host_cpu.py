"""The detector host's job-table rules (cube_slam_wu_amd/csrc/detect_jobs_host.h) WITHOUT a GPU: tools/hostonly/detect_jobs_host_check.cpp is built
against the header with the host compiler, under the address and undefined-behaviour sanitizers, and run.  It holds each rule to the reference's
rule restated in the program, not to the header's own output:
  * the top-edge samples of a box to linespace<int>(left + 5, right - 5, step) with the reference's truncations, for widths 9 (skipped), 10 (one
    sample), 19, 20, 105, 200, 209, 1000 (step capped at 20), a box with fractional left and width, and one with more samples than linespace
    returns; the count-only call (what the batch layout reserves) equals the number written;
  * the yaw list of a camera yaw to the linespace<double> loop for (range, step) = (30, 6), (45, 0.5), (45, 3) at camera yaws 0, +-pi and 1e-3:
    the count fits the capacity, cos / sin are bit-equal to h_cos / h_sin of the entries, a capacity that is too small is reported and nothing is
    written past it;
  * the three slot / vanishing-point span rules on jobs with RP in {1, 3}, Y in {0, 1, 5, 181}, T in {0, 1, 4}: spans disjoint and in order, each
    with room for RP*Y*T*2 slots and RP*Y vanishing-point entries, decode_slot of a job's first and last real slot, the production rule's
    offsets multiples of 256 and 64;
  * the launch order of the line setup: a permutation with non-increasing work bucket;
  * the merged I/O block of a small call: offsets 256-aligned, disjoint, increasing, the input part ending where the job table ends, for 1 and
    256 jobs with and without boxes.
That the three paths then compute the same bytes is tests/test_detect_gpu.py's business."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INC = "/opt/rocm/include"


def test_job_table_rules_stand_alone(tmp_path):
    if shutil.which("g++") is None or not os.path.exists(os.path.join(HIP_INC, "hip", "hip_runtime.h")):
        pytest.skip("needs g++ and the HIP headers")
    exe = tmp_path / "detect_jobs_host_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INC, os.path.join(ROOT, "tools", "hostonly", "detect_jobs_host_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "detect_jobs_host_check: ok"
