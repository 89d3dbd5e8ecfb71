"""The types that own device resources (cube_slam_wu_amd/csrc/cs_hip_util.h: DevBuf, PinBuf, Stream, Event, Guard; ba_dbuf.h: DBuf,
StageArena) WITHOUT a GPU and without the library: tools/hostonly/owners_check.cpp is built with the host compiler against a counting
stand-in for the HIP runtime (tools/hostonly/hip_standin, first on the include path), under the address and undefined-behaviour sanitizers,
and run.  In the stand-in a free or destroy of something that is not live aborts.  The program holds that
  * nothing is live -- device memory, pinned memory, streams, events -- after each scenario: never used; grown three times; release()
    followed by the scope's end; an array of events partly created; a creation guard that fires; one that is disarmed;
  * the capacities follow the three growth rules (restated in the program) and DBuf::append_ptr keeps the old contents across a regrow;
  * none of the types can be copied (static_assert).
That the handles are made of these types and run is the GPU suite's business (test_handle_lifecycle_gpu.py)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_owner_types_give_everything_back_stand_alone(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "owners_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "tools", "hostonly", "hip_standin"),
                           os.path.join(ROOT, "tools", "hostonly", "owners_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "owners_check: ok"
