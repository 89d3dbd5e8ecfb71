"""What the five batched entries share on the host (cube_slam_wu_amd/csrc/cs_batch_handle.h: Layout / Part, the chunk table, BatchCall,
batch_one_shot, Refuse and the argument predicates) WITHOUT a GPU and without the library: tools/hostonly/batch_handle_check.cpp is built with
the host compiler against the counting stand-in for the HIP runtime (tools/hostonly/hip_standin, first on the include path) and run as a
program of its own.  It holds that
  * the typed parts of the five entries' buffers lie exactly where the byte sums written out by hand before them put them (n = 0, 1, odd),
    behind 256-byte aligned offsets, without overlap, empty parts included;
  * the chunk table covers every item once and in order, in chunks of 1 .. 64 items of ONE owner, for owner sizes on both sides of 64 and 128
    and for empty owners first, last and in a row; count_status counts per owner;
  * `ran`, kernel_ms and host_ms are what batch_last_timing documents after an empty call, a refusal before the point of no return, a failure
    behind it and a finished call, for an entry that clears `ran` behind its checks and for one that clears it before them;
  * a one-shot entry frees as much as it made whatever its function returns.
Once plain, once under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "hostonly", "batch_handle_check.cpp")
BASE = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wno-unused-function", "-ffp-contract=off", "-I", os.path.join(ROOT, "tools", "hostonly", "hip_standin")]


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan_ubsan"])
def test_batch_handle_stand_alone(tmp_path, flags):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "batch_handle_check"
    subprocess.check_call(BASE + flags + [SRC, "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "batch_handle_check: ok"
