"""The detector's worker pool (cube_slam_wu_amd/csrc/cs_worker_pool.h) WITHOUT a GPU: tools/hostonly/worker_pool_check.cpp is built against the
header with the host compiler under the thread sanitizer and run.  It holds
  * run(n, fn) to calling fn exactly once for every i in [0, n), for n in {0, 1, 2, 7, 1000} with 0, 1 and 5 workers (the per-item counters are
    plain ints: an item handed out twice is a data race the sanitizer reports as well);
  * a thousand runs back to back to losing and doubling no item (the generation / pending handshake between run() and the workers);
  * max_threads = 1 to running every item on the caller, and max_threads = 2 to at most two distinct threads inside fn in any run.  The pool
    reserves the caller's place among the max_threads before it wakes the workers, so neither depends on which thread wakes first."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_worker_pool_hands_every_item_out_once_under_the_thread_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "worker_pool_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-fsanitize=thread", os.path.join(ROOT, "tools", "hostonly", "worker_pool_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "worker_pool_check: ok"
