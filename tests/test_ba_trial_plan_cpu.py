"""The switches of cs_ba_optimize's trial flow (cube_slam_wu_amd/csrc/ba_trial_plan.h) WITHOUT a GPU and without the library:
tools/hostonly/ba_trial_plan_check.cpp is built against the header alone with the host compiler, under the address and undefined-behaviour
sanitizers, and run.  Over every combination of the facts the plan reads (17 booleans, shard_n in {1, 2, 3}, band_ld in {0, 33}, n_red in
{0, 132}, the solve deferred or not) it holds each switch to
  * the expression cs_ba_optimize / solve_device used before the header existed, restated in the program;
  * the implications the header's comments claim: speculation => stream flow, one rank, no external edges, no stage split, NaN scans off,
    direct scalars; direct scalars => no RCCL; fused linearisation => stream flow, one rank, fused schedule, no external edges;
    pro_in_reduce => deferred, lean head, no stage split; status_in_scalars => deferred, block cyclic reduction; sum_ranks <=> collectives
    active and not separator mode; stream flow => no callback;
  * and pins the one place where the driver's plan and the queued solve's head disagree to its exact set of cases.
That ba_lm.cpp reads the facts off the handle and follows the plan is the GPU suite's business."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_trial_plan_switches_hold_their_definitions_stand_alone(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "ba_trial_plan_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "hostonly", "ba_trial_plan_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "ba_trial_plan_check: ok"
