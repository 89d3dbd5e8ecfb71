"""The segment producers' batch driver (cube_slam_wu_amd/csrc/cs_image_batch.h: run_image_batch, ChunkGate, ChunkEvents, ImageBatchScratch)
WITHOUT a GPU and without the library: tools/hostonly/image_batch_check.cpp is built with the host compiler against the counting stand-in for
the HIP runtime (tools/hostonly/hip_standin, first on the include path) and run as a program of its own.  It defines the detector's hooks
itself (a pool of a few threads that take the tasks in ascending order) and drives the driver with a fake launch and a fake stage.  It holds that
  * the launches cover the images once, in order, in chunks of BATCH_CHUNK (1, 2, 4, 5, 8, 9 images); one image makes one launch and never
    touches the pool;
  * every image's stage runs once and sees its own slice; a failing stage's code comes back (the lowest image's) while every other stage
    still runs; a throwing stage gives CS_ERR_CAPACITY;
  * a failing `done` event gives CS_ERR_HIP, runs no stage of an image whose chunk was not declared ready before it, and lets every task return;
  * one scratch serves 9 images, then 1 larger image, then 3 images, its chunk events never shrinking;
  * nothing is live -- device memory, pinned memory, events -- once the scratch is gone.
Once under the address and undefined-behaviour sanitizers; once plain and under the thread sanitizer, which is skipped where the compiler has
no runtime for it to link or the runtime does not start."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tools", "hostonly", "image_batch_check.cpp")
BASE = ["g++", "-O1", "-g", "-std=c++17", "-Wall", "-pthread", "-I", os.path.join(ROOT, "tools", "hostonly", "hip_standin")]


def _check(out):
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "image_batch_check: ok"


def test_image_batch_driver_stand_alone(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "image_batch_check"
    subprocess.check_call(BASE + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", SRC, "-o", str(exe)])
    _check(subprocess.run([str(exe)], capture_output=True, text=True, timeout=120))


def test_image_batch_driver_under_the_thread_sanitizer(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    # the program itself builds (so a failure of the next build is the missing runtime, not the program) ...
    plain = tmp_path / "image_batch_check_plain"
    subprocess.check_call(BASE + [SRC, "-o", str(plain)])
    _check(subprocess.run([str(plain)], capture_output=True, text=True, timeout=120))
    exe = tmp_path / "image_batch_check_tsan"
    if subprocess.run(BASE + ["-fsanitize=thread", SRC, "-o", str(exe)], capture_output=True).returncode != 0:
        pytest.skip("g++ has no thread sanitizer runtime to link")
    # ... and the runtime starts here: on a kernel whose address-space layout it does not know it ends the program before main, with this
    # message and nothing from the program
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    if out.returncode != 0 and out.stdout == "" and "ThreadSanitizer: unexpected memory mapping" in out.stderr:
        pytest.skip("the thread sanitizer's runtime does not start on this machine")
    _check(out)
