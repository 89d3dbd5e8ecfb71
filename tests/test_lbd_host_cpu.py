"""The line band descriptor's arithmetic (cube_slam_wu_amd/csrc/cs_lbd.h -- the functions the device kernel compiles) built WITHOUT a GPU into
tools/hostonly/lbd_host_check.cpp and held to the numpy restatement tests/lbd_ref.py bit for bit; with a GPU the same inputs go through the C ABI
in tests/test_lbd_gpu.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import lbd_cases
import lbd_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INC = "/opt/rocm/include"
TUM = ("tum0", "tum20", "tum45")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    if shutil.which("g++") is None or not os.path.exists(os.path.join(HIP_INC, "hip", "hip_runtime.h")):
        pytest.skip("needs g++ and the HIP headers")
    exe = tmp_path_factory.mktemp("lbd") / "lbd_host_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INC, os.path.join(ROOT, "tools", "hostonly", "lbd_host_check.cpp"),
                           "-o", str(exe)])
    return str(exe)


def _run(exe, tmp_path, gray, kl):
    dx, dy = lbd_ref.sobel_maps(gray)
    H, W = gray.shape
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.array([W, H, len(kl)], np.int32).tobytes())
        f.write(np.ascontiguousarray(dx, np.int16).tobytes())
        f.write(np.ascontiguousarray(dy, np.int16).tobytes())
        f.write(np.ascontiguousarray(kl).tobytes())
    out = subprocess.run([exe, str(fin), str(fout)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "%d lines described" % len(kl) in out.stdout, out.stdout + out.stderr
    raw = open(fout, "rb").read()
    n = len(kl)
    d72 = np.frombuffer(raw[:n * 72 * 4], np.float32).reshape(n, 72)
    d32 = np.frombuffer(raw[n * 72 * 4:], np.uint8).reshape(n, 32)
    return d32, d72


@pytest.mark.parametrize("name", ["explicit", "small", "flat", "ramp"] + list(TUM))
def test_host_build_of_the_descriptor_equals_the_restatement_bit_for_bit(check_exe, tmp_path, name):
    """desc32 equal, desc72 equal with NaN = NaN, on the device test's shapes (border-hugging lines, a line partly outside, every length class,
    the axis directions, k + 0.5 mid-points; an image smaller than the 63-row support; a flat image: all NaN / all zero; a ramp) and on the
    oracle's segments of TUM frames 0, 20 and 45 (num_pixels = max(|dx|, |dy|) + 1 of the rounded end points, direction = atan2f)."""
    gray, kl, ref32, ref72 = lbd_cases.case(name)
    got32, got72 = _run(check_exe, tmp_path, gray, kl)
    assert np.array_equal(got32, ref32)
    assert lbd_ref.same_floats(got72, ref72)
    if name == "flat":
        assert np.isnan(ref72).all() and not ref32.any()
    if name == "ramp":
        assert np.isfinite(ref72).any()


def test_the_restatement_stays_close_to_its_double_twin_on_the_reference_frames():
    """A guard against a restatement written twice wrong: on TUM frames 0, 20 and 45 the float32 reference contains no NaN and differs from the
    same formulas carried in float64 in at most 0.5 % of the descriptor bits.  Measured: 82 segments, 4 of 20 992 bits differ (0.02 %), worst
    difference of a descriptor element 3.5e-3 -- the bound is 26 times that, so the restatement alone stays well inside it."""
    bits = diff = 0
    worst = 0.0
    for name in TUM:
        gray, kl, ref32, ref72 = lbd_cases.case(name)
        assert len(kl) > 0 and not np.isnan(ref72).any()
        dx, dy = lbd_ref.sobel_maps(gray)
        d32, d72 = lbd_ref.describe(dx, dy, kl, np.float64)
        bits += ref32.size * 8
        diff += int(np.unpackbits(ref32 ^ d32).sum())
        worst = max(worst, float(np.abs(d72 - ref72.astype(np.float64)).max()))
    print("float32 vs float64 reference: %d of %d bits differ, worst element difference %.3g" % (diff, bits, worst))
    assert diff <= 0.005 * bits, (diff, bits, worst)

