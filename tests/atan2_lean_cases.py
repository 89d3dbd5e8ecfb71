"""Shared by tests/test_atan2_lean.py and tests/test_atan2_lean_gpu.py: the host shim around cs_atan2_lean / cs_atan2
(tests/atan2_lean_shim.cpp, built here with g++ -O2 -ffp-contract=off) and the scorer's own atan2 operands."""
import ctypes as C
import functools
import math
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "cube_slam_wu_amd", "csrc")

# test_special_values_follow_ieee's list (tests/test_atan2.py)
SPECIAL_VALUES = [0.0, -0.0, 1.0, -1.0, math.inf, -math.inf, math.nan, 1e-310, -1e-310, 1e308, -1e308, 5e-324, 3.0, 1e-200, 1e200]

# the corner ids of the six edges of score_kernel's angle term (detect_kernels.hip: ID1 / ID2), per configuration
EDGE_IDS = {1: [[0, 1, 7, 4], [3, 0, 4, 5], [3, 7, 1, 5]], 2: [[0, 1, 2, 3], [3, 0, 4, 5], [2, 4, 1, 5]]}


@functools.lru_cache(maxsize=None)
def shim():
    src = os.path.join(ROOT, "tests", "atan2_lean_shim.cpp")
    out = os.path.join(ROOT, "build_tmp", "libatan2_lean_shim.so")
    deps = [src] + [os.path.join(_CSRC, h) for h in ("cs_atan2_lean.h", "cs_atan2.h", "cs_atan2_tab.h")]
    if not os.path.exists(out) or os.path.getmtime(out) < max(os.path.getmtime(d) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        tmp = "%s.%d" % (out, os.getpid())
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function", "-shared", "-o", tmp, src])
        os.replace(tmp, out)
    L = C.CDLL(out)
    dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    L.lean_batch.restype = C.c_longlong
    L.lean_batch.argtypes = [dp, dp, C.c_longlong, dp, bp, dp, bp]
    L.lean_value.restype = C.c_int
    L.lean_value.argtypes = [C.c_double, C.c_double, dp, dp, dp]
    L.lean_compare.restype = C.c_longlong
    L.lean_compare.argtypes = [C.c_longlong, C.c_ulonglong, C.c_int, C.POINTER(C.c_longlong), C.POINTER(C.c_longlong)]
    return L


def lean_batch(y, x):
    """(cs_atan2 values, lean values (0 where declined), accepted flags, special flags, number of accepted pairs whose bits differ)."""
    y, x = np.ascontiguousarray(y, np.float64), np.ascontiguousarray(x, np.float64)
    n = len(y)
    out, ref = np.zeros(n), np.zeros(n)
    acc, spc = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    dp, bp = C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    bad = shim().lean_batch(y.ctypes.data_as(dp), x.ctypes.data_as(dp), n, out.ctypes.data_as(dp), acc.ctypes.data_as(bp), ref.ctypes.data_as(dp), spc.ctypes.data_as(bp))
    return ref, out, acc.astype(bool), spc.astype(bool), int(bad)


def edge_operands(corners, configs):
    """(dy, dx) of the six edges of every proposal, in score_kernel's order: corners [n, 16] = x0..x7, y0..y7, configs [n] in {1, 2}."""
    corners, configs = np.asarray(corners, np.float64), np.asarray(configs).astype(int)
    dy, dx = np.zeros((len(corners), 6)), np.zeros((len(corners), 6))
    for cfg, ids in EDGE_IDS.items():
        m = configs == cfg
        for k in range(3):
            for ee in range(2):
                pa, pb = ids[k][2 * ee], ids[k][2 * ee + 1]
                dy[m, 2 * k + ee] = corners[m, 8 + pb] - corners[m, 8 + pa]
                dx[m, 2 * k + ee] = corners[m, pb] - corners[m, pa]
    return dy.ravel(), dx.ravel()


HALF_DEGREE_SEEDS = ((9110, 2, 120), (4242, 2, 150))      # (seed, boxes, segments) of the two half-degree frames


@functools.lru_cache(maxsize=None)
def scorer_operands():
    """The atan2 operands score_kernel evaluates on two half-degree frames, from the oracle's candidate corners."""
    from cube_slam_wu_amd import synth
    from oracle import oracle_py
    ys, xs = [], []
    for seed, nb, nl in HALF_DEGREE_SEEDS:
        fr = synth.make_frame(seed, n_boxes=nb, n_lines=nl)
        cap = 20000
        _, dbg = oracle_py.detect_cuboid(fr, oracle_py.default_params(whether_sample_cam_roll_pitch=0, yaw_step_deg=0.5), atan2_mode=1, debug_cap=cap)
        for i in range(len(fr["boxes"])):
            for k in range(len(fr["maps"][i])):
                slot = 3 * i + k
                V = int(dbg["n_valid"][slot])
                assert V <= cap
                dy, dx = edge_operands(dbg["cand_corners"][slot][:V], dbg["cand_rows"][slot][:V, 0])
                ys.append(dy); xs.append(dx)
    y, x = np.concatenate(ys), np.concatenate(xs)
    y.setflags(write=False); x.setflags(write=False)
    return y, x
