"""The C-ABI library loads without a GPU and exports every function include/cubeslam_hip.h declares."""
import os
import re
import subprocess

from cube_slam_wu_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "cubeslam_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", src)))


def test_header_functions_are_exported():
    names = _declared()
    assert len(names) >= 30
    out = subprocess.check_output(["nm", "-D", "--defined-only", capi.LIB_PATH], text=True)
    exported = set(line.split()[-1] for line in out.splitlines() if " T " in line)
    missing = [n for n in names if n not in exported]
    assert not missing, missing
    assert sorted(capi.DECLARED_SYMBOLS) == names


def test_library_loads_and_refuses_to_run_without_a_device():
    L = capi.lib()
    if L.cs_device_count() > 0:
        return
    import ctypes as C
    h = C.c_void_p()
    assert L.cs_detector_create(None, 0, C.byref(h)) == -3  # CS_ERR_NO_DEVICE: no CPU fallback
    assert L.cs_ba_create(0, C.byref(h)) == -3
    assert "no CPU fallback" in capi.last_error()


def test_no_product_file_references_the_oracle():
    pkg = os.path.join(ROOT, "cube_slam_wu_amd")
    for d, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".cpp", ".hip", ".h")):
                txt = open(os.path.join(d, f), errors="ignore").read()
                assert "oracle/" not in txt and "import oracle" not in txt and "from oracle" not in txt, os.path.join(d, f)


def test_bench_traffic_passes_fall_back_without_a_device(monkeypatch):
    """bench.py collects roofline.traffic with two rocprofv3 child passes; when they cannot run (here: no HIP device, so the child
    exits at once; on a box without rocprofv3: not found) the function must return None -- the caller then reports the tracked
    figure -- and must not raise."""
    import importlib.util
    import types
    monkeypatch.setenv("HIP_VISIBLE_DEVICES", "-1")      # no HIP device for the child passes, on a GPU machine too
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    args = types.SimpleNamespace(frames=4)
    assert bench.measure_traffic_live(args, 2) is None


def test_sparse_plan_symbolic_phase_on_random_block_graphs():
    """Host side of the general sparse reduced solve (csrc/ba_sparse.h: minimum-degree block ordering, symbolic factorisation, update lists,
    level order -- the place of g2o's LinearSolverEigen, solvers/linear_solver_eigen.h:94-232): on 40 random meshes / chains with long links the
    plan's pattern is exactly the fill of eliminating the vertices in its order, and its processing order respects every update dependency."""
    import subprocess
    exe = os.path.join(ROOT, "build_tmp", "sparse_plan_check")
    if not os.path.exists(exe):
        subprocess.check_call(["hipcc", "-O2", "-std=c++17", os.path.join(ROOT, "tools", "microbench", "sparse_plan_check.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "40 random block graphs" in out.stdout, out.stdout + out.stderr


def test_fast_atan2_error_bound_behind_the_lsd_region_growing():
    """Field::grow (csrc/lsd_host.cpp; the reference: line_lbd/libs/lsd.cpp:644-692) decides a neighbour's alignment from the cos / sin sums
    themselves unless the angle is within 0.2 degrees of the tolerance -- sound because OpenCV's fastAtan2 (csrc/cs_fast_atan.h) is never more
    than 0.0096 degrees from the true angle.  The tool walks every 61st float quotient through all sign / branch cases here (stride 1, every
    quotient, gives 0.009559 degrees in 45 s); the segments themselves are held to the restatement bit for bit in tests/test_lines_gpu.py."""
    import subprocess
    exe = os.path.join(ROOT, "build_tmp", "lsd_atan_bound")
    src = os.path.join(ROOT, "tools", "microbench", "lsd_atan_bound.cpp")
    if not os.path.exists(exe) or os.path.getmtime(exe) < os.path.getmtime(src):
        os.makedirs(os.path.dirname(exe), exist_ok=True)
        subprocess.check_call(["g++", "-O2", "-std=c++17", src, "-o", exe, "-pthread"])
    out = subprocess.run([exe, "61"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "at most 0.0095" in out.stdout, out.stdout + out.stderr
