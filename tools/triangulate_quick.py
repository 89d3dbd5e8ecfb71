"""Time of the batched two-view triangulation of new map points (cs_triangulate_run) at the default parameters, beside the host build of
the same header (tools/hostonly/triangulate_host_check.cpp, g++ -O2, one core: cs::triangulate_pair_serial) over the same batches.

    python tools/triangulate_quick.py [--sizes 20x300,256x300] [--repeat 21] [--out profiles/triangulate_quick.txt]

Two sizes by default: 20 pairs x 300 matches, one keyframe's work in LocalMapping::CreateNewMapPoints, and 256 pairs x 300.  Per size it
prints, and writes to --out, the median and the range (min .. max) over --repeat calls, after two warm-up calls, of the kernel time
(hipEvents on the handle's stream) and of the whole call (host clock: checking, packing, the two copies and the kernel), the bytes the
kernel moves per match, and the serial worker's time per pass; the two must hand out the same statuses and routes."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cube_slam_wu_amd import capi, synth_triangulate  # noqa: E402

BYTES_PER_MATCH = 96 + 66      # a packed match in; X, normal, two distances, status and route out


def host_pass(exe, batch, p, repeat):
    """-> (the host check's `time` line, its statuses and routes)."""
    with tempfile.TemporaryDirectory() as d:
        dump = os.path.join(d, "batch.txt")
        synth_triangulate.write_dump(dump, batch, [p.min_baseline_ratio, p.max_cos_parallax, p.chi2_mono, p.chi2_stereo, p.ratio_factor, p.scale_range])
        timed = subprocess.check_output([exe, "time", str(repeat), dump], text=True).splitlines()[0]
        rows = [[int(x) for x in line.split()[2:4]] for line in subprocess.check_output([exe, "run", dump], text=True).splitlines() if line.startswith("m ")]
        return timed, np.array(rows).reshape(-1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20x300,256x300")
    ap.add_argument("--repeat", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulate_quick.txt"))
    a = ap.parse_args()
    if capi.lib().cs_device_count() < 1:
        raise SystemExit("triangulate_quick needs a HIP device")
    tmp = tempfile.TemporaryDirectory()
    exe = os.path.join(tmp.name, "triangulate_host_check")
    try:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "hostonly", "triangulate_host_check.cpp"), "-o", exe])
    except (OSError, subprocess.CalledProcessError):
        exe = None
    p = capi.triangulate_default_params()
    h = capi.Triangulate()
    lines = []
    for size in a.sizes.split(","):
        pairs, matches = (int(v) for v in size.split("x"))
        b = synth_triangulate.synth_triangulate(pairs, matches, 1)
        for _ in range(2):                                 # warm-up: code object, buffers of this size
            out = h.run(b, p)
        kern, host, wall = [], [], []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            out = h.run(b, p)
            wall.append((time.perf_counter() - t0) * 1e3)
            t = h.timing()
            kern.append(t["kernel_ms"]); host.append(t["host_ms"])
        n = pairs * matches
        k = float(np.median(kern))
        lines.append("triangulate_quick: %d pairs x %d matches, default parameters, median (min .. max) of %d calls after 2 warm-up calls" % (pairs, matches, a.repeat))
        lines.append("  kernel %.4f ms (%.4f .. %.4f): %.2f ns per match, %.1f GB/s of its %d bytes per match   host call %.3f ms (%.3f .. %.3f)   python call %.3f ms"
                     % (k, min(kern), max(kern), k * 1e6 / n, n * BYTES_PER_MATCH / (k * 1e6), BYTES_PER_MATCH, np.median(host), min(host), max(host), np.median(wall)))
        lines.append("  accepted %d of %d; routes none / triangulated / stereo1 / stereo2 %s" % (int(out["n_accepted"].sum()), n, np.bincount(out["route"], minlength=4).tolist()))
        if exe is None:
            lines.append("  host build of cs_triangulate.h: no figure recorded (no g++ here)")
        else:
            timed, rows = host_pass(exe, b, p, a.repeat)
            same = np.array_equal(rows, np.stack([out["status"], out["route"]], 1))
            lines.append("  cs_triangulate.h with g++ -O2 -- " + timed + ("; same statuses and routes as the device" if same else "; RESULTS DIFFER FROM THE DEVICE'S"))
    h.close()
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
