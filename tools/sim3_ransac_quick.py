"""Time of the batched Sim(3) RANSAC of keyframe pairs (cs_sim3_ransac_run) at the default parameters, beside the host build of the same
header (tools/hostonly/sim3_ransac_host_check.cpp, g++ -O2, one core) over the same batch.

    python tools/sim3_ransac_quick.py [--pairs 256] [--matches 100] [--mismatches 0.5] [--repeat 7] [--out profiles/sim3_ransac_quick.txt]

Prints, and writes to --out, the median kernel time (hipEvents on the handle's stream) and the median time of the whole call (host
clock: checking, packing, the two copies and the kernel) over --repeat calls after one warm-up call, the hypotheses the pairs ran, and
the serial worker's time per pass; the two must hand out the same found / hyp / n_inliers."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cube_slam_wu_amd import capi, synth_sim3_ransac  # noqa: E402


def host_pass(batch, p, repeat):
    """-> (the host check's `time` line, its per-pair rows) or (None, None) without g++."""
    with tempfile.TemporaryDirectory() as d:
        exe, dump = os.path.join(d, "sim3_ransac_host_check"), os.path.join(d, "batch.txt")
        try:
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "hostonly", "sim3_ransac_host_check.cpp"), "-o", exe])
        except (OSError, subprocess.CalledProcessError):
            return None, None
        synth_sim3_ransac.write_dump(dump, batch, p.probability, p.min_inliers, p.max_iterations)
        timed = subprocess.check_output([exe, "time", str(repeat), dump], text=True).splitlines()[0]
        rows = [[int(x) for x in line.split()[2:6]] for line in subprocess.check_output([exe, "run", dump], text=True).splitlines() if line.startswith("pair ")]
        return timed, np.array(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--matches", type=int, default=100)
    ap.add_argument("--mismatches", type=float, default=0.5)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_ransac_quick.txt"))
    a = ap.parse_args()
    if capi.lib().cs_device_count() < 1:
        raise SystemExit("sim3_ransac_quick needs a HIP device")
    b = synth_sim3_ransac.synth_sim3_ransac(a.pairs, a.matches, a.mismatches, 1, point_sigma=0.005)
    p = capi.sim3_ransac_default_params()
    h = capi.Sim3Ransac()
    out = h.run(b, p)                                      # warm-up: code object, buffers of this size
    kern, host, wall = [], [], []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        out = h.run(b, p)
        wall.append((time.perf_counter() - t0) * 1e3)
        t = h.timing()
        kern.append(t["kernel_ms"]); host.append(t["host_ms"])
    h.close()
    blocks = (np.where(out["found"] == 1, out["hyp"] + 1, out["iterations"]) + 63) // 64
    lines = ["sim3_ransac_quick: %d pairs x %d matches, %.0f %% mismatches, default parameters (0.99, 20, 300), median of %d calls" % (a.pairs, a.matches, 100 * a.mismatches, a.repeat),
             "kernel %.3f ms (%.2f us per pair)   host call %.3f ms   python call %.3f ms" % (np.median(kern), np.median(kern) * 1e3 / a.pairs, np.median(host), np.median(wall)),
             "found %d of %d; iterations mean %.1f; hypotheses evaluated mean %.0f (blocks of 64); inliers mean %.1f of %d"
             % (int(out["found"].sum()), a.pairs, out["iterations"].mean(), 64 * blocks.mean(), out["n_inliers"].mean(), a.matches)]
    timed, rows = host_pass(b, p, a.repeat)
    if timed is None:
        lines.append("host build of cs_sim3_ransac.h: no figure recorded (no g++ here)")
    else:
        same = np.array_equal(rows, np.stack([out["found"], out["hyp"], out["iterations"], out["n_inliers"]], 1))
        lines.append("cs_sim3_ransac.h with g++ -O2 -- " + timed + ("; same found / hyp / iterations / n_inliers as the device" if same else "; RESULTS DIFFER FROM THE DEVICE'S"))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
