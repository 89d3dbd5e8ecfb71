"""Time of the batched Sim(3) alignment of keyframe pairs (cs_sim3_pairs_optimize) at the default parameters.

    python tools/sim3_pairs_quick.py [--pairs 256] [--matches 100] [--repeat 7] [--out profiles/sim3_pairs_quick.txt]

Prints, and writes to --out, the median kernel time (hipEvents on the handle's stream) and the median time of the whole call (host
clock: checking, packing, the two copies and the kernel) over --repeat calls after one warm-up call, with the iterations the pairs ran."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cube_slam_wu_amd import capi, synth_sim3_pairs  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--matches", type=int, default=100)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_pairs_quick.txt"))
    a = ap.parse_args()
    if capi.lib().cs_device_count() < 1:
        raise SystemExit("sim3_pairs_quick needs a HIP device")
    b = synth_sim3_pairs.synth_sim3_pairs(a.pairs, a.matches, 0.1, 1)
    p = capi.sim3_pair_default_params()
    h = capi.Sim3Pairs()
    out = h.optimize(b, p)                                 # warm-up: code object, buffers of this size
    kern, host, wall = [], [], []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        out = h.optimize(b, p)
        wall.append((time.perf_counter() - t0) * 1e3)
        t = h.timing()
        kern.append(t["kernel_ms"]); host.append(t["host_ms"])
    h.close()
    its = out["iterations"]
    lines = ["sim3_pairs_quick: %d pairs x %d matches, default parameters (5 iterations, then 10 or 5; th2 10), median of %d calls" % (a.pairs, a.matches, a.repeat),
             "kernel %.3f ms (%.2f us per pair)   host call %.3f ms   python call %.3f ms" % (np.median(kern), np.median(kern) * 1e3 / a.pairs, np.median(host), np.median(wall)),
             "iterations per pair: first round mean %.2f, second round mean %.2f; inliers mean %.1f of %d; pairs given up %d"
             % (its[:, 0].mean(), its[:, 1].mean(), out["n_inliers"].mean(), a.matches, int((out["n_inliers"] == 0).sum()))]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
