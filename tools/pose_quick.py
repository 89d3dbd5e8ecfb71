"""Rate of the batched motion-only pose optimisation (cs_pose_batch_optimize) beside the only route the library offered before it:
one BaProblem per frame with every point fixed, creation and structure phase inside the clock (a tracking frame pays them).

    python tools/pose_quick.py [--sizes 1,64,1024,8192] [--obs 300] [--ba-frames 64]

Prints one line per batch size: frames/s of the whole call (host clock), kernel ms (hipEvents), bytes the kernel must move per frame
(its records once, its outputs once) over the kernel time; then the per-frame BaProblem route's frames/s on mono frames."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cube_slam_wu_amd import capi, synth_pose  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,64,1024,8192")
    ap.add_argument("--obs", type=int, default=300)
    ap.add_argument("--ba-frames", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=5)
    a = ap.parse_args()
    if capi.lib().cs_device_count() < 1:
        raise SystemExit("pose_quick needs a HIP device")
    p = capi.pose_default_params()
    sizes = [int(s) for s in a.sizes.split(",")]
    big = synth_pose.synth_pose_batch(max(sizes), a.obs, 0.5, 0.1, 1)
    h = capi.PoseBatch()
    for n in sizes:
        b = synth_pose.take_frames(big, range(n))
        h.optimize(b, p)                                   # warm-up: code object, buffers of this size
        wall, kern = [], []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            h.optimize(b, p)
            wall.append(time.perf_counter() - t0)
            kern.append(h.timing()["kernel_ms"])
        w, k = float(np.median(wall)), float(np.median(kern))
        bytes_frame = a.obs * (128 + 1) + 7 * 8 * 2 + 5 * 8 + 4 + p.n_rounds * 12
        print("pose batch %5d frames x %d obs: %10.0f frames/s (call %.3f ms), kernel %.3f ms = %.2f us/frame, %d B/frame -> %.2f GB/s over the kernel"
              % (n, a.obs, n / w, w * 1e3, k, k * 1e3 / n, bytes_frame, n * bytes_frame / (k * 1e-3) / 1e9))
    h.close()
    # the parent route: a BaProblem per frame, mono observations (the device projection edge has no stereo form), one round's worth of LM
    mono = synth_pose.synth_pose_batch(a.ba_frames, a.obs, 0.0, 0.1, 2)
    ptr = mono["obs_ptr"]

    def ba_frame(f):
        s = slice(ptr[f], ptr[f + 1])
        n = ptr[f + 1] - ptr[f]
        G = capi.BaProblem(mono["Tcw"][f][None], [0], points=mono["Xw"][s], pt_fixed=np.ones(n))
        G.set_edges_proj(np.arange(n), np.zeros(n), mono["meas"][s][:, :2], mono["info"][s][:, [0, 1, 3, 4]], np.tile(mono["intr"][f][:4], (n, 1)), np.full(n, p.huber_mono))
        G.optimize(10)
        G.state()
        G.close()
    ba_frame(0)
    t0 = time.perf_counter()
    for f in range(a.ba_frames):
        ba_frame(f)
    dt = time.perf_counter() - t0
    print("BaProblem per frame (ONE round of 10 iterations, no classification; create + structure inside the clock): %.1f frames/s (%.2f ms per frame) over %d frames"
          % (a.ba_frames / dt, dt * 1e3 / a.ba_frames, a.ba_frames))


if __name__ == "__main__":
    main()
