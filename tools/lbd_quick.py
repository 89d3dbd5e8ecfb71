"""What describing costs on top of detecting, and what the two new kernels take (outside bench.py):
  python tools/lbd_quick.py [--images 64] [--reps 20] [--out profiles/lbd_quick.txt]
64 KITTI-sized (376 x 1241) synthetic images; cs_detect_lines_batch and cs_detect_descrip_lines_batch timed in the same run, alternating, after
warm-up (median of the repetitions; the difference is the cost of describing); the describe kernel's own time from its events; cs_lbd_match_batch
on 64 pairs of the descriptor sets just produced (image i against image i + 1)."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cube_slam_wu_amd import capi  # noqa: E402


def image(seed, h=376, w=1241):
    r = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.full((h, w), 100.0)
    for _ in range(40):
        a = r.uniform(0, np.pi)
        img += np.where((xx - r.uniform(0, w)) * np.cos(a) + (yy - r.uniform(0, h)) * np.sin(a) > 0, r.uniform(-60, 60), 0)
    return np.clip(img + r.normal(0, 3, img.shape), 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cap", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    grays = [image(100 + i) for i in range(a.images)]
    det = capi.Detector(capi.default_params())
    t_det, t_desc, k_desc, t_match, k_match = [], [], [], [], []
    res = None
    for it in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        det.detect_lines_batch(grays, 15.0, cap=a.cap)
        t1 = time.perf_counter()
        res = det.detect_descrip_lines_batch(grays, 15.0, cap=a.cap)
        t2 = time.perf_counter()
        pairs = [(res[i][1], res[(i + 1) % len(res)][1]) for i in range(len(res))]
        t3 = time.perf_counter()
        det.match_lines_batch(pairs)
        t4 = time.perf_counter()
        if it >= a.warmup:
            tm = det.lbd_timing()
            t_det.append((t1 - t0) * 1e3); t_desc.append((t2 - t1) * 1e3); t_match.append((t4 - t3) * 1e3)
            k_desc.append(tm["describe_kernel_ms"]); k_match.append(tm["match_kernel_ms"])
    n_lines = sum(len(k) for k, _ in res)
    med = statistics.median
    lines = [
        "lbd_quick: %d images of 376 x 1241, %d lines in all (%.1f per image), median of %d repetitions after %d warm-up, ms per batch" % (a.images, n_lines, n_lines / a.images, a.reps, a.warmup),
        "  map format read by the describe kernel: the detector's packed 3 bytes per pixel, no unpack pass (chosen by measurement against a short2 map: profiles/lbd_quick.txt)",
        "  cs_detect_lines_batch            %8.3f   (min %.3f)" % (med(t_det), min(t_det)),
        "  cs_detect_descrip_lines_batch    %8.3f   (min %.3f)" % (med(t_desc), min(t_desc)),
        "  difference = cost of describing  %8.3f" % (med(t_desc) - med(t_det)),
        "  lbd_describe_kernel (events)     %8.3f   (min %.3f)" % (med(k_desc), min(k_desc)),
        "  cs_lbd_match_batch, %d pairs     %8.3f   (min %.3f)   lbd_match_kernel (events) %.3f" % (len(res), med(t_match), min(t_match), med(k_match)),
    ]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    det.close()


if __name__ == "__main__":
    main()
