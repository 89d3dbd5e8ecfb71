"""Inputs of the line band descriptor tests, shared by the host-only test (tests/test_lbd_host_cpu.py) and the device test
(tests/test_lbd_gpu.py): images and explicit keyline records that reach every branch of the support-region walk, and the reference's
descriptors of each, computed once per process."""
import functools
import math
import os

import numpy as np

import lbd_ref

DATA = os.path.join(os.path.dirname(__file__), "golden", "object_slam_data")
PI32 = float(np.float32(math.pi))


def synthetic(rng, h, w):
    """half-planes + noise"""
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.full((h, w), 100.0)
    for _ in range(12):
        a = rng.uniform(0, np.pi)
        img += np.where((xx - rng.uniform(0, w)) * np.cos(a) + (yy - rng.uniform(0, h)) * np.sin(a) > 0, rng.uniform(-60, 60), 0)
    img += rng.normal(0, 3, (h, w))
    return np.clip(img, 0, 255).astype(np.uint8)


def tum_gray(k):
    from PIL import Image
    from oracle import edge_oracle_py as E
    img = np.asarray(Image.open(os.path.join(DATA, "raw_imgs", "%04d_rgb_raw.jpg" % k)).convert("RGB"))
    return E.bgr_to_gray(np.ascontiguousarray(img[:, :, ::-1]))


def explicit_records(w, h):
    """Lines along each border (the support region clamps), one partly outside the image (negative coordinates: round(-0.5) = -1, clamp to 0),
    every length class (0, 1, 2, 15, 16, 63, 64, 65 and 200, which is longer than the image), the axis directions (0, +-pi/2, pi, -pi: (float)cos(pi/2)
    is not zero), one direction per quadrant, and axis-aligned lines whose mid-point is k + 0.5 (roundf and rintf part there)."""
    hp = PI32 / 2
    rows = [
        # hugging the four borders
        (2.0, 0.0, w - 3.0, 0.0, 0.0, w - 4), (2.0, h - 1.0, w - 3.0, h - 1.0, PI32, w - 4),
        (0.0, 3.0, 0.0, h - 4.0, hp, h - 6), (w - 1.0, h - 4.0, w - 1.0, 3.0, -hp, h - 6),
        # partly outside
        (-12.5, -7.5, 20.0, 9.0, 0.47, 37), (w - 6.0, h - 3.0, w + 14.0, h + 11.5, 0.61, 25),
        # one direction per quadrant, through the middle
        (10.0, 8.0, 40.0, 30.0, 0.63, 31), (40.0, 8.0, 12.0, 33.0, 2.41, 29), (44.0, 35.0, 9.0, 11.0, -2.5, 36), (11.0, 40.0, 50.0, 12.0, -0.62, 40),
        (30.0, 20.0, 10.0, 20.0, -PI32, 21),
        # mid-point at k + 0.5
        (10.0, 20.0, 25.0, 20.0, 0.0, 16), (31.0, 5.0, 31.0, 20.0, hp, 16), (10.5, 24.5, 26.5, 24.5, 0.0, 17), (20.0, 30.0, 5.0, 30.0, PI32, 16),
    ]
    for n in (0, 1, 2, 15, 16, 63, 64, 65, 200):
        rows.append((12.0, 14.0, 12.0 + 0.8 * n, 14.0 + 0.6 * n, 0.6435011, n))
    return lbd_ref.keylines(rows)


def oracle_records(gray, thr=15.0):
    """The oracle's segments as keyline records: num_pixels = max(|dx|, |dy|) + 1 of the rounded end points, direction = atan2f."""
    from oracle import edlines_oracle_py as L
    seg = L.detect_filter_lines(gray, thr)
    rows = []
    for x1, y1, x2, y2 in seg:
        rx1, ry1, rx2, ry2 = (int(math.floor(float(v) + 0.5)) for v in (x1, y1, x2, y2))
        n = max(abs(rx2 - rx1), abs(ry2 - ry1)) + 1
        d = np.arctan2(np.float32(y2) - np.float32(y1), np.float32(x2) - np.float32(x1), dtype=np.float32)
        rows.append((x1, y1, x2, y2, d, n))
    return lbd_ref.keylines(rows)


def ramp_image(h, w):
    """a ramp along x: each band has only one gradient sign, so some sums and variances are exactly zero"""
    return np.tile(np.clip(20 + 3 * np.arange(w), 0, 255).astype(np.uint8), (h, 1))


@functools.lru_cache(maxsize=None)
def case(name):
    """name -> (gray, records, ref desc32, ref desc72): the reference is computed once and shared (treat the arrays as read-only)"""
    if name == "explicit":
        gray = synthetic(np.random.default_rng(6448), 48, 64)
        kl = explicit_records(64, 48)
    elif name == "small":
        gray = synthetic(np.random.default_rng(4040), 40, 40)
        kl = explicit_records(40, 40)
    elif name == "flat":
        gray = np.full((48, 64), 77, np.uint8)
        kl = explicit_records(64, 48)[[0, 4, 6, 11, 15, 18]]
    elif name == "ramp":
        gray = ramp_image(48, 64)
        kl = explicit_records(64, 48)[[0, 2, 6, 7, 11, 12, 18, 21]]
    elif name.startswith("tum"):
        gray = tum_gray(int(name[3:]))
        kl = oracle_records(gray)
    else:
        raise KeyError(name)
    dx, dy = lbd_ref.sobel_maps(gray)
    d32, d72 = lbd_ref.describe(dx, dy, kl)
    for a in (gray, kl, d32, d72):
        a.setflags(write=False)
    return gray, kl, d32, d72
