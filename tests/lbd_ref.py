"""The reference of the line band descriptor tests: a numpy restatement of BinaryDescriptor::computeLBD + binaryConversion
(line_lbd/libs/binary_descriptor.cpp:1150-1513, :405-416, :769-773; weights :146-177) under the numerical contract at the top of
cube_slam_wu_amd/csrc/cs_lbd.h, and a brute-force Hamming matcher.

Every intermediate is a value of `dtype` (np.float32 for the reference proper; np.float64 for its twin, the same formulas carried in
double, which only serves to show how far rounding alone moves the bits).  The 63 support rows of a line are independent of each other,
so they are carried side by side as arrays of 63 -- each element still sees exactly the reference's sequence of single operations (numpy
rounds every elementwise operation on its own and fuses nothing); where the ORDER of a sum matters (pixels along a row, rows into a band,
the normalisations) the sum is a Python loop in that order.  Nothing is np.sum()ed."""
import math

import numpy as np

BAND_W, BANDS, ROWS = 7, 9, 63
COMBINATIONS = [(0, 1), (0, 2), (0, 3), (0, 4), (0, 5), (0, 6), (1, 2), (1, 3), (1, 4), (1, 5), (1, 6), (2, 3), (2, 4), (2, 5), (2, 6), (2, 7), (2, 8),
                (3, 4), (3, 5), (3, 6), (3, 7), (3, 8), (4, 5), (4, 6), (4, 7), (4, 8), (5, 6), (5, 7), (5, 8), (6, 7), (6, 8), (7, 8)]
KEYLINE = np.dtype([("sx", np.float32), ("sy", np.float32), ("ex", np.float32), ("ey", np.float32), ("direction", np.float32), ("num_pixels", np.int32)])


def keylines(rows):
    """[(sx, sy, ex, ey, direction, num_pixels), ...] -> structured array"""
    out = np.zeros(len(rows), KEYLINE)
    for i, r in enumerate(rows):
        out[i] = tuple(r)
    return out


def weights():
    """gaussCoefG_ (63) and gaussCoefL_ (21) in double, with the reference's integer divisions (u = 10, sigma = 7; u = sigma = 31)"""
    u, sigma = float((BAND_W * 3 - 1) // 2), float((BAND_W * 2 + 1) // 2)
    inv = -1 / (2 * sigma * sigma)
    wl = [math.exp((i - u) * (i - u) * inv) for i in range(3 * BAND_W)]
    u = float((BANDS * BAND_W - 1) // 2)
    inv = -1 / (2 * u * u)
    wg = [math.exp((i - u) * (i - u) * inv) for i in range(ROWS)]
    return wg, wl


def sobel_maps(gray):
    """dxImg / dyImg of BinaryDescriptor::computeSobel (:352-402): GaussianBlur 5 x 5 sigma 1 (the oracle's integer blur), then the 3 x 3 Sobel in
    integers, borders reflected without the edge pixel (BORDER_REFLECT_101)."""
    from oracle import edlines_oracle_py
    b = np.pad(edlines_oracle_py.blur(gray).astype(np.int32), 1, mode="reflect")
    dx = (b[:-2, 2:] + 2 * b[1:-1, 2:] + b[2:, 2:]) - (b[:-2, :-2] + 2 * b[1:-1, :-2] + b[2:, :-2])
    dy = (b[2:, :-2] + 2 * b[2:, 1:-1] + b[2:, 2:]) - (b[:-2, :-2] + 2 * b[:-2, 1:-1] + b[:-2, 2:])
    return dx.astype(np.int16), dy.astype(np.int16)


def _roundf(x):
    """round half away from zero (roundf), exact: x - trunc(x) is exact in any binary format"""
    t = np.trunc(x)
    return t + np.where(np.abs(x - t) >= 0.5, np.copysign(1.0, x), 0.0).astype(x.dtype)


def describe_one(dxf, dyf, kl, wg, wl, T):
    """One keyline record -> 72 values of type T.  dxf / dyf: the maps as arrays of T."""
    H, W = dxf.shape
    n = int(kl["num_pixels"])
    direction = float(np.float32(kl["direction"]))
    dl0, dl1 = T(math.cos(direction)), T(math.sin(direction))          # float32: (float)cos((double)direction); float64: the double itself
    do0, do1 = -dl1, dl0
    half_w, half_h = T(int((n - 1) / 2)), T((ROWS - 1) // 2)           # C's division truncates towards zero: (0 - 1) / 2 = 0
    mx, my = T(0.5 * (float(kl["sx"]) + float(kl["ex"]))), T(0.5 * (float(kl["sy"]) + float(kl["ey"])))
    x0s, y0s = T(T(T(-dl0 * half_w) + T(dl1 * half_h)) + mx), T(T(T(-dl1 * half_w) - T(dl0 * half_h)) + my)
    # row starts: h running updates each
    x0, y0 = np.full(ROWS, x0s, T), np.full(ROWS, y0s, T)
    for k in range(1, ROWS):
        x0[k:] = x0[k:] - dl1
        y0[k:] = y0[k:] + dl0
    pl, nl, po, no = (np.zeros(ROWS, T) for _ in range(4))
    x, y = x0.copy(), y0.copy()
    for _ in range(n):
        xc = np.clip(_roundf(x), 0, W - 1).astype(np.int64)
        yc = np.clip(_roundf(y), 0, H - 1).astype(np.int64)
        dx, dy = dxf[yc, xc], dyf[yc, xc]
        gl = dx * dl0 + dy * dl1
        go = dx * do0 + dy * do1
        pl, nl = np.where(gl > 0, pl + gl, pl), np.where(gl > 0, nl, nl - gl)
        po, no = np.where(go > 0, po + go, po), np.where(go > 0, no, no - go)
        x = x + dl0
        y = y + dl1
    rows = np.stack([pl, nl, po, no], axis=1)                          # [63][4]
    band = np.zeros((BANDS, 4), T)
    band2 = np.zeros((BANDS, 4), T)
    for h in range(ROWS):
        r = T(wg[h]) * rows[h]
        r2 = r * r
        b, k = h // BAND_W, h % BAND_W
        for bb, c in ((b, wl[k + BAND_W]), (b - 1, wl[k + 2 * BAND_W]), (b + 1, wl[k])):        # own band, the band above, the band below
            if 0 <= bb < BANDS:
                c = T(c)
                band[bb] = band[bb] + c * r
                band2[bb] = band2[bb] + (c * c) * r2
    des = np.zeros(8 * BANDS, T)
    inv2, inv3 = T(1.0 / (BAND_W * 2.0)), T(1.0 / (BAND_W * 3.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        for b in range(BANDS):
            inv = inv2 if b in (0, BANDS - 1) else inv3
            mean = band[b] * inv
            des[8 * b:8 * b + 4] = mean
            des[8 * b + 4:8 * b + 8] = np.sqrt(band2[b] * inv - mean * mean)
        tm, ts = T(0), T(0)
        for b in range(BANDS):
            for k in range(4):
                tm = T(tm + T(des[8 * b + k] * des[8 * b + k]))
            for k in range(4, 8):
                ts = T(ts + T(des[8 * b + k] * des[8 * b + k]))
        tm, ts = T(T(1) / np.sqrt(tm)), T(T(1) / np.sqrt(ts))
        scale = np.tile(np.array([tm] * 4 + [ts] * 4, T), BANDS)
        des = des * scale
        des = np.where(des.astype(np.float64) > 0.4, T(np.float32(0.4)), des)      # compares against the double 0.4, stores 0.4f; NaN stays
        t = T(0)
        for i in range(8 * BANDS):
            t = T(t + T(des[i] * des[i]))
        t = T(T(1) / np.sqrt(t))
        des = des * t
    assert des.dtype == T
    return des


def binarise(des):
    out = np.zeros(32, np.uint8)
    for c, (a, b) in enumerate(COMBINATIONS):
        v = 0
        for i in range(8):
            if des[8 * a + i] > des[8 * b + i]:
                v |= 1 << i
        out[c] = v
    return out


def describe(dx, dy, kls, dtype=np.float32):
    """(dx, dy, keyline records) -> ((n, 32) uint8, (n, 72) dtype)"""
    T = dtype
    wg, wl = weights()
    dxf, dyf = np.asarray(dx).astype(T), np.asarray(dy).astype(T)
    d72 = np.zeros((len(kls), 72), T)
    d32 = np.zeros((len(kls), 32), np.uint8)
    for i in range(len(kls)):
        d72[i] = describe_one(dxf, dyf, kls[i], wg, wl, T)
        d32[i] = binarise(d72[i])
    return d32, d72


def hamming(q, t):
    q, t = np.asarray(q, np.uint8).reshape(-1, 32), np.asarray(t, np.uint8).reshape(-1, 32)
    return np.unpackbits(q[:, None, :] ^ t[None, :, :], axis=2).sum(axis=2).astype(np.int32)


def match(q, t):
    """brute force: (train_idx, dist, dist2) per query row; the first minimum wins; -1 where there is no (second) train row"""
    D = hamming(q, t)
    nq, nt = D.shape
    if nt == 0:
        return np.full(nq, -1, np.int32), np.full(nq, -1, np.int32), np.full(nq, -1, np.int32)
    idx = np.argmin(D, axis=1).astype(np.int32)
    dist = D[np.arange(nq), idx]
    dist2 = np.sort(D, axis=1)[:, 1] if nt > 1 else np.full(nq, -1, np.int32)
    return idx, dist.astype(np.int32), dist2.astype(np.int32)


def same_floats(a, b):
    """bit equality with NaN equal to NaN (a NaN's sign and payload are not part of the contract)"""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return a.shape == b.shape and bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))))
