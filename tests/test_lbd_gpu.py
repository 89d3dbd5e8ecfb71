"""Line band descriptors and their Hamming matching on the device (cs_lbd_describe_gray, cs_detect_descrip_lines_gray / _batch, cs_lbd_match /
_batch) against tests/lbd_ref.py: the numpy float32 restatement of computeLBD + binaryConversion under the contract of csrc/cs_lbd.h -- bit for
bit, NaN equal to NaN -- and a brute-force matcher.  The same inputs go through a host build of the same functions in tests/test_lbd_host_cpu.py."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import lbd_cases
import lbd_ref
from cube_slam_wu_amd import capi
from oracle import edlines_oracle_py as L

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def det():
    d = capi.Detector(capi.default_params())
    yield d
    d.close()


def _reference(gray, kl):
    dx, dy = lbd_ref.sobel_maps(gray)
    return lbd_ref.describe(dx, dy, kl)


# ---- describe -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["explicit", "small", "flat", "ramp"])
def test_describe_explicit_records_equal_the_restatement_bit_for_bit(det, name):
    """explicit: 64 x 48 half-planes + noise; lines along each border, one partly outside, num_pixels 0, 1, 2, 15, 16, 63, 64, 65, 200, directions
    0, +-pi/2, pi, -pi and one per quadrant, mid-points at k + 0.5.  small: 40 x 40, smaller than the 63-row support.  flat: all 72 floats NaN and
    all 32 bytes zero -- as the reference has them.  ramp: single-signed gradients, sums and variances that are exactly zero."""
    gray, kl, ref32, ref72 = lbd_cases.case(name)
    got32, got72 = det.describe_lines(gray, kl, want_float=True)
    assert np.array_equal(got32, ref32)
    assert lbd_ref.same_floats(got72, ref72)
    assert np.array_equal(det.describe_lines(gray, kl), ref32)          # desc72 == NULL
    if name == "flat":
        assert np.isnan(ref72).all() and not ref32.any()


def test_describe_empty_input_writes_nothing(det):
    gray = lbd_cases.case("explicit")[0]
    d32 = np.full((2, 32), 0xAB, np.uint8)
    d72 = np.full((2, 72), 7.0, np.float32)
    rc = capi.lib().cs_lbd_describe_gray(det.h, gray.ctypes.data_as(C.POINTER(C.c_ubyte)), 64, 48, None, 0, C.c_void_p(d32.ctypes.data), C.c_void_p(d72.ctypes.data))
    assert rc == 0 and (d32 == 0xAB).all() and (d72 == 7.0).all()
    assert det.describe_lines(gray, np.zeros(0, capi.KEYLINE_DTYPE)).shape == (0, 32)


def test_describe_argument_checks(det):
    gray, kl = lbd_cases.case("explicit")[:2]
    one = np.array(kl[6:7])
    d32 = np.zeros((1, 32), np.uint8)
    wide = np.zeros((3, 40000), np.uint8)
    args = lambda g, k: (det.h, g.ctypes.data_as(C.POINTER(C.c_ubyte)), int(g.shape[1]), int(g.shape[0]), C.c_void_p(k.ctypes.data), 1, C.c_void_p(d32.ctypes.data), None)
    assert capi.lib().cs_lbd_describe_gray(*args(wide, one)) == -1                     # CS_ERR_INVALID_ARG: the reference indexes with short
    n = C.c_int()
    assert capi.lib().cs_detect_descrip_lines_gray(det.h, wide.ctypes.data_as(C.POINTER(C.c_ubyte)), 40000, 3, C.c_double(15.0), C.c_void_p(one.ctypes.data), C.c_void_p(d32.ctypes.data), 1, C.byref(n)) == -1
    bad = one.copy(); bad["num_pixels"] = -1
    assert capi.lib().cs_lbd_describe_gray(*args(gray, bad)) == -1
    bad = one.copy(); bad["num_pixels"] = 32768
    assert capi.lib().cs_lbd_describe_gray(*args(gray, bad)) == -1
    for field in ("sx", "ey", "direction"):
        for v in (np.nan, np.inf):
            bad = one.copy(); bad[field] = v
            assert capi.lib().cs_lbd_describe_gray(*args(gray, bad)) == -1
    with pytest.raises(RuntimeError):
        det.describe_lines(gray, bad)
    assert capi.lib().cs_lbd_describe_gray(*args(gray, one)) == 0


# ---- detect + describe ----------------------------------------------------------------------------------------------------------
def _check_records(det, gray, thr, kl, d32):
    seg = det.detect_lines(gray, thr)
    assert len(kl) == len(seg) == len(d32)
    got = np.stack([kl["sx"], kl["sy"], kl["ex"], kl["ey"]], axis=1) if len(kl) else np.zeros((0, 4), np.float32)
    assert np.array_equal(got, seg)                                      # which the existing tests pin to the oracle
    ref32, _ = _reference(gray, kl)
    assert np.array_equal(d32, ref32)
    for k in kl:
        # loose sanity bounds: the exact record is not observable through the oracle
        a = math.atan2(float(k["ey"]) - float(k["sy"]), float(k["ex"]) - float(k["sx"]))
        d = (a - float(k["direction"]) + math.pi) % (2 * math.pi) - math.pi
        assert abs(d) < 0.2, (k, a)
        chebyshev = max(abs(float(k["ex"]) - float(k["sx"])), abs(float(k["ey"]) - float(k["sy"]))) + 1
        assert k["num_pixels"] >= 15 and chebyshev / 2 <= k["num_pixels"] <= 2 * chebyshev, (k, chebyshev)


@pytest.mark.parametrize("frame", [0, 20, 45, "cuboid"])
def test_detect_descrip_lines_on_the_reference_frames(det, frame):
    if frame == "cuboid":
        from PIL import Image
        gray = np.ascontiguousarray(np.asarray(Image.open(os.path.join(GOLDEN, "detect_3d_cuboid_data", "0000_gray.png"))))
    else:
        gray = lbd_cases.tum_gray(frame)
    kl, d32 = det.detect_descrip_lines(gray, 15.0)
    assert len(kl) > 0
    _check_records(det, gray, 15.0, kl, d32)
    assert np.array_equal(np.stack([kl["sx"], kl["sy"], kl["ex"], kl["ey"]], axis=1), L.detect_filter_lines(gray, 15.0))


def test_detect_descrip_lines_flat_image_and_small_cap(det):
    kl, d32 = det.detect_descrip_lines(np.full((120, 160), 77, np.uint8))
    assert kl.shape == (0,) and d32.shape == (0, 32)
    gray = lbd_cases.tum_gray(20)
    with pytest.raises(RuntimeError, match="cap"):
        det.detect_descrip_lines(gray, 15.0, cap=3)
    n = C.c_int()
    kl, d32 = np.zeros(3, capi.KEYLINE_DTYPE), np.zeros((3, 32), np.uint8)
    rc = capi.lib().cs_detect_descrip_lines_gray(det.h, gray.ctypes.data_as(C.POINTER(C.c_ubyte)), 640, 480, C.c_double(15.0), C.c_void_p(kl.ctypes.data), C.c_void_p(d32.ctypes.data), 3, C.byref(n))
    assert rc == -4 and "cap" in capi.last_error()                       # CS_ERR_CAPACITY


def test_detect_descrip_lines_without_a_length_filter(det):
    """length_thres < 0 (the Mat overload): every validated line, the filtered call's lines among them in order."""
    gray = lbd_cases.synthetic(np.random.default_rng(77), 97, 131)
    kl_all, d_all = det.detect_descrip_lines(gray, -1.0)
    kl, d32 = det.detect_descrip_lines(gray, 30.0)
    assert 0 < len(kl) < len(kl_all)
    length = np.hypot(kl_all["ex"] - kl_all["sx"], kl_all["ey"] - kl_all["sy"])
    assert kl_all[length > 31].tobytes() == kl[np.hypot(kl["ex"] - kl["sx"], kl["ey"] - kl["sy"]) > 31].tobytes()
    assert np.array_equal(d_all, _reference(gray, kl_all)[0])


def test_batch_equals_the_single_image_calls(det):
    """9 synthetic 200 x 311 images: the batch (all lines described in one launch over the resident maps of the whole batch) equals the single-image
    calls, also on a second call and after a call with a different image size; detect_lines afterwards still equals the oracle."""
    grays = [lbd_cases.synthetic(np.random.default_rng(40 + i), 200, 311) for i in range(9)]
    single = [det.detect_descrip_lines(g, 15.0) for g in grays]
    assert all(len(k) > 0 for k, _ in single)
    kl0, d0 = single[0]
    assert np.array_equal(d0, _reference(grays[0], kl0)[0])
    def same(got, want):
        assert len(got) == len(want)
        for (ka, da), (kb, db) in zip(got, want):
            assert ka.tobytes() == kb.tobytes() and np.array_equal(da, db)
    for _ in range(2):
        same(det.detect_descrip_lines_batch(grays, 15.0), single)
    small = lbd_cases.synthetic(np.random.default_rng(7), 97, 120)
    same(det.detect_descrip_lines_batch([small], 15.0), [det.detect_descrip_lines(small, 15.0)])
    same(det.detect_descrip_lines_batch(grays[:3], 15.0), single[:3])
    assert np.array_equal(det.detect_lines(grays[4], 15.0), L.detect_filter_lines(grays[4], 15.0))
    assert det.lbd_timing()["describe_kernel_ms"] > 0


# ---- matching -------------------------------------------------------------------------------------------------------------------
def _descriptors(rng, nq, nt):
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    if nt >= 60 and nq >= 3:
        t[40] = t[7]; t[55] = t[7]            # duplicates: the lowest row wins a tie
        q[0] = t[7]                           # identical: distance 0 (three ways)
        q[1] = ~t[11]                         # complement: distance 256 from row 11
        q[2] = t[20]; q[2, 3] ^= 0x10         # one bit from row 20
    return q, t


def _check_match(det, q, t):
    idx, dist, dist2 = det.match_lines(q, t)
    r_idx, r_dist, r_dist2 = lbd_ref.match(q, t)
    assert idx.dtype == np.int32 and np.array_equal(idx, r_idx) and np.array_equal(dist, r_dist) and np.array_equal(dist2, r_dist2)
    return idx, dist, dist2


@pytest.mark.parametrize("nq,nt", [(1, 1), (3, 0), (0, 3), (1, 257), (65, 63), (130, 300)])
def test_match_equals_the_numpy_brute_force(det, nq, nt):
    q, t = _descriptors(np.random.default_rng(1000 * nq + nt), nq, nt)
    idx, dist, dist2 = _check_match(det, q, t)
    assert len(idx) == nq
    if nt == 0:
        assert (idx == -1).all() and (dist == -1).all() and (dist2 == -1).all()
    if nt == 1:
        assert (dist2 == -1).all()
    if nt >= 60 and nq >= 3:
        assert idx[0] == 7 and dist[0] == 0 and dist2[0] == 0
        assert lbd_ref.hamming(q[1:2], t)[0, 11] == 256 and idx[1] != 11
        assert idx[2] == 20 and dist[2] == 1


def test_match_line_descrip_keeps_exactly_the_distances_below_the_threshold(det):
    rng = np.random.default_rng(9)
    q, t = _descriptors(rng, 20, 80)
    def flip(row, nbits):
        out = row.copy()
        for b in range(nbits):
            out[b // 8] ^= 1 << (b % 8)
        return out
    q[5], q[6] = flip(t[30], 24), flip(t[31], 25)
    m = det.match_line_descrip(q, t, 25.0)
    idx, dist, _ = lbd_ref.match(q, t)
    keep = np.nonzero(dist < 25)[0]
    assert np.array_equal(m, np.stack([keep, idx[keep], dist[keep]], axis=1))
    assert [5, 30, 24] in m.tolist() and 6 not in m[:, 0] and dist[6] == 25


def test_match_batch_equals_the_per_pair_calls(det):
    rng = np.random.default_rng(12)
    pairs = [_descriptors(rng, nq, nt) for nq, nt in ((70, 90), (3, 1), (0, 0), (129, 64), (5, 200))]
    idx, dist, dist2 = det.match_lines_batch(pairs)
    for p, (q, t) in enumerate(pairs):
        a, b, c = det.match_lines(q, t)
        assert np.array_equal(idx[p], a) and np.array_equal(dist[p], b) and np.array_equal(dist2[p], c)
        r = lbd_ref.match(q, t)
        assert np.array_equal(a, r[0]) and np.array_equal(b, r[1]) and np.array_equal(c, r[2])
    assert det.lbd_timing()["match_kernel_ms"] > 0


def test_end_to_end_frames_20_and_21(det):
    """detect + describe both frames, match them: the matcher's result on the device's descriptors equals the numpy matcher on the reference's."""
    g0, g1 = lbd_cases.tum_gray(20), lbd_cases.tum_gray(21)
    (k0, d0), (k1, d1) = det.detect_descrip_lines(g0, 15.0), det.detect_descrip_lines(g1, 15.0)
    r0, r1 = _reference(g0, k0)[0], _reference(g1, k1)[0]
    idx, dist, dist2 = det.match_lines(d0, d1)
    r = lbd_ref.match(r0, r1)
    assert np.array_equal(idx, r[0]) and np.array_equal(dist, r[1]) and np.array_equal(dist2, r[2])
    good = det.match_line_descrip(d0, d1, 25.0)
    assert len(good) > 0                                                 # (how many is data)
