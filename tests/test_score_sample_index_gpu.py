"""The scorer's distance-map index (detect_kernels.hip: score_sample_index -- the reference's two integer casts, row * width + column)
on the device through cs_check_score_sample_index, one sample per lane, against numpy; and the double-precision sum every lane forms
right behind it, which tells whether the index function left the lane's rounding mode as the rest of the scorer's arithmetic needs it."""
import numpy as np
import pytest

from cube_slam_wu_amd import capi

pytestmark = pytest.mark.gpu

LIMIT = 4096            # coordinates and map widths of the cases: [0, LIMIT)
PROBE_A, PROBE_B = 1.0, float.fromhex("0x1.8p-53")      # 1 + 2^-52 rounded to nearest, 1 rounded toward zero


def _coordinates(rng, n_random):
    k = np.arange(LIMIT, dtype=np.float64)
    below = np.nextafter(k[1:], -np.inf)        # the double below every integer from 1 on: truncates to k - 1
    above = np.nextafter(k, np.inf)             # (above 0: the smallest subnormal)
    halves = k + 0.5
    special = np.array([0.0, -0.0, 5e-324, np.nextafter(float(LIMIT), 0.0)])
    return np.concatenate([k, below, above, halves, special, rng.uniform(0.0, LIMIT, n_random)])


def test_index_is_the_two_integer_casts_and_the_rounding_mode_is_round_to_nearest_in_every_lane():
    rng = np.random.default_rng(17)
    base = _coordinates(rng, 30_000)
    n = 100_003                                 # not a multiple of 64: the last wavefront is partly inactive
    assert n % 64 != 0 and n > 2 * len(base)
    # every listed coordinate once as the row and once as the column, each against a random partner; random pairs behind them
    other = rng.uniform(0.0, LIMIT, len(base))
    sy = np.concatenate([base, other, rng.uniform(0.0, LIMIT, n - 2 * len(base))])
    sx = np.concatenate([other, base, rng.uniform(0.0, LIMIT, n - 2 * len(base))])
    map_w = rng.integers(1, LIMIT, n).astype(np.int32)
    map_w[:LIMIT] = LIMIT - 1                   # the widest map against the integer rows
    assert len(sy) == len(sx) == n
    a, b = np.full(n, PROBE_A), np.full(n, PROBE_B)

    idx, probe = capi.check_score_sample_index(sy, sx, map_w, a, b)

    ref = np.trunc(sy).astype(np.int64) * map_w.astype(np.int64) + np.trunc(sx).astype(np.int64)
    assert ref.min() >= 0 and ref.max() < 2 ** 31
    bad = np.flatnonzero(idx.astype(np.int64) != ref)
    assert len(bad) == 0, (len(bad), bad[:10], sy[bad[:10]], sx[bad[:10]], map_w[bad[:10]], idx[bad[:10]], ref[bad[:10]])
    want = a + b
    assert want[0] == 1.0 + 2.0 ** -52          # numpy rounds to nearest: the probe distinguishes the two modes
    bad = np.flatnonzero(probe.view(np.int64) != want.view(np.int64))
    assert len(bad) == 0, (len(bad), bad[:10], probe[bad[:10]])
