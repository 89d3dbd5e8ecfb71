"""cs_atan2_lean (cube_slam_wu_amd/csrc/cs_atan2_lean.h) on the host: wherever it accepts it returns cs_atan2's bits, it declines
every special argument pair and few ordinary ones, and the error of its evaluation stays four times below the bound of its rounding
test.  It consists of IEEE-exact operations only, so these tests speak for the device as well (tests/test_atan2_lean_gpu.py runs it there)."""
import ctypes as C

import mpmath
import numpy as np

import atan2_lean_cases as cases

N_PER_KIND = 4_000_000
KINDS = {0: "uniform coordinates in +-1500", 1: "integer differences", 2: "half-pixel differences", 3: "exponent spreads of +-60",
         4: "quotients next to the table cell edges, four sign combinations, both argument orders"}


def test_accepted_values_are_cs_atan2_bit_for_bit_and_few_ordinary_arguments_are_declined():
    """Five kinds of 4 M argument pairs each (tests/atan2_lean_shim.cpp: lean_compare).  No accepted value differs from cs_atan2's;
    no special pair (a zero difference, on the integer and half-pixel grids) is accepted; the share of ordinary pairs that the
    rounding test declines stays below 5e-4.  Measured, in the order of the kinds: 4.4e-5, 5.0e-5, 4.1e-5, 4.0e-5, 3.9e-5
    (bound 2^-68 against roundings at 2^-53: 2 * 2^-15 of the values in the upper half of a binade, half as many in the lower half)."""
    L = cases.shim()
    for kind in KINDS:
        dec, spc = C.c_longlong(0), C.c_longlong(0)
        bad = L.lean_compare(N_PER_KIND, 99 + kind, kind, C.byref(dec), C.byref(spc))
        rate = dec.value / N_PER_KIND
        print("kind %d (%s): %d differences, %d special pairs, ordinary pairs declined: %.3g" % (kind, KINDS[kind], bad, spc.value, rate))
        assert bad == 0, (kind, bad)
        assert rate < 5e-4, (kind, rate)
        if kind in (1, 2):
            assert spc.value > 0       # the grids do produce zero differences
        else:
            assert spc.value == 0


def test_the_scorers_own_operands():
    """The six edge differences per proposal that score_kernel evaluates (its ID1 / ID2 tables), from the oracle's candidate corners of
    two half-degree frames: every proposal the two frames have (4 261 proposals, 25 566 pairs: the frames, not a count, define this kind).
    Measured: no special pair, 3.9e-5 of the pairs declined."""
    y, x = cases.scorer_operands()
    assert len(y) >= 6 * 4000
    ref, out, acc, spc, bad = cases.lean_batch(y, x)
    rate = np.count_nonzero(~acc & ~spc) / len(y)
    print("scorer operands: %d pairs, %d special, %d differences, ordinary pairs declined: %.3g" % (len(y), np.count_nonzero(spc), bad, rate))
    assert bad == 0
    assert not (acc & spc).any()
    assert np.array_equal(out[acc].view(np.int64), ref[acc].view(np.int64))
    assert rate < 5e-4


def test_special_arguments_are_declined():
    """Every pair from test_special_values_follow_ieee's list: zeros, infinities, NaN, subnormals, and quotients too small to scale."""
    L = cases.shim()
    for y in cases.SPECIAL_VALUES:
        for x in cases.SPECIAL_VALUES:
            hi, lo, bound = C.c_double(), C.c_double(), C.c_double()
            ordinary = L.lean_value(y, x, C.byref(hi), C.byref(lo), C.byref(bound))
            _, _, acc, spc, _ = cases.lean_batch([y], [x])
            if spc[0]:
                assert not acc[0] and not ordinary, (y, x)
    # of the list, only pairs of two ordinary magnitudes (1, 3, 1e-200, 1e200, 1e308 and their negatives) may be accepted
    ordinary_vals = [v for v in cases.SPECIAL_VALUES if v in (1.0, -1.0, 3.0, 1e-200, 1e200, 1e308, -1e308)]
    yy, xx = np.meshgrid(cases.SPECIAL_VALUES, cases.SPECIAL_VALUES)
    ref, out, acc, spc, bad = cases.lean_batch(yy.ravel(), xx.ravel())
    assert bad == 0
    for y, x, a in zip(yy.ravel(), xx.ravel(), acc):
        if a:
            assert y in ordinary_vals and x in ordinary_vals, (y, x)
    assert acc.any()
    # the cut on the scaled smaller magnitude: 2^-200 is taken, the next double below is not
    _, _, acc, _, _ = cases.lean_batch([2.0 ** -200, np.nextafter(2.0 ** -200, 0), 1.5 * 2.0 ** -181, 1.75 * 2.0 ** 823], [1.0, 1.0, 1.9 * 2.0 ** 20, -1.2 * 2.0 ** 1023])
    assert list(acc) == [True, False, False, True]


def test_evaluation_error_stays_four_times_below_the_bound():
    """The rounding test is sound only if hi + lo of the lean evaluation, octant reflection included, is closer to the true angle than
    the bound it assumes.  The cases of test_fast_path_error_stays_four_times_below_its_bound (tests/test_atan2.py), each in the four
    (swap, x < 0) arrangements, against mpmath at 300 bits.  Measured: worst relative error 2^-70.5 against the bound 2^-68."""
    L = cases.shim()
    mpmath.mp.prec = 300
    rng = np.random.default_rng(5)
    pairs = []
    for _ in range(3000):
        big = 1 + rng.random()
        pairs.append((big * rng.random(), big))
        i = rng.integers(0, 257)
        pairs.append((min(max(big * ((i + (rng.random() - 0.5) * 1.02) / 256), 1e-9), big), big))   # edges of the table cells
        big = 2 - rng.random() * 1e-6
        pairs.append((big * rng.random(), big))
        big = 1 + rng.random()
        pairs.append((big * 2.0 ** (-rng.random() * 60), big))
    worst, bound = mpmath.mpf(0), None
    for small, big in pairs:
        small, big = float(small), float(big)
        for y, x in ((small, big), (big, small), (small, -big), (big, -small)):
            hi, lo, b = C.c_double(), C.c_double(), C.c_double()
            assert L.lean_value(y, x, C.byref(hi), C.byref(lo), C.byref(b)) == 1
            bound = b.value
            exact = mpmath.atan2(mpmath.mpf(y), mpmath.mpf(x))
            worst = max(worst, abs(abs(mpmath.mpf(hi.value) + mpmath.mpf(lo.value)) - exact) / exact)     # (the sum may carry the negated angle)
    print("worst relative error of hi + lo: 2^%.2f; bound 2^%.2f" % (float(mpmath.log(worst, 2)), float(mpmath.log(bound, 2))))
    assert bound == 2.0 ** -68
    assert 4 * worst <= mpmath.mpf(bound)
