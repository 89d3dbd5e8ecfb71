"""The scorer's atan2 call sequence on the device -- cs_atan2_lean, then cs_atan2 behind a wavefront vote for the lanes it declined
(detect_kernels.hip: score_atan2) -- against cs_atan2 on the host, bit for bit; and the angle-error column of the sweep against the oracle."""
import numpy as np
import pytest

from cube_slam_wu_amd import capi, synth
from oracle import oracle_py

import atan2_lean_cases as cases

pytestmark = pytest.mark.gpu

N_PAIRS = 64 * 1024 + 17        # the last wavefront is partial


def _pairs():
    """Argument pairs by wavefront of 64, every flag taken from the host shim beforehand: a background of accepted ordinary pairs (the
    scorer's own operands and uniform coordinates), then wavefronts 10-13 all special, 20 / 21 one special lane at lane 0 / lane 63,
    30 one declined ordinary pair, 31 five of them, 32 a declined ordinary pair next to a special one, and one declined ordinary pair
    in the partial last wavefront."""
    rng = np.random.default_rng(11)
    sy, sx = cases.scorer_operands()
    py = np.concatenate([sy, rng.uniform(-1500, 1500, 3_000_000)])
    px = np.concatenate([sx, rng.uniform(-1500, 1500, 3_000_000)])
    _, _, acc, spc, bad = cases.lean_batch(py, px)
    assert bad == 0
    good = np.flatnonzero(acc)[:N_PAIRS]
    declined = np.flatnonzero(~acc & ~spc)
    assert len(good) == N_PAIRS and len(declined) >= 8, (len(good), len(declined))
    y, x = py[good].copy(), px[good].copy()
    vals = cases.SPECIAL_VALUES
    special = [(a, b) for a in vals for b in vals]
    special = [p for p, s in zip(special, cases.lean_batch([p[0] for p in special], [p[1] for p in special])[3]) if s]
    assert len(special) > 100
    for q in range(4 * 64):
        y[10 * 64 + q], x[10 * 64 + q] = special[q % len(special)]
    y[20 * 64], x[20 * 64] = np.nan, 1.0
    y[21 * 64 + 63], x[21 * 64 + 63] = 0.0, -2.5
    put = [30 * 64 + 5, 31 * 64, 31 * 64 + 1, 31 * 64 + 17, 31 * 64 + 40, 31 * 64 + 63, 32 * 64 + 9, N_PAIRS - 3]
    for pos, src in zip(put, declined):
        y[pos], x[pos] = py[src], px[src]
    y[32 * 64 + 10], x[32 * 64 + 10] = -np.inf, np.inf
    return y, x


def test_device_call_sequence_equals_host_cs_atan2():
    y, x = _pairs()
    ref, _, acc, spc, bad = cases.lean_batch(y, x)
    assert bad == 0
    # the arrangement the docstring of _pairs promises
    n_w = (N_PAIRS + 63) // 64
    a_w = [acc[w * 64:(w + 1) * 64] for w in range(n_w)]
    s_w = [spc[w * 64:(w + 1) * 64] for w in range(n_w)]
    assert sum(a.all() for a in a_w) > 1000
    assert all(s_w[w].all() and not a_w[w].any() for w in range(10, 14))
    assert list(np.flatnonzero(~a_w[20])) == [0] and s_w[20][0] and list(np.flatnonzero(~a_w[21])) == [63] and s_w[21][63]
    assert list(np.flatnonzero(~a_w[30])) == [5] and not s_w[30].any()
    assert np.count_nonzero(~a_w[31]) == 5 and not s_w[31].any()
    assert list(np.flatnonzero(~a_w[32])) == [9, 10] and list(np.flatnonzero(s_w[32])) == [10]
    assert len(a_w[-1]) == 17 and np.count_nonzero(~a_w[-1]) == 1 and not s_w[-1].any()

    got, got_acc = capi.check_score_atan2(y, x)
    assert np.array_equal(got_acc, acc), np.flatnonzero(got_acc != acc)[:10]
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.int64), ref[~nan].view(np.int64)), np.flatnonzero(got.view(np.int64) != ref.view(np.int64))[:10]


def test_sweep_angle_error_column_equals_the_oracle():
    """Two half-degree frames and a three-box frame through the C ABI, configuration 1 and configuration 2 switched off in turn: the
    angle-error column of every candidate row."""
    frames = [synth.make_frame(seed, n_boxes=nb, n_lines=nl) for seed, nb, nl in cases.HALF_DEGREE_SEEDS] + [synth.make_frame(4243, n_boxes=3, n_lines=150)]
    cap = 20000
    for off in ("consider_config_1", "consider_config_2"):
        kw = {off: 0, "whether_sample_cam_roll_pitch": 0, "yaw_step_deg": 0.5}
        det = capi.Detector(capi.default_params(**kw))
        bat = capi.Batch(det, frames, debug=True)
        bat.run()
        rows_total = 0
        for f, fr in enumerate(frames):
            _, dbg = oracle_py.detect_cuboid(fr, oracle_py.default_params(**kw), atan2_mode=1, debug_cap=cap)
            for i in range(len(fr["boxes"])):
                for k in range(len(fr["maps"][i])):
                    slot = 3 * i + k
                    V = int(dbg["n_valid"][slot])
                    assert V <= cap
                    rows, _ = bat.debug_candidates(f, i, k, with_corners=False)
                    assert rows.shape[0] == V, (off, f, i, k)
                    assert np.array_equal(rows[:, 5], dbg["cand_rows"][slot][:V, 5]), (off, f, i, k)
                    rows_total += V
        assert rows_total > 256, (off, rows_total)          # (configuration 2 alone leaves a few hundred rows)
        bat.close()
        det.close()
