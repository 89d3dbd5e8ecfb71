"""The detector sweep on two hand-built frames, sized so that the loop structure of its kernels shows: candidate_compact_kernel's trips of
2 048 proposals per configuration and its job record (read once per workgroup), and the chunks of 64 staged segments whose survivors the
first pass of the VP support keeps as one bit each.  Everything the sweep produces is held to the oracle bit for bit, on the
path that keeps every candidate (tests/test_detect_gpu.py: _check) and on the production path (_check_final).

  frame "trips": box 0 is 300 px wide (15 top-edge samples) and the yaw sweep has 151 samples: 2 265 proposals per configuration, two
      trips, the second one 217 proposals long.  Box 1 is 10 px wide: ONE top-edge sample (T == 1: the division by T is not replaced by
      a multiplication), 151 proposals, one short trip.  No proposal of a box that narrow can pass the reference's 20-pixel edge tests
      -- two of its edges run between the box's sides along rays to two vanishing points 90 degrees of yaw apart, and only one of them
      can be steep -- so the oracle's count for it is 0 and the device's has to be 0 as well; every other box here has proposals.
      Box 2 (10 samples, 1 510 proposals) stays below one trip as well.  All eight bounds (raw box and expanded ROI) differ between consecutive
      boxes: a record kept from the previous workgroup's job, or a bound taken from the wrong field, changes the decisions.
  frame "masks": five boxes with disjoint ROIs that hold exactly 31, 32, 33, 64 and 65 merged segments: either side of bit 32 of a chunk's
      survivor mask, a full chunk, and a second chunk of one segment."""
import numpy as np
import pytest
from scipy import ndimage

from cube_slam_wu_amd import capi, synth
from oracle import oracle_py

import test_detect_gpu as detect_checks

pytestmark = pytest.mark.gpu

YAW_STEP = 0.6
SEGMENT_COUNTS = (31, 32, 33, 64, 65)


def _with_boxes(base, boxes, lines):
    """base's camera with the given boxes and segments: ROIs and distance maps rebuilt as synth.make_frame builds them."""
    fr = dict(base)
    fr["boxes"] = np.asarray(boxes, float)
    fr["lines"] = np.asarray(lines, float).reshape(-1, 4)
    fr["rois"] = [synth.box_rois(b, fr["img_w"], fr["img_h"]) for b in fr["boxes"]]
    maps = []
    for rr in fr["rois"]:
        mm = []
        for (l, t, w, h), _ in rr:
            edge = synth._rasterise(fr["lines"], l, t, w, h)
            buf = np.zeros(h * w + w + 1, np.float32)
            buf[: h * w] = (ndimage.distance_transform_edt(~edge) if edge.any() else np.full((h, w), 1e3)).astype(np.float32).ravel()
            mm.append(buf)
        maps.append(mm)
    fr["maps"] = maps
    return fr


def _frame_trips():
    base = synth.make_frame(9100, n_boxes=1, n_lines=160)
    boxes = [[250, 170, 300, 130, 0.9], [620, 150, 10, 170, 0.8], [760, 185, 88, 110, 0.7]]
    return _with_boxes(base, boxes, base["lines"])


def _separate_segments(cx, cy, count):
    """count segments of 36 px around (cx, cy) that merge_break_lines leaves alone: 30 directions 6 degrees apart (it merges below 5), and
    up to three parallel copies per direction 7 px apart sideways (it merges when an end is within 20 px of the other's start: these
    are 36 px away)."""
    segs = []
    for q in range(count):
        a = np.deg2rad(6.0 * (q % 30) - 87.0)
        off = 7.0 * ((q // 30 + 1) // 2) * (1 if (q // 30) % 2 else -1)
        mx, my = cx - np.sin(a) * off, cy + np.cos(a) * off
        segs.append([mx - 18 * np.cos(a), my - 18 * np.sin(a), mx + 18 * np.cos(a), my + 18 * np.sin(a)])      # (x1 < x2: cos > 0 on -87..87)
    return segs


def _frame_masks():
    base = synth.make_frame(9200, n_boxes=1, n_lines=10)
    boxes = [[40 + 235 * i, 170 + 7 * i, 120 + 6 * i, 110 - 4 * i, 0.9] for i in range(5)]
    lines = []
    for b, m in zip(boxes, SEGMENT_COUNTS):
        lines += _separate_segments(b[0] + b[2] / 2, b[1] + b[3] / 2, m)
    return _with_boxes(base, boxes, lines)


@pytest.fixture(scope="module")
def frames():
    return [_frame_trips(), _frame_masks()]


def _params():
    return capi.default_params(whether_sample_cam_roll_pitch=0, yaw_step_deg=YAW_STEP)


def preconditions(frames):
    """What the docstring promises about the two frames, from the oracle alone (no device): yaw and top-edge sample counts, the bounds
    of consecutive boxes, the merged segment counts, and proposals to compare for every box but the 10 px one."""
    trips, masks = frames
    op = oracle_py.default_params(yaw_step_deg=YAW_STEP)
    _, dbg = oracle_py.detect_cuboid(trips, op, atan2_mode=1, debug_cap=20000)
    Y = int(dbg["yaw_count"][0])
    tops = [len(range(int(b[0]) + 5, int(b[0] + b[2]) - 5 + 1, min(20, int(b[2]) // 10))) for b in trips["boxes"]]
    assert tops == [15, 1, 10] and Y * tops[0] > 2048 > Y * tops[0] - 2048 > 0 and Y * tops[2] < 2048, (Y, tops)
    bounds = []
    for b, rr in zip(trips["boxes"], trips["rois"]):
        (l, t, w, h), _ = rr[0]
        bounds.append((int(b[0]), int(b[1]), int(b[0] + b[2]), int(b[1]) + int(b[3]), l, t, l + w, t + h))
    for p, q in zip(bounds, bounds[1:]):
        assert all(x != y for x, y in zip(p, q)), (p, q)
    nv = [int(dbg["n_valid"][3 * i]) for i in range(3)]
    assert nv[0] >= 1 and nv[1] == 0 and nv[2] >= 1, nv
    _, dbg = oracle_py.detect_cuboid(masks, op, atan2_mode=1, debug_cap=20000)
    assert tuple(int(dbg["n_merged_lines"][3 * i]) for i in range(5)) == SEGMENT_COUNTS
    assert all(int(dbg["n_valid"][3 * i]) >= 1 for i in range(5)), dbg["n_valid"][::3]
    return nv


def test_every_candidate_and_kept_set_equals_the_oracle(frames):
    preconditions(frames)
    assert detect_checks._check(frames, _params()) > 100


def test_production_path_records_equal_the_oracle(frames):
    """candidate_compact_kernel and the lean VP support run only here: nothing but the winners' records comes back.  The batch is run
    twice over the same slots (the work list and the counts are rebuilt), and once more with the frames in the other order, so that
    every job has had another job's record in front of it."""
    n, tm = detect_checks._check_final(frames, _params())
    assert n >= 7 and tm["rank_kernel_ms"] > 0
    n, _ = detect_checks._check_final(frames[::-1], _params())
    assert n >= 7
    det = capi.Detector(_params())
    bat = capi.Batch(det, frames)
    bat.run()
    first = bat.raw_out_bytes()
    bat.run()
    assert bat.raw_out_bytes() == first
    bat.close(); det.close()
