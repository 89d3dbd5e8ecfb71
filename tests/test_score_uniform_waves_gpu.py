"""GPU parity of the scorer's distance term by wavefront configuration: score_kernel sums the edge samples through one of three
instances of the same loop -- wavefronts that hold only configuration 1, only configuration 2, or both after the block's counting
sort (detect_kernels.hip: score_edge_sum).  Every candidate row (slot order, configuration, vanishing-point side, yaw and top ids,
distance and angle error), the rebuilt corners, and the kept ids / scores the ranking derives from the distance, angle and skew
columns are compared with the oracle bit for bit, through the C ABI, on the smallest shapes that reach each instance and each
boundary between them.

Which instance a wavefront takes follows from the rows: a workgroup scores 256 consecutive valid rows of one job (capacity layout,
no roll/pitch sampling), sorted by (configuration, top-edge sample), 64 sorted positions per wavefront.  The tests derive the
kinds of wavefront from the oracle's rows and assert that the kinds they are about occurred.
"""
import numpy as np
import pytest
from scipy import ndimage

from cube_slam_wu_amd import capi, synth
from oracle import oracle_py

pytestmark = pytest.mark.gpu


def _oracle_params(p):
    return oracle_py.default_params(
        consider_config_1=p.consider_config_1, consider_config_2=p.consider_config_2,
        whether_sample_cam_roll_pitch=p.whether_sample_cam_roll_pitch, whether_sample_bbox_height=p.whether_sample_bbox_height,
        max_cuboid_num=p.max_cuboid_num, nominal_skew_ratio=p.nominal_skew_ratio, max_cut_skew=p.max_cut_skew,
        yaw_range_deg=p.yaw_range_deg, yaw_step_deg=p.yaw_step_deg)


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return np.array_equal(a, b, equal_nan=True)
    return np.array_equal(a, b)


def wave_kinds(configs):
    """Kinds of the wavefronts that score one job's valid rows (capacity layout): per block of 256 rows, sorted by configuration,
    one entry per 64 sorted positions -- '1' / '2' one configuration, 'M' both; a trailing 'p' marks a partial wavefront."""
    out = []
    for b0 in range(0, len(configs), 256):
        c = np.sort(np.asarray(configs[b0:b0 + 256]).astype(int))
        for w0 in range(0, len(c), 64):
            w = c[w0:w0 + 64]
            out.append(("1" if (w == 1).all() else "2" if (w == 2).all() else "M") + ("p" if len(w) < 64 else ""))
    return out


def _check(frames, params, cap=20000):
    """Rows, corners, kept ids and scores, final records of every box against the oracle; returns per (frame, box) the valid count
    and the wavefront kinds derived from the oracle's rows."""
    det = capi.Detector(params)
    bat = capi.Batch(det, frames, debug=True)
    bat.run()
    info = []
    for f, fr in enumerate(frames):
        ref, dbg = oracle_py.detect_cuboid(fr, _oracle_params(params), atan2_mode=1, debug_cap=cap)
        got = bat.cuboids(f)
        for i in range(len(fr["boxes"])):
            for k in range(len(fr["maps"][i])):
                slot = 3 * i + k
                V = int(dbg["n_valid"][slot])
                assert V <= cap
                rows, corners = bat.debug_candidates(f, i, k)
                assert rows.shape[0] == V, (f, i, k, rows.shape[0], V)
                want = dbg["cand_rows"][slot][:V]
                bad = [c for c in range(want.shape[1]) if not _same(rows[:, c], want[:, c])]
                assert not bad, (f, i, k, "columns", bad)
                assert _same(corners, dbg["cand_corners"][slot][:V]), (f, i, k)
                ids, sc = bat.debug_kept(f, i, k)
                nk = int(dbg["n_keep"][slot])
                assert len(ids) == nk
                assert _same(ids, dbg["keep_ids"][slot][:nk]) and _same(sc, dbg["keep_scores"][slot][:nk]), (f, i, k)
                info.append((V, wave_kinds(want[:, 0])))
            assert len(got[i]) == len(ref[i]), (f, i)
            for a, b in zip(got[i], ref[i]):
                for key in b:
                    assert _same(a[key], b[key]), (f, i, key)
    bat.close()
    det.close()
    return info


def _two_boxes():
    return synth.make_frame(9110, n_boxes=2, n_lines=120)


def test_one_configuration_only():
    """consider_config_1 alone, then consider_config_2 alone: every wavefront is of one configuration, full ones and a partial tail."""
    fr = _two_boxes()
    kinds = [k for _, kk in _check([fr], capi.default_params(whether_sample_cam_roll_pitch=0, consider_config_2=0, yaw_step_deg=1.0)) for k in kk]
    assert set(kinds) <= {"1", "1p"} and "1" in kinds and "1p" in kinds, kinds
    kinds = [k for _, kk in _check([fr], capi.default_params(whether_sample_cam_roll_pitch=0, consider_config_1=0, yaw_step_deg=1.0)) for k in kk]
    assert set(kinds) <= {"2", "2p"} and "2" in kinds and "2p" in kinds, kinds


def test_mixed_wavefronts_and_partial_tails():
    """Both configurations.  The coarse (6 degree) yaw list leaves one job fewer than 64 valid rows -- its single wavefront is mixed and
    partial -- and the other a block whose last, partial wavefront is mixed behind a full one of configuration 1.  At one degree the
    first box has a full block whose wavefronts are of configuration 1, mixed (full) and of configuration 2."""
    fr = _two_boxes()
    info = _check([fr], capi.default_params(whether_sample_cam_roll_pitch=0, yaw_step_deg=6.0))
    assert any(V < 64 and kk == ["Mp"] for V, kk in info), info
    assert any(V > 64 and kk[-1] == "Mp" and "1" in kk for V, kk in info), info
    info = _check([fr], capi.default_params(whether_sample_cam_roll_pitch=0, yaw_step_deg=1.0))
    blocks = [kk[q:q + 4] for _, kk in info for q in range(0, len(kk), 4)]
    assert any(blk == ["1", "1", "1", "1"] for blk in blocks), blocks                     # a block that never leaves the one-configuration path
    assert any({"1", "M", "2"} <= set(blk) for blk in blocks), blocks                     # all three instances within one full block


def test_valid_count_at_a_multiple_of_the_block_and_one_more():
    """The yaw range trimmed until a job's valid count is 4 x 256 (its last block is full) and until it is 256 + 1 (a block of one row)."""
    fr = _two_boxes()
    info = _check([fr], capi.default_params(whether_sample_cam_roll_pitch=0, yaw_step_deg=0.5, yaw_range_deg=39.3))
    assert info[0][0] == 1024, info
    info = _check([fr], capi.default_params(whether_sample_cam_roll_pitch=0, yaw_step_deg=0.5, yaw_range_deg=35.5))
    assert info[1][0] == 257 and info[1][1][-1] in ("1p", "2p"), info


def _moved_to(fr, left, top):
    """The one-box frame with its box (and the segments, by the same offset) moved so that the box starts at (left, top)."""
    fr = dict(fr)
    box = fr["boxes"][0].copy()
    dx, dy = left - box[0], top - box[1]
    box[0], box[1] = left, top
    W, H = fr["img_w"], fr["img_h"]
    lines = np.clip(np.asarray(fr["lines"], np.float64) + [dx, dy, dx, dy], 0, [W - 1, H - 1, W - 1, H - 1])
    rois = synth.box_rois(box, W, H)
    maps = []
    for (l, t, w, h), _ in rois:
        edge = synth._rasterise(lines, l, t, w, h)
        assert edge.any()
        buf = np.zeros(h * w + w + 1, np.float32)
        buf[: h * w] = ndimage.distance_transform_edt(~edge).astype(np.float32).ravel()
        maps.append(buf)
    fr.update(boxes=box[None, :], lines=lines, rois=[rois], maps=[maps])
    return fr


def test_boxes_touching_the_image_border():
    """A box in the image's top-left corner and one in its bottom-right corner: the ROI is clamped to the image, so the end points of the
    edges -- the corners -- lie on the map's first row and column, or on its last."""
    fr = synth.make_frame(9110, n_boxes=1, n_lines=120)
    w, h = fr["boxes"][0][2], fr["boxes"][0][3]
    first = _moved_to(fr, 0.0, 0.0)
    last = _moved_to(fr, fr["img_w"] - 1 - w, fr["img_h"] - 1 - h)
    assert first["rois"][0][0][0][:2] == (0, 0)
    l, t, rw, rh = last["rois"][0][0][0]
    assert l + rw == fr["img_w"] - 1 and t + rh == fr["img_h"] - 1
    info = _check([first, last], capi.default_params(whether_sample_cam_roll_pitch=0, yaw_step_deg=1.0))
    assert all(V > 64 for V, _ in info), info


def test_roll_pitch_sampling_blocks_spanning_jobs():
    """whether_sample_cam_roll_pitch = 1: the scorer's other instantiation (blocks of 256 rows that span jobs)."""
    fr = synth.make_frame(9110, n_boxes=1, n_lines=120)
    info = _check([fr], capi.default_params(whether_sample_cam_roll_pitch=1, yaw_step_deg=3.0))
    assert info[0][0] > 256, info
