"""ctypes view of libcubeslam_hip.so (include/cubeslam_hip.h) for the tests and bench.py.

This is plumbing, not a second implementation: every function here forwards to the C ABI, and
loading fails loudly when the HIP library has not been built (run __graft_entry__.build()).
"""
from __future__ import annotations

import os as _os
# (the library sizes its set of working streams by this value and gives every detector streams of its own for the three roles of a sweep when there are eight
# queues or more -- INTEGRATION.md; only effective when nothing has initialised HIP yet, and a value already in the environment wins)
_os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcubeslam_hip.so")


class CsDetectParams(C.Structure):
    _fields_ = [
        ("consider_config_1", C.c_int), ("consider_config_2", C.c_int),
        ("whether_sample_cam_roll_pitch", C.c_int), ("whether_sample_bbox_height", C.c_int),
        ("max_cuboid_num", C.c_int), ("nominal_skew_ratio", C.c_double), ("max_cut_skew", C.c_double),
        ("yaw_range_deg", C.c_double), ("yaw_step_deg", C.c_double),
        ("vp12_edge_angle_thre", C.c_double), ("vp3_edge_angle_thre", C.c_double), ("shorted_edge_thre", C.c_double),
        ("weight_vp_angle", C.c_double), ("weight_skew_error", C.c_double),
        ("pre_merge_dist_thre", C.c_double), ("pre_merge_angle_thre", C.c_double), ("edge_length_threshold", C.c_double),
        ("host_threads", C.c_int),
    ]


class CsCuboid(C.Structure):
    _fields_ = [
        ("pos", C.c_double * 3), ("scale", C.c_double * 3), ("rotY", C.c_double),
        ("box_config_type", C.c_double * 2), ("box_corners_2d", C.c_int32 * 16),
        ("box_corners_3d_world", C.c_double * 24), ("rect_detect_2d", C.c_double * 4),
        ("edge_distance_error", C.c_double), ("edge_angle_error", C.c_double),
        ("normalized_error", C.c_double), ("skew_ratio", C.c_double), ("down_expand_height", C.c_double),
        ("camera_roll_delta", C.c_double), ("camera_pitch_delta", C.c_double),
    ]


class CsRoi(C.Structure):
    _fields_ = [("left", C.c_int), ("top", C.c_int), ("width", C.c_int), ("height", C.c_int), ("down_expand", C.c_int)]


class CsFrameDesc(C.Structure):
    _fields_ = [
        ("K", C.POINTER(C.c_double)), ("T_wc", C.POINTER(C.c_double)), ("img_w", C.c_int), ("img_h", C.c_int),
        ("boxes", C.POINTER(C.c_double)), ("n_boxes", C.c_int), ("lines", C.POINTER(C.c_double)), ("n_lines", C.c_int),
        ("dist_maps", C.POINTER(C.POINTER(C.c_float))),
    ]


class CsDetectTiming(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("setup_host_ms", "h2d_ms", "vp_kernel_ms", "cand_kernel_ms", "compact_ms", "d2h_ms",
                                          "rank_host_ms", "finalize_ms", "total_ms")] + \
               [("n_jobs", C.c_longlong), ("n_slots", C.c_longlong), ("n_valid", C.c_longlong),
                ("cand_kernel_bytes", C.c_longlong), ("cand_kernel_launches", C.c_int), ("n_fallback_boxes", C.c_int), ("n_redo_frames", C.c_int),
                ("rank_kernel_ms", C.c_double), ("line_setup_ms", C.c_double), ("score_kernel_ms", C.c_double), ("score_kernel_bytes", C.c_longlong)]


# every symbol include/cubeslam_hip.h declares (tests/test_capi_symbols.py checks the export table)
DECLARED_SYMBOLS = [
    "cs_last_error", "cs_device_count", "cs_diag_build", "cs_detect_default_params", "cs_box_rois", "cs_cam_euler_zyx", "cs_detector_create",
    "cs_detector_destroy", "cs_detect_cuboids", "cs_batch_create", "cs_batch_max_boxes", "cs_batch_run", "cs_batch_submit", "cs_batch_collect",
    "cs_bgr_to_gray", "cs_edge_distance_maps", "cs_edge_distance_maps_multi", "cs_detect_cuboids_gray", "cs_batch_create_gray", "cs_batch_refill_gray", "cs_batch_refill_wait", "cs_batch_destroy", "cs_batch_last_timing", "cs_batch_debug_candidates", "cs_batch_debug_kept", "cs_batch_set_debug", "cs_batch_set_pipeline_chunks", "cs_detect_lines_gray", "cs_detect_lines_batch", "cs_detect_lines_last_timing", "cs_detect_lsd_gray", "cs_detect_lsd_batch", "cs_detect_lsd_last_timing",
    "cs_lbd_describe_gray", "cs_detect_descrip_lines_gray", "cs_detect_descrip_lines_batch", "cs_lbd_match", "cs_lbd_match_batch", "cs_lbd_last_timing",
    "cs_check_score_atan2", "cs_check_score_sample_index", "cs_check_line_setup", "cs_check_vp_support",
]

# cs_keyline (one octave: start / end point, direction, length of the support region in pixels)
KEYLINE_DTYPE = np.dtype([("sx", np.float32), ("sy", np.float32), ("ex", np.float32), ("ey", np.float32), ("direction", np.float32), ("num_pixels", np.int32)])

_lib = None


def lib():
    """Load libcubeslam_hip.so; raises if it is missing (no fallback of any kind)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("libcubeslam_hip.so not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        # One HIP runtime per process: the PyTorch wheel ships its own libamdhip64, and whichever copy is loaded
        # first serves both (same SONAME).  Loading ours first leaves torch unable to see the GPU, so when torch is
        # installed it goes first.  (A C++ host, e.g. the reference's ROS nodes, has no torch and no such issue.)
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        L.cs_last_error.restype = C.c_char_p
        _lib = L
    return _lib


def last_error():
    return lib().cs_last_error().decode()


def _default_params(struct_type, symbol, kw, hook=None):
    """A parameter struct as <symbol> fills it, with the overrides `kw`; hook(p, k, v) -> True where it has set field k itself."""
    p = struct_type()
    getattr(lib(), symbol)(C.byref(p))
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(k)
        if hook is None or not hook(p, k, v):
            setattr(p, k, v)
    return p


def _ptr_array(batch, key, n, what):
    """batch[key] as int32, which must hold n + 1 entries (`what` names the n) -> (the array, its last entry = the number of items)."""
    ptr = _i32(batch[key])
    if len(ptr) != n + 1:
        raise ValueError("%s must hold %s + 1 entries" % (key, what))
    return ptr, (int(ptr[-1]) if n else 0)


def default_params(**kw):
    return _default_params(CsDetectParams, "cs_detect_default_params", kw)


def check_score_atan2(y, x):
    """The scorer's atan2 call sequence on the device, one pair per lane: (values, accepted flags of the lean evaluation)."""
    y, x = np.ascontiguousarray(y, np.float64), np.ascontiguousarray(x, np.float64)
    if y.shape != x.shape or y.ndim != 1:
        raise ValueError("y and x must be 1-D arrays of the same length")
    out, acc = np.zeros(len(y)), np.zeros(len(y), np.int32)
    rc = lib().cs_check_score_atan2(_dp(y), _dp(x), len(y), _dp(out), acc.ctypes.data_as(C.POINTER(C.c_int)))
    if rc != 0:
        raise RuntimeError("cs_check_score_atan2 failed (%d): %s" % (rc, last_error()))
    return out, acc.astype(bool)


def check_vp_support(mid_x, mid_y, angle, vp_x, vp_y, thre, swapped=False, form=0):
    """The vanishing-point support of one segment table against the points (vp_x, vp_y): (device, host), each (n, 2) bounding segment angles
    (NaN = no inlier).  form 0 = staged wavefront form on pairs of points, 1 = unstaged on pairs, 2 = unstaged on single points."""
    mid_x, mid_y, angle = (np.ascontiguousarray(a, np.float64) for a in (mid_x, mid_y, angle))
    vp_x, vp_y = np.ascontiguousarray(vp_x, np.float64), np.ascontiguousarray(vp_y, np.float64)
    if not (mid_x.ndim == 1 and mid_x.shape == mid_y.shape == angle.shape) or vp_x.ndim != 1 or vp_x.shape != vp_y.shape:
        raise ValueError("mid_x, mid_y, angle must be 1-D of one length, vp_x and vp_y 1-D of one length")
    n = len(vp_x)
    dev, host = np.zeros((n, 2)), np.zeros((n, 2))
    rc = lib().cs_check_vp_support(_dp(mid_x), _dp(mid_y), _dp(angle), len(mid_x), _dp(vp_x), _dp(vp_y), n, C.c_double(thre), int(bool(swapped)), int(form), _dp(dev), _dp(host))
    if rc != 0:
        raise RuntimeError("cs_check_vp_support failed (%d): %s" % (rc, last_error()))
    return dev, host


def check_score_sample_index(sy, sx, map_w, a, b):
    """The scorer's distance-map index on the device, one sample per lane, and the double-precision sum a + b the same lane forms right
    behind it: (indices, sums)."""
    sy, sx, a, b = (np.ascontiguousarray(t, np.float64) for t in (sy, sx, a, b))
    map_w = np.ascontiguousarray(map_w, np.int32)
    if sy.ndim != 1 or any(t.shape != sy.shape for t in (sx, map_w, a, b)):
        raise ValueError("sy, sx, map_w, a and b must be 1-D arrays of the same length")
    idx, probe = np.zeros(len(sy), np.int32), np.zeros(len(sy))
    ip = C.POINTER(C.c_int)
    rc = lib().cs_check_score_sample_index(_dp(sy), _dp(sx), map_w.ctypes.data_as(ip), _dp(a), _dp(b), len(sy), idx.ctypes.data_as(ip), _dp(probe))
    if rc != 0:
        raise RuntimeError("cs_check_score_sample_index failed (%d): %s" % (rc, last_error()))
    return idx, probe


def check_line_setup(lines, rois, yt, dist_thre=20.0, angle_thre_deg=5.0, len_thre=30.0):
    """The line setup on its own: one frame's segments (n x 4) against r expanded ROIs (r x 4 inclusive integer bounds) with yaw / top-edge
    sample counts yt (r x 2).  Returns (device, host), each a dict of m (r) and angle, mid_x, mid_y (r x n, zero behind the m[k] entries)."""
    lines = np.ascontiguousarray(lines, np.float64).reshape(-1, 4)
    rois, yt = np.ascontiguousarray(rois, np.int32).reshape(-1, 4), np.ascontiguousarray(yt, np.int32).reshape(-1, 2)
    if len(rois) != len(yt):
        raise ValueError("rois and yt must have one row per ROI")
    n, r = len(lines), len(rois)
    ip = C.POINTER(C.c_int)
    m, tab = [np.zeros(r, np.int32) for _ in range(2)], [np.zeros((3, r, n)) for _ in range(2)]
    rc = lib().cs_check_line_setup(_dp(lines), n, rois.ctypes.data_as(ip), yt.ctypes.data_as(ip), r, C.c_double(dist_thre), C.c_double(angle_thre_deg), C.c_double(len_thre),
                                   m[0].ctypes.data_as(ip), _dp(tab[0]), m[1].ctypes.data_as(ip), _dp(tab[1]))
    if rc != 0:
        raise RuntimeError("cs_check_line_setup failed (%d): %s" % (rc, last_error()))
    return tuple({"m": m[q], "angle": tab[q][0], "mid_x": tab[q][1], "mid_y": tab[q][2]} for q in range(2))


def box_rois(box5, img_w, img_h, sample_height=False):
    out = (CsRoi * 3)()
    b = (C.c_double * 5)(*[float(x) for x in box5])
    n = lib().cs_box_rois(b, int(img_w), int(img_h), int(bool(sample_height)), out)
    return [((out[k].left, out[k].top, out[k].width, out[k].height), out[k].down_expand) for k in range(n)]


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def cuboid_to_dict(c):
    return dict(
        pos=np.array(c.pos[:]), scale=np.array(c.scale[:]), rotY=c.rotY, box_config_type=np.array(c.box_config_type[:]),
        box_corners_2d=np.array(c.box_corners_2d[:], dtype=np.int32).reshape(2, 8),
        box_corners_3d_world=np.array(c.box_corners_3d_world[:]).reshape(3, 8),
        rect_detect_2d=np.array(c.rect_detect_2d[:]), edge_distance_error=c.edge_distance_error,
        edge_angle_error=c.edge_angle_error, normalized_error=c.normalized_error, skew_ratio=c.skew_ratio,
        down_expand_height=c.down_expand_height, camera_roll_delta=c.camera_roll_delta, camera_pitch_delta=c.camera_pitch_delta)


class Detector:
    """cs_detector handle."""

    def __init__(self, params=None, device=0):
        self.params = params if params is not None else default_params()
        self.h = C.c_void_p()
        rc = lib().cs_detector_create(C.byref(self.params), int(device), C.byref(self.h))
        if rc != 0:
            raise RuntimeError("cs_detector_create failed (%d): %s" % (rc, last_error()))

    def edge_distance_maps(self, gray, rois):
        """Canny(80, 200) + 3x3 L2 distance transform of each ROI (left, top, width, height) of a uint8 gray image, on the
        device (cs_edge_distance_maps).  Returns one float32 (h, w) array per ROI."""
        gray = np.ascontiguousarray(gray, np.uint8)
        H, W = gray.shape
        n = len(rois)
        rr = (CsRoi * max(1, n))()
        outs, ptrs = [], (C.POINTER(C.c_float) * max(1, n))()
        for k, (l, t, w, h) in enumerate(rois):
            rr[k].left, rr[k].top, rr[k].width, rr[k].height, rr[k].down_expand = int(l), int(t), int(w), int(h), 0
            o = np.zeros((int(h), int(w)), np.float32)
            outs.append(o)
            ptrs[k] = o.ctypes.data_as(C.POINTER(C.c_float))
        rc = lib().cs_edge_distance_maps(self.h, gray.ctypes.data_as(C.POINTER(C.c_ubyte)), W, H, rr, n, ptrs)
        if rc != 0:
            raise RuntimeError("cs_edge_distance_maps failed (%d): %s" % (rc, last_error()))
        return outs

    def edge_distance_maps_time(self, grays, rois, roi_image):
        """Device time (ms) of Canny + distance transform over ROIs of several equally sized images; maps are discarded."""
        grays = [np.ascontiguousarray(g, np.uint8) for g in grays]
        H, W = grays[0].shape
        gp = (C.POINTER(C.c_ubyte) * len(grays))(*[g.ctypes.data_as(C.POINTER(C.c_ubyte)) for g in grays])
        n = len(rois)
        rr = (CsRoi * max(1, n))()
        for k, (l, t, w, h) in enumerate(rois):
            rr[k].left, rr[k].top, rr[k].width, rr[k].height, rr[k].down_expand = int(l), int(t), int(w), int(h), 0
        ri = np.ascontiguousarray(roi_image, np.int32)
        ms = C.c_double()
        rc = lib().cs_edge_distance_maps_multi(self.h, gp, len(grays), W, H, rr, ri.ctypes.data_as(C.POINTER(C.c_int)), n, None, C.byref(ms))
        if rc != 0:
            raise RuntimeError("cs_edge_distance_maps_multi failed (%d): %s" % (rc, last_error()))
        return ms.value

    def detect_lines(self, gray, length_thres=15.0, cap=20000, use_lsd=False):
        """cs_detect_lines_gray / cs_detect_lsd_gray: line_lbd_detect::detect_filter_lines (EDLines, or LSD with the reference's
        use_LSD flag; one octave) -> (n, 4) float32 x1 y1 x2 y2."""
        gray = np.ascontiguousarray(gray, np.uint8)
        out = np.zeros((cap, 4), np.float32)
        n = C.c_int()
        rc = (lib().cs_detect_lsd_gray if use_lsd else lib().cs_detect_lines_gray)(self.h, gray.ctypes.data_as(C.POINTER(C.c_ubyte)), int(gray.shape[1]), int(gray.shape[0]), C.c_double(length_thres),
                                        out.ctypes.data_as(C.POINTER(C.c_float)), int(cap), C.byref(n))
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % ("cs_detect_lsd_gray" if use_lsd else "cs_detect_lines_gray", rc, last_error()))
        return out[:n.value].copy()

    def detect_lines_batch(self, grays, length_thres=15.0, cap=20000, use_lsd=False):
        """cs_detect_lines_batch / cs_detect_lsd_batch: images of one size -> list of (n_i, 4) float32 arrays.
        (The marshalling is kept light -- uninitialised result rows, plain addresses instead of a typed pointer object per image: it was
        3.4 ms per 64-image call, against 5 ms for the library's own work.)"""
        grays = [g if (isinstance(g, np.ndarray) and g.dtype == np.uint8 and g.flags.c_contiguous) else np.ascontiguousarray(g, np.uint8) for g in grays]
        n = len(grays)
        H, W = grays[0].shape
        if any(g.shape != (H, W) for g in grays):
            raise ValueError("detect_lines_batch: the images of a batch have one size")
        out = np.empty((n, cap, 4), np.float32)
        cnt = np.zeros(n, np.int32)
        gp = (C.c_void_p * n)(*[g.ctypes.data for g in grays])
        base, stride = out.ctypes.data, out.strides[0]
        op = (C.c_void_p * n)(*[base + i * stride for i in range(n)])
        rc = (lib().cs_detect_lsd_batch if use_lsd else lib().cs_detect_lines_batch)(self.h, gp, n, int(W), int(H), C.c_double(length_thres), op, int(cap), cnt.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % ("cs_detect_lsd_batch" if use_lsd else "cs_detect_lines_batch", rc, last_error()))
        return [out[i, :cnt[i]].copy() for i in range(n)]

    def describe_lines(self, gray, keylines, want_float=False):
        """cs_lbd_describe_gray: BinaryDescriptor::compute on the caller's keylines (records of KEYLINE_DTYPE, one octave) -> (n, 32) uint8
        [, (n, 72) float32 with want_float]."""
        gray = np.ascontiguousarray(gray, np.uint8)
        kl = np.ascontiguousarray(keylines, KEYLINE_DTYPE)
        n = len(kl)
        d32 = np.zeros((n, 32), np.uint8)
        d72 = np.zeros((n, 72), np.float32) if want_float else None
        rc = lib().cs_lbd_describe_gray(self.h, gray.ctypes.data_as(C.POINTER(C.c_ubyte)), int(gray.shape[1]), int(gray.shape[0]), C.c_void_p(kl.ctypes.data), n,
                                        C.c_void_p(d32.ctypes.data), C.c_void_p(d72.ctypes.data) if want_float else None)
        if rc != 0:
            raise RuntimeError("cs_lbd_describe_gray failed (%d): %s" % (rc, last_error()))
        return (d32, d72) if want_float else d32

    def detect_descrip_lines(self, gray, length_thres=15.0, cap=20000):
        """cs_detect_descrip_lines_gray: line_lbd_detect::detect_descrip_lines (EDLines, one octave) -> (keyline records, (n, 32) uint8)."""
        gray = np.ascontiguousarray(gray, np.uint8)
        kl = np.empty(cap, KEYLINE_DTYPE)
        d32 = np.empty((cap, 32), np.uint8)
        n = C.c_int()
        rc = lib().cs_detect_descrip_lines_gray(self.h, gray.ctypes.data_as(C.POINTER(C.c_ubyte)), int(gray.shape[1]), int(gray.shape[0]), C.c_double(length_thres),
                                                C.c_void_p(kl.ctypes.data), C.c_void_p(d32.ctypes.data), int(cap), C.byref(n))
        if rc != 0:
            raise RuntimeError("cs_detect_descrip_lines_gray failed (%d): %s" % (rc, last_error()))
        return kl[:n.value].copy(), d32[:n.value].copy()

    def detect_descrip_lines_batch(self, grays, length_thres=15.0, cap=20000):
        """cs_detect_descrip_lines_batch: images of one size -> list of (keyline records, (n_i, 32) uint8), all lines described in one launch."""
        grays = [g if (isinstance(g, np.ndarray) and g.dtype == np.uint8 and g.flags.c_contiguous) else np.ascontiguousarray(g, np.uint8) for g in grays]
        n = len(grays)
        if n == 0:
            return []
        H, W = grays[0].shape
        if any(g.shape != (H, W) for g in grays):
            raise ValueError("detect_descrip_lines_batch: the images of a batch have one size")
        kl = np.empty((n, cap), KEYLINE_DTYPE)
        d32 = np.empty((n, cap, 32), np.uint8)
        cnt = np.zeros(n, np.int32)
        gp = (C.c_void_p * n)(*[g.ctypes.data for g in grays])
        kp = (C.c_void_p * n)(*[kl.ctypes.data + i * kl.strides[0] for i in range(n)])
        dp = (C.c_void_p * n)(*[d32.ctypes.data + i * d32.strides[0] for i in range(n)])
        rc = lib().cs_detect_descrip_lines_batch(self.h, gp, n, int(W), int(H), C.c_double(length_thres), kp, dp, int(cap), cnt.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != 0:
            raise RuntimeError("cs_detect_descrip_lines_batch failed (%d): %s" % (rc, last_error()))
        return [(kl[i, :cnt[i]].copy(), d32[i, :cnt[i]].copy()) for i in range(n)]

    def match_lines(self, q, t):
        """cs_lbd_match: BinaryDescriptorMatcher::match on (nq, 32) / (nt, 32) uint8 descriptors -> (train_idx, dist, dist2) int32 per query row
        (nearest train row, ties to the lowest; its Hamming distance; the second-smallest distance; -1 where there is none)."""
        idx, dist, dist2 = self.match_lines_batch([(q, t)])
        return idx[0], dist[0], dist2[0]

    def match_lines_batch(self, pairs):
        """cs_lbd_match_batch: [(q, t), ...] matched in one launch -> (list of train_idx, list of dist, list of dist2), one array per pair."""
        qs = [np.ascontiguousarray(q, np.uint8).reshape(-1, 32) for q, _ in pairs]
        ts = [np.ascontiguousarray(t, np.uint8).reshape(-1, 32) for _, t in pairs]
        q_ptr = np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.int32)
        t_ptr = np.concatenate([[0], np.cumsum([len(t) for t in ts])]).astype(np.int32)
        qa = np.ascontiguousarray(np.concatenate(qs)) if qs else np.zeros((0, 32), np.uint8)
        ta = np.ascontiguousarray(np.concatenate(ts)) if ts else np.zeros((0, 32), np.uint8)
        nq = int(q_ptr[-1])
        out = np.zeros((3, max(nq, 1)), np.int32)
        ip = C.POINTER(C.c_int)
        rc = lib().cs_lbd_match_batch(self.h, len(pairs), C.c_void_p(qa.ctypes.data), q_ptr.ctypes.data_as(ip), C.c_void_p(ta.ctypes.data), t_ptr.ctypes.data_as(ip),
                                      out[0].ctypes.data_as(ip), out[1].ctypes.data_as(ip), out[2].ctypes.data_as(ip))
        if rc != 0:
            raise RuntimeError("cs_lbd_match_batch failed (%d): %s" % (rc, last_error()))
        cut = lambda row: [row[q_ptr[p]:q_ptr[p + 1]].copy() for p in range(len(pairs))]
        return cut(out[0]), cut(out[1]), cut(out[2])

    def match_line_descrip(self, q, t, dist_thres=25.0):
        """line_lbd_detect::match_line_descrip: the matches with dist < dist_thres (matching_dist_thres, 25 by default) as (query_idx, train_idx, dist)
        rows, int32."""
        idx, dist, _ = self.match_lines(q, t)
        keep = np.nonzero((idx >= 0) & (dist < dist_thres))[0]
        return np.stack([keep.astype(np.int32), idx[keep], dist[keep]], axis=1).astype(np.int32).reshape(-1, 3)

    def lbd_timing(self):
        """Device time (ms) of the last descriptor kernel and the last matching kernel of this detector (-1: not run)."""
        a, b = C.c_double(), C.c_double()
        rc = lib().cs_lbd_last_timing(self.h, C.byref(a), C.byref(b))
        if rc != 0:
            raise RuntimeError("cs_lbd_last_timing failed (%d)" % rc)
        return {"describe_kernel_ms": a.value, "match_kernel_ms": b.value}

    def lines_timing(self, use_lsd=False):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        rc = (lib().cs_detect_lsd_last_timing if use_lsd else lib().cs_detect_lines_last_timing)(self.h, C.byref(a), C.byref(b), C.byref(c))
        if rc != 0:
            raise RuntimeError("cs_detect_lines_last_timing failed (%d)" % rc)
        return {"device_ms": a.value, "host_ms": b.value, "total_ms": c.value}

    def frame_call(self, frame, gray=None):
        """A reusable zero-argument callable for cs_detect_cuboids (or cs_detect_cuboids_gray when `gray` is given) on one frame: the
        ctypes descriptor is built once, so repeated calls time the library, not the marshalling.  call() -> list of lists of dicts."""
        K = np.ascontiguousarray(frame["K"], np.float64).reshape(9)
        T = np.ascontiguousarray(frame["T_wc"], np.float64).reshape(16)
        boxes = np.ascontiguousarray(frame["boxes"], np.float64).reshape(-1, 5)
        lines = np.ascontiguousarray(frame["lines"], np.float64).reshape(-1, 4)
        nb = boxes.shape[0]
        arr = (C.POINTER(C.c_float) * max(1, 3 * nb))()
        keep = [K, T, boxes, lines]
        if gray is None:
            for i in range(nb):
                for k, m in enumerate(frame["maps"][i]):
                    m = np.ascontiguousarray(m, np.float32); keep.append(m)
                    arr[3 * i + k] = m.ctypes.data_as(C.POINTER(C.c_float))
        else:
            gray = np.ascontiguousarray(gray, np.uint8); keep.append(gray)
        d = CsFrameDesc()
        d.K, d.T_wc, d.img_w, d.img_h = _dp(K), _dp(T), int(frame["img_w"]), int(frame["img_h"])
        d.boxes, d.n_boxes, d.lines, d.n_lines, d.dist_maps = _dp(boxes), nb, _dp(lines), lines.shape[0], arr
        kmax = self.params.max_cuboid_num
        out = (CsCuboid * max(1, nb * kmax))()
        counts = np.zeros(max(1, nb), np.int32)
        cp = counts.ctypes.data_as(C.POINTER(C.c_int))
        L, h = lib(), self.h
        gp = gray.ctypes.data_as(C.POINTER(C.c_ubyte)) if gray is not None else None

        def call(parse=False):
            rc = L.cs_detect_cuboids(h, C.byref(d), out, cp) if gp is None else L.cs_detect_cuboids_gray(h, C.byref(d), gp, out, cp)
            if rc != 0:
                raise RuntimeError("cs_detect_cuboids failed (%d): %s" % (rc, last_error()))
            if parse:
                return [[cuboid_to_dict(out[i * kmax + k]) for k in range(int(counts[i]))] for i in range(nb)]
        call._keep = keep
        return call

    def detect_gray(self, frame, gray):
        """cs_detect_cuboids_gray: image in, cuboids out (the frame's 'maps' are not used)."""
        gray = np.ascontiguousarray(gray, np.uint8)
        K = np.ascontiguousarray(frame["K"], np.float64).reshape(9)
        T = np.ascontiguousarray(frame["T_wc"], np.float64).reshape(16)
        boxes = np.ascontiguousarray(frame["boxes"], np.float64).reshape(-1, 5)
        lines = np.ascontiguousarray(frame["lines"], np.float64).reshape(-1, 4)
        d = CsFrameDesc()
        d.K, d.T_wc, d.img_w, d.img_h = _dp(K), _dp(T), int(frame["img_w"]), int(frame["img_h"])
        d.boxes, d.n_boxes, d.lines, d.n_lines, d.dist_maps = _dp(boxes), boxes.shape[0], _dp(lines), lines.shape[0], None
        kmax = self.params.max_cuboid_num
        out = (CsCuboid * max(1, boxes.shape[0] * kmax))()
        counts = np.zeros(max(1, boxes.shape[0]), np.int32)
        rc = lib().cs_detect_cuboids_gray(self.h, C.byref(d), gray.ctypes.data_as(C.POINTER(C.c_ubyte)), out, counts.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != 0:
            raise RuntimeError("cs_detect_cuboids_gray failed (%d): %s" % (rc, last_error()))
        return [[cuboid_to_dict(out[i * kmax + k]) for k in range(int(counts[i]))] for i in range(boxes.shape[0])]

    def close(self):
        if self.h:
            lib().cs_detector_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """cs_batch handle over a list of frame dicts (cube_slam_wu_amd.synth.make_frame layout)."""

    def __init__(self, det: Detector, frames, debug=False, force_host_rank=False, force_host_setup=False, force_no_pipeline=False, pipeline_chunks=1, grays=None):
        self.det = det
        self.n_frames = len(frames)
        self._keep = []
        descs = (CsFrameDesc * max(1, self.n_frames))()
        for f, fr in enumerate(frames):
            K = np.ascontiguousarray(fr["K"], np.float64).reshape(9)
            T = np.ascontiguousarray(fr["T_wc"], np.float64).reshape(16)
            boxes = np.ascontiguousarray(fr["boxes"], np.float64).reshape(-1, 5)
            lines = np.ascontiguousarray(fr["lines"], np.float64).reshape(-1, 4)
            n = boxes.shape[0]
            arr = (C.POINTER(C.c_float) * max(1, 3 * n))()
            for i in range(n if grays is None else 0):
                for k, m in enumerate(fr["maps"][i]):
                    m = np.ascontiguousarray(m, np.float32)
                    self._keep.append(m)
                    arr[3 * i + k] = m.ctypes.data_as(C.POINTER(C.c_float))
            self._keep += [K, T, boxes, lines, arr]
            d = descs[f]
            d.K, d.T_wc, d.img_w, d.img_h = _dp(K), _dp(T), int(fr["img_w"]), int(fr["img_h"])
            d.boxes, d.n_boxes, d.lines, d.n_lines, d.dist_maps = _dp(boxes), n, _dp(lines), lines.shape[0], arr
        self.h = C.c_void_p()
        if grays is None:
            rc = lib().cs_batch_create(det.h, descs, self.n_frames, C.byref(self.h))
        else:   # image input: the maps are produced on the device from the gray images
            gs = [np.ascontiguousarray(g, np.uint8) for g in grays]
            self._gray_px = int(gs[0].size) if gs else 0
            gp = (C.POINTER(C.c_ubyte) * max(1, len(gs)))(*[g.ctypes.data_as(C.POINTER(C.c_ubyte)) for g in gs])
            rc = lib().cs_batch_create_gray(det.h, descs, gp, self.n_frames, C.byref(self.h))
        if rc != 0:
            raise RuntimeError("cs_batch_create failed (%d): %s" % (rc, last_error()))
        self._keep = []  # inputs were copied by the library
        self.max_boxes = lib().cs_batch_max_boxes(self.h)
        self.kmax = det.params.max_cuboid_num
        self._out = (CsCuboid * max(1, self.n_frames * max(1, self.max_boxes) * self.kmax))()
        self._counts = np.zeros(max(1, self.n_frames * max(1, self.max_boxes)), np.int32)
        if debug or force_host_rank or force_host_setup or force_no_pipeline:
            lib().cs_batch_set_debug(self.h, (1 if debug else 0) | (2 if force_host_rank else 0) | (4 if force_host_setup else 0) | (8 if force_no_pipeline else 0))

        if pipeline_chunks != 1:
            if lib().cs_batch_set_pipeline_chunks(self.h, int(pipeline_chunks)) != 0:
                raise RuntimeError("cs_batch_set_pipeline_chunks failed")

    def refill_gray(self, grays=None, base_ptr=None):
        """cs_batch_refill_gray: new gray images for the same frames (asynchronous).  grays: a list of uint8 arrays, or base_ptr: the address of
        n_frames images contiguous in (ideally pinned) host memory."""
        px = None
        if base_ptr is not None:
            t = lib().cs_batch_max_boxes(self.h)      # (any call: keeps the handle checked)
            px = self._gray_px
            ptrs = (C.POINTER(C.c_ubyte) * self.n_frames)(*[C.cast(base_ptr + f * px, C.POINTER(C.c_ubyte)) for f in range(self.n_frames)])
        else:
            self._refill_keep = [np.ascontiguousarray(g, np.uint8) for g in grays]
            ptrs = (C.POINTER(C.c_ubyte) * self.n_frames)(*[g.ctypes.data_as(C.POINTER(C.c_ubyte)) for g in self._refill_keep])
        rc = lib().cs_batch_refill_gray(self.det.h, self.h, ptrs)
        if rc != 0:
            raise RuntimeError("cs_batch_refill_gray failed (%d): %s" % (rc, last_error()))

    def refill_wait(self):
        rc = lib().cs_batch_refill_wait(self.h)
        if rc != 0:
            raise RuntimeError("cs_batch_refill_wait failed (%d): %s" % (rc, last_error()))

    def run(self):
        rc = lib().cs_batch_run(self.det.h, self.h, self._out, self._counts.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != 0:
            raise RuntimeError("cs_batch_run failed (%d): %s" % (rc, last_error()))

    def submit(self):
        """First half of run(): pack + queue the sweep, do not wait (cs_batch_submit)."""
        rc = lib().cs_batch_submit(self.det.h, self.h, self._out, self._counts.ctypes.data_as(C.POINTER(C.c_int)))
        if rc != 0:
            raise RuntimeError("cs_batch_submit failed (%d): %s" % (rc, last_error()))

    def collect(self):
        """Second half of run(): wait for the sweep, write the records (cs_batch_collect)."""
        rc = lib().cs_batch_collect(self.det.h, self.h)
        if rc != 0:
            raise RuntimeError("cs_batch_collect failed (%d): %s" % (rc, last_error()))

    def cuboids(self, frame):
        res = []
        for i in range(self.max_boxes):
            cnt = int(self._counts[frame * self.max_boxes + i])
            res.append([cuboid_to_dict(self._out[(frame * self.max_boxes + i) * self.kmax + k]) for k in range(cnt)])
        return res

    def raw_out_bytes(self):
        return bytes(self._out)

    def counts_bytes(self):
        return self._counts.tobytes()

    def timing(self):
        t = CsDetectTiming()
        rc = lib().cs_batch_last_timing(self.h, C.byref(t))
        if rc != 0:
            raise RuntimeError("cs_batch_last_timing failed (%d)" % rc)
        return {n: getattr(t, n) for n, _ in CsDetectTiming._fields_}

    def debug_candidates(self, frame, box, k=0, with_corners=True):
        L = lib()
        n = L.cs_batch_debug_candidates(self.h, frame, box, k, 0, None, None)
        if n < 0:
            raise RuntimeError("cs_batch_debug_candidates failed (%d): %s" % (n, last_error()))
        rows = np.zeros((n, 9))
        corners = np.zeros((n, 16))
        if n:
            rc = L.cs_batch_debug_candidates(self.h, frame, box, k, n, _dp(rows), _dp(corners) if with_corners else None)
            if rc < 0:
                raise RuntimeError("cs_batch_debug_candidates failed (%d): %s" % (rc, last_error()))
        return rows, corners

    def debug_kept(self, frame, box, k=0):
        L = lib()
        n = L.cs_batch_debug_kept(self.h, frame, box, k, 0, None, None)
        if n < 0:
            raise RuntimeError("cs_batch_debug_kept failed (%d)" % n)
        ids = np.zeros(n, np.int32)
        sc = np.zeros(n)
        if n:
            L.cs_batch_debug_kept(self.h, frame, box, k, n, ids.ctypes.data_as(C.POINTER(C.c_int)), _dp(sc))
        return ids, sc

    def close(self):
        if self.h:
            lib().cs_batch_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------ Path B: bundle adjustment ----------
class CsBaTiming(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("errors_ms", "linearize_ms", "reduce_ms", "schur_ms", "factor_ms", "backsub_ms", "update_ms", "total_ms")] + \
               [("n_linearizations", C.c_longlong), ("n_solves", C.c_longlong), ("linearize_bytes", C.c_longlong), ("schur_entries", C.c_longlong), ("structure_ms", C.c_double)]


class CsBaClassify(C.Structure):
    _fields_ = [("chi2_mono", C.c_double), ("chi2_stereo", C.c_double), ("depth_positive", C.c_int), ("sticky", C.c_int)]


class CsBaRound(C.Structure):
    _fields_ = [("iterations", C.c_int), ("kernels_enabled", C.c_int), ("classify", CsBaClassify)]


DECLARED_SYMBOLS += [
    "cs_ba_create", "cs_ba_destroy", "cs_ba_set_vertices", "cs_ba_set_estimates", "cs_ba_set_edges_proj", "cs_ba_set_edges_cuboid", "cs_ba_set_edges_cuboid_proj", "cs_ba_set_edges_odom",
    "cs_ba_compute_errors", "cs_ba_build_system", "cs_ba_solve", "cs_ba_update", "cs_ba_push", "cs_ba_pop", "cs_ba_optimize",
    "cs_ba_get_state", "cs_ba_sizes", "cs_ba_solver_layout", "cs_ba_get_system", "cs_ba_last_timing", "cs_ba_set_shard", "cs_ba_optimize_sharded",
    "cs_ba_shard_landmark_owners", "cs_ba_get_landmark_owners", "cs_ba_shard_info", "cs_ba_shard_timing", "cs_ba_append_vertices", "cs_ba_append_edges_proj", "cs_ba_append_edges_cuboid", "cs_ba_append_edges_cuboid_proj", "cs_ba_append_edges_odom", "cs_ba_get_vertex_hessians", "cs_ba_schur_layout", "cs_ba_structure_digest", "cs_ba_reduced_size", "cs_ba_solver_path", "cs_ba_band_order", "cs_ba_comm_unique_id", "cs_ba_comm_init", "cs_ba_set_robust_kernels",
    "cs_ba_set_external_edges", "cs_ba_set_external_terms", "cs_ba_set_external_chi2", "cs_ba_set_external_callback", "cs_ba_check_finite", "cs_ba_dump", "cs_ba_load", "cs_ba_get_reduced_system", "cs_ba_set_stage_timing", "cs_ba_set_lm_params", "cs_ba_pose_marginals",
    "cs_ba_set_edges_proj_stereo", "cs_ba_append_edges_proj_stereo",
    "cs_ba_set_edge_levels", "cs_ba_get_edge_levels", "cs_ba_set_kernels_enabled", "cs_ba_classify_edges", "cs_ba_optimize_rounds",
]


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int)) if a is not None else None


def _f64(a, shape):
    return np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape))


def _i32(a):
    return np.ascontiguousarray(np.asarray(a, np.int32).ravel())


def _chk(rc, what):
    if rc != 0:
        raise RuntimeError("%s failed (%d): %s" % (what, rc, last_error()))


class BaProblem:
    """cs_ba handle; the method names mirror the g2o calls each one replaces."""

    def __init__(self, cams, cam_fixed, cuboids=None, cub_fixed=None, points=None, pt_fixed=None, cuboids_first=False, device=0):
        L = lib()
        self.h = C.c_void_p()
        _chk(L.cs_ba_create(int(device), C.byref(self.h)), "cs_ba_create")
        cams = _f64(cams, (-1, 7)); self.nc = len(cams)
        cub = _f64(cuboids if cuboids is not None else np.zeros((0, 10)), (-1, 10)); self.no = len(cub)
        pts = _f64(points if points is not None else np.zeros((0, 3)), (-1, 3)); self.np_ = len(pts)
        cf = _i32(cam_fixed); of = _i32(cub_fixed if cub_fixed is not None else np.zeros(self.no)); pf = _i32(pt_fixed if pt_fixed is not None else np.zeros(self.np_))
        _chk(L.cs_ba_set_vertices(self.h, _dp(cams), _ip(cf), self.nc, _dp(cub), _ip(of), self.no, _dp(pts), _ip(pf), self.np_, int(cuboids_first)), "cs_ba_set_vertices")
        self.n_proj = self.n_cub = self.n_odom = 0

    def set_edges_proj(self, pt, cam, uv, info4, intr4, huber=None):
        pt, cam = _i32(pt), _i32(cam); self.n_proj = len(pt)
        hb = _f64(huber, (-1,)) if huber is not None else None
        _chk(lib().cs_ba_set_edges_proj(self.h, self.n_proj, _ip(pt), _ip(cam), _dp(_f64(uv, (-1, 2))), _dp(_f64(info4, (-1, 4))), _dp(_f64(intr4, (-1, 4))),
                                        _dp(hb) if hb is not None else None), "cs_ba_set_edges_proj")

    def set_edges_proj_stereo(self, pt, cam, uvr3, info9, intr5, huber=None):
        """EdgeStereoSE3ProjectXYZ: uvr3 = (u_left, v, u_right), info9 row-major 3 x 3, intr5 = fx fy cx cy bf; they follow the mono edges in g2o's order."""
        pt, cam = _i32(pt), _i32(cam); self.n_stereo = len(pt)
        hb = _f64(huber, (-1,)) if huber is not None else None
        _chk(lib().cs_ba_set_edges_proj_stereo(self.h, self.n_stereo, _ip(pt), _ip(cam), _dp(_f64(uvr3, (-1, 3))), _dp(_f64(info9, (-1, 9))), _dp(_f64(intr5, (-1, 5))),
                                               _dp(hb) if hb is not None else None), "cs_ba_set_edges_proj_stereo")

    def set_edges_cuboid(self, cam, cub, meas10, info81):
        cam, cub = _i32(cam), _i32(cub); self.n_cub = len(cam)
        _chk(lib().cs_ba_set_edges_cuboid(self.h, self.n_cub, _ip(cam), _ip(cub), _dp(_f64(meas10, (-1, 10))), _dp(_f64(info81, (-1, 81)))), "cs_ba_set_edges_cuboid")

    def set_edges_cuboid_proj(self, cam, cub, meas4, info16, K9):
        """EdgeSE3CuboidProj: bounding-box (cx, cy, w, h) error of the projected cuboid."""
        cam, cub = _i32(cam), _i32(cub); self.n_cproj = len(cam)
        _chk(lib().cs_ba_set_edges_cuboid_proj(self.h, self.n_cproj, _ip(cam), _ip(cub), _dp(_f64(meas4, (-1, 4))), _dp(_f64(info16, (-1, 16))), _dp(_f64(K9, (-1, 9)))),
             "cs_ba_set_edges_cuboid_proj")

    def set_edges_odom(self, ci, cj, meas7, info36):
        ci, cj = _i32(ci), _i32(cj); self.n_odom = len(ci)
        _chk(lib().cs_ba_set_edges_odom(self.h, self.n_odom, _ip(ci), _ip(cj), _dp(_f64(meas7, (-1, 7))), _dp(_f64(info36, (-1, 36)))), "cs_ba_set_edges_odom")

    def set_robust_kernels(self, edge_class, kind, delta):
        """cs_ba_set_robust_kernels: edge_class 0 projection / 1 EdgeSE3Cuboid / 2 EdgeSE3CuboidProj / 3 EdgeSE3Expmap; kind per edge
        (RK_* below), delta = RobustKernel::delta(); 4 = the stereo projection edges.  kind None removes the class's kernels."""
        if kind is None:        # (the library counts the class's edges itself: no shadow count here, a handle from Problem.load() has none)
            _chk(lib().cs_ba_set_robust_kernels(self.h, int(edge_class), 0, None, None), "cs_ba_set_robust_kernels")
            return
        kind, delta = _i32(kind), _f64(delta, (-1,))
        _chk(lib().cs_ba_set_robust_kernels(self.h, int(edge_class), len(kind), _ip(kind), _dp(delta)), "cs_ba_set_robust_kernels")

    # ---- edge levels, kernels switched in place, classification, rounds (ORB-SLAM2's LocalBundleAdjustment on the device)
    def _class_count(self, edge_class):
        return {EDGE_PROJ: self.n_proj, EDGE_PROJ_STEREO: getattr(self, "n_stereo", 0), EDGE_CUBOID: self.n_cub, EDGE_CUBOID_PROJ: getattr(self, "n_cproj", 0),
                EDGE_ODOM: self.n_odom}[int(edge_class)]

    def set_edge_levels(self, edge_class, level, n=None):
        """Edge::setLevel over a class (cs_ba_set_edge_levels): level[k] in {0, 1} in the caller's edge order, None = all 0; n (default: the
        class's count as this wrapper has seen it) must equal the library's count."""
        lv = np.ascontiguousarray(np.asarray(level, np.uint8).ravel()) if level is not None else None
        n = int(n) if n is not None else (len(lv) if lv is not None else self._class_count(edge_class))
        _chk(lib().cs_ba_set_edge_levels(self.h, int(edge_class), n, lv.ctypes.data_as(C.POINTER(C.c_ubyte)) if lv is not None else None), "cs_ba_set_edge_levels")

    def edge_levels(self, edge_class, n=None):
        """The class's levels in the caller's edge order (cs_ba_get_edge_levels)."""
        n = int(n) if n is not None else self._class_count(edge_class)
        out = np.zeros(max(1, n), np.uint8)
        _chk(lib().cs_ba_get_edge_levels(self.h, int(edge_class), n, out.ctypes.data_as(C.POINTER(C.c_ubyte))), "cs_ba_get_edge_levels")
        return out[:n]

    def set_kernels_enabled(self, edge_class, enabled):
        """setRobustKernel(0) over a class, and back, without forgetting the deltas or touching the structure (cs_ba_set_kernels_enabled)."""
        _chk(lib().cs_ba_set_kernels_enabled(self.h, int(edge_class), 1 if enabled else 0), "cs_ba_set_kernels_enabled")

    def classify_edges(self, chi2_mono=5.991, chi2_stereo=7.815, depth_positive=True, sticky=False, want_chi2=False):
        """cs_ba_classify_edges at the current estimates -> (n_outliers mono, stereo) [, chi2 mono, chi2 stereo in the caller's order]."""
        p = CsBaClassify(float(chi2_mono), float(chi2_stereo), 1 if depth_positive else 0, 1 if sticky else 0)
        cnt = (C.c_int * 2)()
        cm = np.zeros(max(1, self.n_proj)) if want_chi2 else None
        cs_ = np.zeros(max(1, getattr(self, "n_stereo", 0))) if want_chi2 else None
        _chk(lib().cs_ba_classify_edges(self.h, C.byref(p), cnt, _dp(cm) if want_chi2 else None, _dp(cs_) if want_chi2 else None), "cs_ba_classify_edges")
        n = (int(cnt[0]), int(cnt[1]))
        return (n, cm[:self.n_proj], cs_[:getattr(self, "n_stereo", 0)]) if want_chi2 else n

    def optimize_rounds(self, rounds, cap=64):
        """cs_ba_optimize_rounds: rounds = [(iterations, kernels_enabled, (chi2_mono, chi2_stereo, depth_positive, sticky) or None), ...];
        -> (iterations done per round, n_outliers (n_rounds, 2)); rounds_history() has the per-round chi2 / lambda / trials."""
        nr = len(rounds)
        arr = (CsBaRound * max(1, nr))()
        for r, (its, ke, cl) in enumerate(rounds):
            cl = cl if cl is not None else (0.0, 0.0, 0, 0)
            arr[r] = CsBaRound(int(its), 1 if ke else 0, CsBaClassify(float(cl[0]), float(cl[1]), int(cl[2]), int(cl[3])))
        done, nout = np.zeros(max(1, nr), np.int32), np.zeros((max(1, nr), 2), np.int32)
        self._rchi, self._rlam, self._rtr = np.zeros((max(1, nr), cap)), np.zeros((max(1, nr), cap)), np.zeros((max(1, nr), cap), np.int32)
        _chk(lib().cs_ba_optimize_rounds(self.h, arr, nr, _ip(done), _ip(nout), _dp(self._rchi), _dp(self._rlam), _ip(self._rtr), int(cap)), "cs_ba_optimize_rounds")
        self._rdone = done[:nr].copy()
        return self._rdone, nout[:nr].copy()

    def rounds_history(self):
        """[(chi2, lambda, trials) of round r] after optimize_rounds."""
        return [(self._rchi[r, :n].copy(), self._rlam[r, :n].copy(), self._rtr[r, :n].copy()) for r, n in enumerate(self._rdone)]

    # ---- external (host-evaluated) edges
    def set_external_edges(self, class_i, idx_i, class_j, idx_j):
        ci, ii, cj, ij = _i32(class_i), _i32(idx_i), _i32(class_j), _i32(idx_j)
        self.n_ext = len(ci)
        _chk(lib().cs_ba_set_external_edges(self.h, len(ci), _ip(ci), _ip(ii), _ip(cj), _ip(ij)), "cs_ba_set_external_edges")

    def set_external_terms(self, cam36=None, cam6=None, cub81=None, cub9=None, pt9=None, pt3=None, Hij81=None, chi2=0.0):
        a = [(_f64(x, (-1,)) if x is not None else None) for x in (cam36, cam6, cub81, cub9, pt9, pt3, Hij81)]
        _chk(lib().cs_ba_set_external_terms(self.h, *[(_dp(x) if x is not None else None) for x in a], C.c_double(chi2)), "cs_ba_set_external_terms")

    def set_external_chi2(self, chi2):
        _chk(lib().cs_ba_set_external_chi2(self.h, C.c_double(chi2)), "cs_ba_set_external_chi2")

    def set_external_callback(self, fn):
        """fn(want_system) -> None: re-evaluates the external edges at self.state() (see cs_ba_set_external_callback)."""
        CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int)

        def _cb(ctx, ba, want_system):
            try:
                fn(int(want_system))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1
        self._ext_cb = CB(_cb) if fn is not None else None
        _chk(lib().cs_ba_set_external_callback(self.h, self._ext_cb, None), "cs_ba_set_external_callback")

    # ---- growing graphs: new vertices / edges behind the existing ones, device-side estimates kept
    def append_vertices(self, cams=None, cam_fixed=None, cuboids=None, cub_fixed=None, points=None, pt_fixed=None):
        c = _f64(cams if cams is not None else np.zeros((0, 7)), (-1, 7)); o = _f64(cuboids if cuboids is not None else np.zeros((0, 10)), (-1, 10))
        q = _f64(points if points is not None else np.zeros((0, 3)), (-1, 3))
        cf = _i32(cam_fixed if cam_fixed is not None else np.zeros(len(c))); of = _i32(cub_fixed if cub_fixed is not None else np.zeros(len(o))); pf = _i32(pt_fixed if pt_fixed is not None else np.zeros(len(q)))
        _chk(lib().cs_ba_append_vertices(self.h, _dp(c), _ip(cf), len(c), _dp(o), _ip(of), len(o), _dp(q), _ip(pf), len(q)), "cs_ba_append_vertices")
        self.nc += len(c); self.no += len(o); self.np_ += len(q)

    def append_edges_proj(self, pt, cam, uv, info4, intr4, huber=None):
        pt, cam = _i32(pt), _i32(cam)
        hb = _f64(huber, (-1,)) if huber is not None else None
        _chk(lib().cs_ba_append_edges_proj(self.h, len(pt), _ip(pt), _ip(cam), _dp(_f64(uv, (-1, 2))), _dp(_f64(info4, (-1, 4))), _dp(_f64(intr4, (-1, 4))), _dp(hb) if hb is not None else None), "cs_ba_append_edges_proj")
        self.n_proj = getattr(self, "n_proj", 0) + len(pt)

    def append_edges_proj_stereo(self, pt, cam, uvr3, info9, intr5, huber=None):
        pt, cam = _i32(pt), _i32(cam)
        hb = _f64(huber, (-1,)) if huber is not None else None
        _chk(lib().cs_ba_append_edges_proj_stereo(self.h, len(pt), _ip(pt), _ip(cam), _dp(_f64(uvr3, (-1, 3))), _dp(_f64(info9, (-1, 9))), _dp(_f64(intr5, (-1, 5))),
                                                  _dp(hb) if hb is not None else None), "cs_ba_append_edges_proj_stereo")
        self.n_stereo = getattr(self, "n_stereo", 0) + len(pt)

    def append_edges_cuboid(self, cam, cub, meas10, info81):
        cam, cub = _i32(cam), _i32(cub)
        _chk(lib().cs_ba_append_edges_cuboid(self.h, len(cam), _ip(cam), _ip(cub), _dp(_f64(meas10, (-1, 10))), _dp(_f64(info81, (-1, 81)))), "cs_ba_append_edges_cuboid")
        self.n_cub = getattr(self, "n_cub", 0) + len(cam)

    def append_edges_cuboid_proj(self, cam, cub, meas4, info16, K9):
        cam, cub = _i32(cam), _i32(cub)
        _chk(lib().cs_ba_append_edges_cuboid_proj(self.h, len(cam), _ip(cam), _ip(cub), _dp(_f64(meas4, (-1, 4))), _dp(_f64(info16, (-1, 16))), _dp(_f64(K9, (-1, 9)))),
             "cs_ba_append_edges_cuboid_proj")
        self.n_cproj = getattr(self, "n_cproj", 0) + len(cam)

    def append_edges_odom(self, ci, cj, meas7, info36):
        ci, cj = _i32(ci), _i32(cj)
        _chk(lib().cs_ba_append_edges_odom(self.h, len(ci), _ip(ci), _ip(cj), _dp(_f64(meas7, (-1, 7))), _dp(_f64(info36, (-1, 36)))), "cs_ba_append_edges_odom")
        self.n_odom = getattr(self, "n_odom", 0) + len(ci)

    def compute_errors(self):
        chi = C.c_double()
        _chk(lib().cs_ba_compute_errors(self.h, C.byref(chi)), "cs_ba_compute_errors")
        return chi.value

    def sizes(self):
        a, b = C.c_int(), C.c_int()
        _chk(lib().cs_ba_sizes(self.h, C.byref(a), C.byref(b)), "cs_ba_sizes")
        return a.value, b.value

    def build_system(self, dense_hpp=True):
        _chk(lib().cs_ba_build_system(self.h), "cs_ba_build_system")
        n, nl = self.sizes()
        Hpp, Hll, Hpl, b = (np.zeros((n, n)) if dense_hpp else None), np.zeros((nl // 3, 9)), np.zeros((self.n_proj + getattr(self, "n_stereo", 0), 18)), np.zeros(n + nl)
        _chk(lib().cs_ba_get_system(self.h, _dp(Hpp) if dense_hpp else None, _dp(Hll), _dp(Hpl), _dp(b), None), "cs_ba_get_system")
        return Hpp, Hll, Hpl, b

    def pose_marginals(self, pairs):
        """cs_ba_pose_marginals (Solver::computeMarginals): pairs = [((class_i, idx_i), (class_j, idx_j)), ...] with class 0 = camera (6), 1 = cuboid (9);
        -> (list of d_i x d_j blocks of inv(H_pp), positive_definite)."""
        n = len(pairs)
        ci = np.array([p[0][0] for p in pairs], np.int32); ii = np.array([p[0][1] for p in pairs], np.int32)
        cj = np.array([p[1][0] for p in pairs], np.int32); ij = np.array([p[1][1] for p in pairs], np.int32)
        dims = [({0: 6, 1: 9}.get(int(a), 3), {0: 6, 1: 9}.get(int(b), 3)) for a, b in zip(ci, cj)]      # (a point: the library refuses it)
        out = np.zeros(max(1, sum(a * b for a, b in dims)))
        pd = C.c_int(1)
        _chk(lib().cs_ba_pose_marginals(self.h, n, _ip(ci), _ip(ii), _ip(cj), _ip(ij), _dp(out), C.byref(pd)), "cs_ba_pose_marginals")
        blocks, o = [], 0
        for a, b in dims:
            blocks.append(out[o:o + a * b].reshape(a, b).copy()); o += a * b
        return blocks, bool(pd.value)

    def reduced_system(self, lam):
        """(S dense n_red x n_red, rhs, camera columns, cuboid columns) in solver order -- cs_ba_get_reduced_system."""
        n = self.reduced_size()[0]
        S, rhs, cc, oc = np.zeros((n, n)), np.zeros(n), np.zeros(max(1, self.nc), np.int32), np.zeros(max(1, self.no), np.int32)
        _chk(lib().cs_ba_get_reduced_system(self.h, C.c_double(lam), _dp(S), _dp(rhs), _ip(cc), _ip(oc)), "cs_ba_get_reduced_system")
        return S, rhs, cc[:self.nc], oc[:self.no]

    def vertex_hessians(self):
        """A_ii of every vertex (what g2o maps into BaseVertex::_hessian): (nc, 6, 6), (no, 9, 9), (np, 3, 3)."""
        hc, ho, hp = np.zeros((self.nc, 36)), np.zeros((self.no, 81)), np.zeros((self.np_, 9))
        _chk(lib().cs_ba_get_vertex_hessians(self.h, _dp(hc), _dp(ho), _dp(hp)), "cs_ba_get_vertex_hessians")
        return hc.reshape(-1, 6, 6), ho.reshape(-1, 9, 9), hp.reshape(-1, 3, 3)

    def set_estimates(self, cams=None, cuboids=None, points=None):
        """New estimates for the same graph (after a g2o-side update()/pop()): no structure rebuild."""
        c = _f64(cams, (-1, 7)) if cams is not None else None
        o = _f64(cuboids, (-1, 10)) if cuboids is not None else None
        q = _f64(points, (-1, 3)) if points is not None else None
        _chk(lib().cs_ba_set_estimates(self.h, _dp(c) if c is not None else None, _dp(o) if o is not None else None, _dp(q) if q is not None else None), "cs_ba_set_estimates")

    def update(self):
        _chk(lib().cs_ba_update(self.h), "cs_ba_update")

    def push(self):
        _chk(lib().cs_ba_push(self.h), "cs_ba_push")

    def pop(self):
        _chk(lib().cs_ba_pop(self.h), "cs_ba_pop")

    def system_vectors(self):
        """(b, x) of the last build / solve in g2o's order [poses..., landmarks...] (Solver::b(), Solver::x())."""
        n, nl = self.sizes()
        b, x = np.zeros(n + nl), np.zeros(n + nl)
        _chk(lib().cs_ba_get_system(self.h, None, None, None, _dp(b), _dp(x)), "cs_ba_get_system")
        return b, x

    def reduced_size(self):
        """(unknowns of the factorised system, cuboids eliminated?) -- cs_ba_reduced_size."""
        a, b = C.c_int(), C.c_int()
        _chk(lib().cs_ba_reduced_size(self.h, C.byref(a), C.byref(b)), "cs_ba_reduced_size")
        return a.value, bool(b.value)

    def band_order(self):
        """(block cyclic reduction?, levels) of a banded reduced system -- cs_ba_band_order."""
        a, b = C.c_int(0), C.c_int(0)
        _chk(lib().cs_ba_band_order(self.h, C.byref(a), C.byref(b)), "cs_ba_band_order")
        return bool(a.value), b.value

    def solver_path(self, detail=False):
        """'band' / 'sparse' / 'dense': the factorisation the reduced system takes (cs_ba_solver_path); detail: (path, bandwidth, sparse fill)."""
        a, b, f = C.c_int(), C.c_int(), C.c_double()
        _chk(lib().cs_ba_solver_path(self.h, C.byref(a), C.byref(b), C.byref(f)), "cs_ba_solver_path")
        name = {0: "dense", 1: "band", 2: "sparse"}[a.value]
        return (name, b.value, f.value) if detail else name

    def structure_digest(self):
        """One 64-bit hash per index table of the structure phase (cs_ba_structure_digest)."""
        n = C.c_int(0)
        _chk(lib().cs_ba_structure_digest(self.h, None, 0, C.byref(n)), "cs_ba_structure_digest")
        out = (C.c_ulonglong * n.value)()
        _chk(lib().cs_ba_structure_digest(self.h, out, n.value, C.byref(n)), "cs_ba_structure_digest")
        return [int(v) for v in out]

    def schur_layout(self):
        """(fused, segments, partial blocks, destination blocks) of the Schur-complement build (cs_ba_schur_layout)."""
        a, b, c, d = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _chk(lib().cs_ba_schur_layout(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)), "cs_ba_schur_layout")
        return bool(a.value), b.value, c.value, d.value

    def solver_layout(self):
        a, b = C.c_int(), C.c_int()
        _chk(lib().cs_ba_solver_layout(self.h, C.byref(a), C.byref(b)), "cs_ba_solver_layout")
        return a.value, b.value

    def solve(self, lam):
        pd = C.c_int()
        _chk(lib().cs_ba_solve(self.h, C.c_double(lam), C.byref(pd)), "cs_ba_solve")
        n, nl = self.sizes()
        x = np.zeros(n + nl)
        if pd.value:
            _chk(lib().cs_ba_get_system(self.h, None, None, None, None, _dp(x)), "cs_ba_get_system")
        return bool(pd.value), x

    def optimize(self, iters, cap=64):
        done = C.c_int()
        self._chi, self._lam, self._tr = np.zeros(cap), np.zeros(cap), np.zeros(cap, np.int32)
        _chk(lib().cs_ba_optimize(self.h, int(iters), C.byref(done), _dp(self._chi), _dp(self._lam), _ip(self._tr), cap), "cs_ba_optimize")
        self._done = done.value
        return done.value

    def history(self):
        n = self._done
        return self._chi[:n], self._lam[:n], self._tr[:n]

    # ---- sharded BA -------------------------------------------------------------------------------
    def set_shard(self, rank, n_ranks):
        _chk(lib().cs_ba_set_shard(self.h, int(rank), int(n_ranks)), "cs_ba_set_shard")
        self.shard = (int(rank), int(n_ranks))

    def comm_init(self, rank, n_ranks, unique_id):
        """RCCL communicator for the sharded BA (cs_ba_comm_init): unique_id = the 128 bytes rank 0 got from comm_unique_id()."""
        buf = (C.c_ubyte * 128).from_buffer_copy(bytes(unique_id))
        _chk(lib().cs_ba_comm_init(self.h, int(rank), int(n_ranks), buf), "cs_ba_comm_init")
        self.shard = (int(rank), int(n_ranks))

    def landmark_owners(self):
        """Rank owning each landmark under the rule in force for this handle (cs_ba_get_landmark_owners)."""
        out = np.zeros(max(1, self.np_), np.int32)
        _chk(lib().cs_ba_get_landmark_owners(self.h, _ip(out)), "cs_ba_get_landmark_owners")
        return out[:self.np_]

    def shard_info(self):
        """dict(sep_mode, n_sep, w_max, bytes_per_trial, bytes_per_trial_allreduce, interior_n) -- cs_ba_shard_info."""
        a, b, c, f = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        d, e = C.c_longlong(), C.c_longlong()
        _chk(lib().cs_ba_shard_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(e), C.byref(f)), "cs_ba_shard_info")
        return dict(sep_mode=a.value, n_sep=b.value, w_max=c.value, bytes_per_trial=d.value, bytes_per_trial_allreduce=e.value, interior_n=f.value)

    def shard_timing(self):
        """Accumulated ms of the separator-mode solve stages (cs_ba_shard_timing)."""
        out = (C.c_double * 5)()
        _chk(lib().cs_ba_shard_timing(self.h, out), "cs_ba_shard_timing")
        return dict(zip(("interior_factor_ms", "separator_message_ms", "gather_ms", "separator_solve_ms", "interior_backsolve_ms"), list(out)))

    def optimize_sharded(self, iters, allreduce=None, cap=64):
        """allreduce(ptr, n_doubles, on_device, op) -> 0: in-place all-reduce (op 0 = SUM, 1 = MAX) of n doubles; None = the
        library's own RCCL communicator (comm_init)."""
        if allreduce is None:
            done = C.c_int()
            self._chi, self._lam, self._tr = np.zeros(cap), np.zeros(cap), np.zeros(cap, np.int32)
            _chk(lib().cs_ba_optimize_sharded(self.h, int(iters), None, None, C.byref(done), _dp(self._chi), _dp(self._lam), _ip(self._tr), cap), "cs_ba_optimize_sharded")
            self._done = done.value
            return done.value
        CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_int)

        def _cb(ctx, data, n, on_device, op):
            try:
                return int(allreduce(data, int(n), int(on_device), int(op)) or 0)
            except Exception as e:  # never let an exception cross the C boundary
                import traceback
                traceback.print_exc()
                return 1
        cb = CB(_cb)
        done = C.c_int()
        self._chi, self._lam, self._tr = np.zeros(cap), np.zeros(cap), np.zeros(cap, np.int32)
        _chk(lib().cs_ba_optimize_sharded(self.h, int(iters), cb, None, C.byref(done), _dp(self._chi), _dp(self._lam), _ip(self._tr), cap), "cs_ba_optimize_sharded")
        self._done = done.value
        return done.value

    def check_finite(self):
        """(number of non-finite values, report) -- cs_ba_check_finite."""
        n, buf = C.c_int(), C.create_string_buffer(4096)
        _chk(lib().cs_ba_check_finite(self.h, C.byref(n), buf, 4096), "cs_ba_check_finite")
        return n.value, buf.value.decode()

    def dump(self, path):
        _chk(lib().cs_ba_dump(self.h, str(path).encode()), "cs_ba_dump")

    @classmethod
    def load(cls, path, sizes, device=0):
        """cs_ba_load; sizes = (n_cams, n_cuboids, n_points, n_proj) of the dumped problem, n_proj counting mono and stereo projection edges (the Python wrapper sizes its host arrays with them)."""
        P = cls.__new__(cls)
        P.h = C.c_void_p()
        _chk(lib().cs_ba_load(str(path).encode(), int(device), C.byref(P.h)), "cs_ba_load")
        P.nc, P.no, P.np_, P.n_proj = [int(x) for x in sizes]
        P.n_cub = P.n_odom = 0
        return P

    def state(self):
        cams, cubs, pts = np.zeros((self.nc, 7)), np.zeros((self.no, 10)), np.zeros((self.np_, 3))
        _chk(lib().cs_ba_get_state(self.h, _dp(cams), _dp(cubs), _dp(pts)), "cs_ba_get_state")
        return cams, cubs, pts

    def stage_timing(self, on=True):
        """g2o's setComputeBatchStatistics: turn the per-stage split of timing() on (off by default: its phase marks cost ~6 us each on the stream)."""
        _chk(lib().cs_ba_set_stage_timing(self.h, 1 if on else 0), "cs_ba_set_stage_timing")
        return self

    def set_lm_params(self, user_lambda_init=0.0, max_trials_after_failure=10):
        """OptimizationAlgorithmLevenberg::setUserLambdaInit / setMaxTrialsAfterFailure (optimization_algorithm_levenberg.cpp:191-199)."""
        lib().cs_ba_set_lm_params.argtypes = [C.c_void_p, C.c_double, C.c_int]
        _chk(lib().cs_ba_set_lm_params(self.h, float(user_lambda_init), int(max_trials_after_failure)), "cs_ba_set_lm_params")
        return self

    def timing(self):
        t = CsBaTiming()
        _chk(lib().cs_ba_last_timing(self.h, C.byref(t)), "cs_ba_last_timing")
        return {n: getattr(t, n) for n, _ in CsBaTiming._fields_}

    def close(self):
        if self.h:
            lib().cs_ba_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


RK_NONE, RK_HUBER, RK_PSEUDO_HUBER, RK_CAUCHY, RK_SATURATED, RK_DCS, RK_TUKEY = range(7)      # enum cs_robust_kernel
EDGE_PROJ, EDGE_CUBOID, EDGE_CUBOID_PROJ, EDGE_ODOM, EDGE_PROJ_STEREO = range(5)               # enum cs_edge_class


def ba_from_dict(pr, device=0, cuboids_first=False):
    """BaProblem from a cube_slam_wu_amd.synth_ba.make_problem() dict."""
    P = BaProblem(pr["cams"], pr["cam_fixed"], pr["cuboids"], pr["cub_fixed"], pr["points"], pr["pt_fixed"], cuboids_first=cuboids_first, device=device)
    if len(pr["e_pt"]):
        P.set_edges_proj(pr["e_pt"], pr["e_cam"], pr["e_uv"], pr["e_info"], pr["e_intr"], pr["e_huber"])
    if len(pr.get("se_pt", [])):          # (synth_ba.make_stereo_problem)
        P.set_edges_proj_stereo(pr["se_pt"], pr["se_cam"], pr["se_uvr"], pr["se_info"], pr["se_intr"], pr["se_huber"])
    if len(pr["ce_cam"]):
        P.set_edges_cuboid(pr["ce_cam"], pr["ce_cub"], pr["ce_meas"], pr["ce_info"])
    if len(pr.get("pe_cam", [])):
        P.set_edges_cuboid_proj(pr["pe_cam"], pr["pe_cub"], pr["pe_meas"], pr["pe_info"], pr["pe_K"])
    if len(pr["oe_i"]):
        P.set_edges_odom(pr["oe_i"], pr["oe_j"], pr["oe_meas"], pr["oe_info"])
    for cls, (kind, delta) in pr.get("robust", {}).items():       # optional: {edge class: (kinds, deltas)}
        P.set_robust_kernels(cls, kind, delta)
    return P


def comm_unique_id():
    """128-byte RCCL unique id (ncclGetUniqueId); call on rank 0 and broadcast."""
    buf = (C.c_ubyte * 128)()
    _chk(lib().cs_ba_comm_unique_id(buf), "cs_ba_comm_unique_id")
    return bytes(buf)


def landmark_owners(n_ranks, n_cams, n_points, e_pt, e_cam):
    """Host-only: rank owning each landmark in the sharded BA (cs_ba_shard_landmark_owners)."""
    e_pt, e_cam = _i32(e_pt), _i32(e_cam)
    out = np.zeros(int(n_points), np.int32)
    _chk(lib().cs_ba_shard_landmark_owners(int(n_ranks), int(n_cams), int(n_points), len(e_pt), _ip(e_pt), _ip(e_cam), _ip(out)), "cs_ba_shard_landmark_owners")
    return out


class DeviceDoubles:
    """__cuda_array_interface__ view of n doubles at a raw device pointer (for torch.as_tensor(..., device='cuda'))."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "<f8", "data": (int(ptr), False), "version": 2}


def torch_allreduce(dist, device):
    """all-reduce callback for BaProblem.optimize_sharded backed by torch.distributed (NCCL = RCCL on ROCm)."""
    import torch

    def fn(ptr, n, on_device, op):
        rop = dist.ReduceOp.SUM if op == 0 else dist.ReduceOp.MAX
        if on_device:
            t = torch.as_tensor(DeviceDoubles(ptr, n), device=device)
            if dist.get_backend() == "gloo":      # CPU collective: stage through the host
                h = t.cpu()
                dist.all_reduce(h, op=rop)
                t.copy_(h)
            else:
                dist.all_reduce(t, op=rop)
            torch.cuda.synchronize(device)
        else:
            a = np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_double)), shape=(n,))
            t = torch.from_numpy(a)
            if dist.get_backend() == "gloo":
                dist.all_reduce(t, op=rop)
            else:
                d = t.to(device)
                dist.all_reduce(d, op=rop)
                t.copy_(d.cpu())
        return 0
    return fn


def cam_rank(cam, n_cams, n_ranks):
    """Rank owning a camera in the sharded BA: contiguous subsequences [r*Nc/R, (r+1)*Nc/R) (ba_host.cpp cam_rank)."""
    return (np.asarray(cam, np.int64) * int(n_ranks)) // max(1, int(n_cams))


def shard_frames(n_frames, rank, world):
    """Path A multi-GPU: frames are independent units, dealt round-robin; returns this rank's frame indices."""
    return list(range(int(rank), int(n_frames), int(world)))


# ------------------------------------------------------------------ motion-only pose optimisation, batched ----------
class CsPoseParams(C.Structure):
    _fields_ = [("n_rounds", C.c_int), ("iterations", C.c_int * 8), ("robust_rounds", C.c_int), ("restart_each_round", C.c_int),
                ("huber_mono", C.c_double), ("huber_stereo", C.c_double), ("chi2_mono", C.c_double), ("chi2_stereo", C.c_double)]


DECLARED_SYMBOLS += ["cs_pose_default_params", "cs_pose_optimize_batch", "cs_pose_batch_create", "cs_pose_batch_destroy", "cs_pose_batch_optimize", "cs_pose_batch_last_timing",
                     "cs_pose_linearize_batch"]


def pose_default_params(**kw):
    """cs_pose_default_params with overrides; `iterations` takes a list of n_rounds counts."""
    def iterations(p, k, v):
        if k == "iterations":
            for r, n in enumerate(v):
                p.iterations[r] = int(n)
        return k == "iterations"
    return _default_params(CsPoseParams, "cs_pose_default_params", kw, iterations)


def _pose_inputs(batch):
    """A batch dict (synth_pose.synth_pose_batch layout: Tcw, intr, obs_ptr, Xw, meas, info, is_stereo) as C arguments."""
    T = _f64(batch["Tcw"], (-1, 7)); n = len(T)
    intr, (ptr, N) = _f64(batch["intr"], (n, 5)), _ptr_array(batch, "obs_ptr", n, "n_frames")
    X, m, W = _f64(batch["Xw"], (N, 3)), _f64(batch["meas"], (N, 3)), _f64(batch["info"], (N, 9))
    st = np.ascontiguousarray(np.asarray(batch["is_stereo"]).ravel().astype(np.uint8))
    if len(st) != N:
        raise ValueError("is_stereo must hold one entry per observation")
    keep = (T, intr, ptr, X, m, W, st)
    return n, N, keep, (n, _dp(T), _dp(intr), _ip(ptr), _dp(X), _dp(m), _dp(W), st.ctypes.data_as(C.POINTER(C.c_ubyte)))


def _pose_call(fn, head, batch, params):
    """Marshals a batch dict into one optimize call."""
    p = params if params is not None else pose_default_params()
    n, N, keep, args = _pose_inputs(batch)
    T_out, inl = np.zeros((n, 7)), np.zeros(N, np.uint8)
    chi2, iters = np.zeros((n, p.n_rounds)), np.zeros((n, p.n_rounds), np.int32)
    rc = fn(*head, C.byref(p), *args, _dp(T_out), inl.ctypes.data_as(C.POINTER(C.c_ubyte)), _dp(chi2), _ip(iters))
    return rc, dict(Tcw=T_out, inlier=inl, chi2=chi2, iterations=iters)


class _BatchHandle:
    """What the batch handles share: <_SYM>_create, _last_timing and _destroy of a handle that keeps its stream and device buffers between calls."""
    _SYM = None

    def __init__(self, device=0):
        self.h = C.c_void_p()
        _chk(getattr(lib(), self._SYM + "_create")(int(device), C.byref(self.h)), self._SYM + "_create")

    def timing(self):
        k, h = C.c_double(), C.c_double()
        _chk(getattr(lib(), self._SYM + "_last_timing")(self.h, C.byref(k), C.byref(h)), self._SYM + "_last_timing")
        return {"kernel_ms": k.value, "host_ms": h.value}

    def close(self):
        if self.h:
            getattr(lib(), self._SYM + "_destroy")(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class PoseBatch(_BatchHandle):
    """cs_pose_batch handle: keeps its stream and device buffers between optimize() calls."""

    _SYM = "cs_pose_batch"

    def optimize(self, batch, params=None):
        """-> dict: Tcw (n, 7), inlier (N, uint8), chi2 and iterations (n, n_rounds)."""
        rc, out = _pose_call(lib().cs_pose_batch_optimize, (self.h,), batch, params)
        _chk(rc, "cs_pose_batch_optimize")
        return out


def pose_optimize_batch(batch, params=None, device=0):
    """cs_pose_optimize_batch: the one-shot form."""
    rc, out = _pose_call(lib().cs_pose_optimize_batch, (int(device),), batch, params)
    _chk(rc, "cs_pose_optimize_batch")
    return out


def pose_linearize_batch(batch, robust=True, huber_mono=None, huber_stereo=None, device=0):
    """cs_pose_linearize_batch -> (H (n, 21): the upper entries row by row, b (n, 6), chi2 (n)) at batch["Tcw"] over all observations;
    the Huber widths default to cs_pose_default_params'."""
    d = pose_default_params()
    hm, hs = (d.huber_mono if huber_mono is None else huber_mono), (d.huber_stereo if huber_stereo is None else huber_stereo)
    n, N, keep, args = _pose_inputs(batch)
    H, b, chi2 = np.zeros((n, 21)), np.zeros((n, 6)), np.zeros(n)
    _chk(lib().cs_pose_linearize_batch(int(device), int(bool(robust)), C.c_double(hm), C.c_double(hs), *args, _dp(H), _dp(b), _dp(chi2)), "cs_pose_linearize_batch")
    return H, b, chi2


# ------------------------------------------------------------------ Sim(3) alignment of keyframe pairs, batched ----------
class CsSim3PairParams(C.Structure):
    _fields_ = [("iterations_first", C.c_int), ("iterations_more_clean", C.c_int), ("iterations_more_outliers", C.c_int), ("robust_second_round", C.c_int),
                ("min_inliers", C.c_int), ("th2", C.c_double), ("huber_delta", C.c_double)]


DECLARED_SYMBOLS += ["cs_sim3_pair_default_params", "cs_sim3_optimize_pairs", "cs_sim3_pairs_create", "cs_sim3_pairs_destroy", "cs_sim3_pairs_optimize",
                     "cs_sim3_pairs_last_timing", "cs_sim3_pairs_linearize"]


def sim3_pair_default_params(**kw):
    """cs_sim3_pair_default_params with overrides."""
    return _default_params(CsSim3PairParams, "cs_sim3_pair_default_params", kw)


def _sim3_pair_inputs(batch):
    """A batch dict (synth_sim3_pairs.synth_sim3_pairs layout: S12, intr, fix_scale, match_ptr, P1, P2, obs1, obs2, info12, info21) as C arguments."""
    S = _f64(batch["S12"], (-1, 8)); n = len(S)
    intr, (ptr, N) = _f64(batch["intr"], (n, 8)), _ptr_array(batch, "match_ptr", n, "n_pairs")
    fs = np.ascontiguousarray(np.asarray(batch["fix_scale"]).ravel().astype(np.uint8))
    if len(fs) != n:
        raise ValueError("fix_scale must hold one entry per pair")
    P1, P2, o1, o2 = _f64(batch["P1"], (N, 3)), _f64(batch["P2"], (N, 3)), _f64(batch["obs1"], (N, 2)), _f64(batch["obs2"], (N, 2))
    W12 = _f64(batch["info12"], (N, 4)) if batch.get("info12") is not None else None
    W21 = _f64(batch["info21"], (N, 4)) if batch.get("info21") is not None else None
    keep = (S, intr, ptr, fs, P1, P2, o1, o2, W12, W21)
    return n, N, keep, (_dp(S), _dp(intr), _u8p(fs), _ip(ptr), _dp(P1), _dp(P2), _dp(o1), _dp(o2))


def _sim3_pair_call(fn, head, batch, params):
    p = params if params is not None else sim3_pair_default_params()
    n, N, keep, args = _sim3_pair_inputs(batch)
    W12, W21 = keep[8], keep[9]
    S_out, inl, n_in = np.zeros((n, 8)), np.zeros(N, np.uint8), np.zeros(n, np.int32)
    chi2, iters = np.zeros((n, 2)), np.zeros((n, 2), np.int32)
    rc = fn(*head, C.byref(p), n, *args, _dp(W12) if W12 is not None else None, _dp(W21) if W21 is not None else None,
            _dp(S_out), _u8p(inl), _ip(n_in), _dp(chi2), _ip(iters))
    return rc, dict(S12=S_out, inlier=inl, n_inliers=n_in, chi2=chi2, iterations=iters)


class Sim3Pairs(_BatchHandle):
    """cs_sim3_pairs handle: keeps its stream and device buffers between optimize() calls."""

    _SYM = "cs_sim3_pairs"

    def optimize(self, batch, params=None):
        """-> dict: S12 (n, 8), inlier (N, uint8), n_inliers (n), chi2 and iterations (n, 2)."""
        rc, out = _sim3_pair_call(lib().cs_sim3_pairs_optimize, (self.h,), batch, params)
        _chk(rc, "cs_sim3_pairs_optimize")
        return out


def sim3_optimize_pairs(batch, params=None, device=0):
    """cs_sim3_optimize_pairs: the one-shot form."""
    rc, out = _sim3_pair_call(lib().cs_sim3_optimize_pairs, (int(device),), batch, params)
    _chk(rc, "cs_sim3_optimize_pairs")
    return out


def sim3_pairs_linearize(batch, device=0):
    """cs_sim3_pairs_linearize -> (err (N, 4): e12 e21, jac (N, 2, 2, 7): edge, error component, update dimension) at batch["S12"]."""
    n, N, keep, args = _sim3_pair_inputs(batch)
    err, jac = np.zeros((N, 4)), np.zeros((N, 2, 2, 7))
    _chk(lib().cs_sim3_pairs_linearize(int(device), n, *args, _dp(err), _dp(jac)), "cs_sim3_pairs_linearize")
    return err, jac


# ------------------------------------------------------------------ Sim(3) RANSAC of keyframe pairs, batched ----------
class CsSim3RansacParams(C.Structure):
    _fields_ = [("probability", C.c_double), ("min_inliers", C.c_int), ("max_iterations", C.c_int)]


DECLARED_SYMBOLS += ["cs_sim3_ransac_default_params", "cs_sim3_ransac_pairs", "cs_sim3_ransac_create", "cs_sim3_ransac_destroy", "cs_sim3_ransac_run",
                     "cs_sim3_ransac_last_timing", "cs_sim3_ransac_triplets", "cs_sim3_ransac_hypotheses"]


def sim3_ransac_default_params(**kw):
    """cs_sim3_ransac_default_params with overrides."""
    return _default_params(CsSim3RansacParams, "cs_sim3_ransac_default_params", kw)


def _sim3_ransac_inputs(batch):
    """A batch dict (synth_sim3_ransac layout: intr, fix_scale, seed, match_ptr, P1, P2, max_err1, max_err2) as C arguments."""
    intr = _f64(batch["intr"], (-1, 8)); n = len(intr)
    ptr, N = _ptr_array(batch, "match_ptr", n, "n_pairs")
    fs = np.ascontiguousarray(np.asarray(batch["fix_scale"]).ravel().astype(np.uint8))
    seed = np.ascontiguousarray(np.asarray(batch["seed"]).ravel().astype(np.uint64))
    if len(fs) != n or len(seed) != n:
        raise ValueError("fix_scale and seed must hold one entry per pair")
    P1, P2, t1, t2 = _f64(batch["P1"], (N, 3)), _f64(batch["P2"], (N, 3)), _f64(batch["max_err1"], (N,)), _f64(batch["max_err2"], (N,))
    keep = (intr, fs, seed, ptr, P1, P2, t1, t2)
    return n, N, keep, (_dp(intr), _u8p(fs), seed.ctypes.data_as(C.POINTER(C.c_ulonglong)), _ip(ptr), _dp(P1), _dp(P2), _dp(t1), _dp(t2))


def _sim3_ransac_call(fn, head, batch, params):
    p = params if params is not None else sim3_ransac_default_params()
    n, N, keep, args = _sim3_ransac_inputs(batch)
    found, hyp, its, n_in = (np.zeros(n, np.int32) for _ in range(4))
    S_out, inl = np.zeros((n, 8)), np.zeros(N, np.uint8)
    rc = fn(*head, C.byref(p), n, *args, _ip(found), _ip(hyp), _ip(its), _dp(S_out), _u8p(inl), _ip(n_in))
    return rc, dict(found=found, hyp=hyp, iterations=its, S12=S_out, inlier=inl, n_inliers=n_in)


class Sim3Ransac(_BatchHandle):
    """cs_sim3_ransac handle: keeps its stream and device buffers between run() calls."""

    _SYM = "cs_sim3_ransac"

    def run(self, batch, params=None):
        """-> dict: found, hyp, iterations, n_inliers (n), S12 (n, 8), inlier (N, uint8)."""
        rc, out = _sim3_ransac_call(lib().cs_sim3_ransac_run, (self.h,), batch, params)
        _chk(rc, "cs_sim3_ransac_run")
        return out


def sim3_ransac_pairs(batch, params=None, device=0):
    """cs_sim3_ransac_pairs: the one-shot form."""
    rc, out = _sim3_ransac_call(lib().cs_sim3_ransac_pairs, (int(device),), batch, params)
    _chk(rc, "cs_sim3_ransac_pairs")
    return out


def sim3_ransac_triplets(seed, n_matches, n_hyp):
    """cs_sim3_ransac_triplets -> (n_hyp, 3) match indices; runs without a device."""
    out = np.zeros((int(n_hyp), 3), np.int32)
    _chk(lib().cs_sim3_ransac_triplets(C.c_ulonglong(int(seed)), int(n_matches), int(n_hyp), _ip(out)), "cs_sim3_ransac_triplets")
    return out


def sim3_ransac_hypotheses(batch, n_hyp, device=0):
    """cs_sim3_ransac_hypotheses -> (S12 (n, n_hyp, 8), count (n, n_hyp)): every hypothesis of every pair; a refused one has count -1."""
    n, N, keep, args = _sim3_ransac_inputs(batch)
    S, cnt = np.zeros((n, int(n_hyp), 8)), np.zeros((n, int(n_hyp)), np.int32)
    _chk(lib().cs_sim3_ransac_hypotheses(int(device), n, *args, int(n_hyp), _dp(S), _ip(cnt)), "cs_sim3_ransac_hypotheses")
    return S, cnt


# ------------------------------------------------------------------ two-view triangulation of new map points, batched ----------
class CsTriangulateParams(C.Structure):
    _fields_ = [("min_baseline_ratio", C.c_double), ("max_cos_parallax", C.c_double), ("chi2_mono", C.c_double), ("chi2_stereo", C.c_double),
                ("ratio_factor", C.c_double), ("scale_range", C.c_double)]


DECLARED_SYMBOLS += ["cs_triangulate_default_params", "cs_triangulate_pairs", "cs_triangulate_create", "cs_triangulate_destroy", "cs_triangulate_run",
                     "cs_triangulate_last_timing", "cs_triangulate_inspect"]

# cs_triangulate_status / cs_triangulate_route
TRI_STATUS = {"OK": 0, "PAIR_NOT_RUN": 1, "LOW_PARALLAX": 2, "W_ZERO": 3, "DEPTH1": 4, "DEPTH2": 5, "REPROJ1": 6, "REPROJ2": 7, "ZERO_DIST": 8, "SCALE": 9}
TRI_ROUTE = {"NONE": 0, "TRIANGULATED": 1, "STEREO1": 2, "STEREO2": 3}


def triangulate_default_params(**kw):
    """cs_triangulate_default_params with overrides."""
    return _default_params(CsTriangulateParams, "cs_triangulate_default_params", kw)


def _triangulate_inputs(batch):
    """A batch dict (synth_triangulate layout: Tcw1, Tcw2, cam1, cam2, median_depth2, match_ptr, kp1, kp2) as C arguments."""
    T1 = _f64(batch["Tcw1"], (-1, 7)); n = len(T1)
    T2, c1, c2, md = _f64(batch["Tcw2"], (n, 7)), _f64(batch["cam1"], (n, 6)), _f64(batch["cam2"], (n, 6)), _f64(batch["median_depth2"], (n,))
    ptr, N = _ptr_array(batch, "match_ptr", n, "n_pairs")
    k1, k2 = _f64(batch["kp1"], (N, 6)), _f64(batch["kp2"], (N, 6))
    keep = (T1, T2, c1, c2, md, ptr, k1, k2)
    return n, N, keep, (_dp(T1), _dp(T2), _dp(c1), _dp(c2), _dp(md), _ip(ptr), _dp(k1), _dp(k2))


def _triangulate_call(fn, head, batch, params, inspect=False):
    p = params if params is not None else triangulate_default_params()
    n, N, keep, args = _triangulate_inputs(batch)
    X, nrm, dmin, dmax = np.zeros((N, 3)), np.zeros((N, 3)), np.zeros(N), np.zeros(N)
    status, route, ran, n_acc = np.zeros(N, np.uint8), np.zeros(N, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.int32)
    out = dict(X=X, normal=nrm, min_distance=dmin, max_distance=dmax, status=status, route=route, ran=ran, n_accepted=n_acc)
    tail = ()
    if inspect:
        out["cos3"] = np.zeros((N, 3))
        tail = (_dp(out["cos3"]),)
    rc = fn(*head, C.byref(p), n, *args, _dp(X), _dp(nrm), _dp(dmin), _dp(dmax), _u8p(status), _u8p(route), _u8p(ran), _ip(n_acc), *tail)
    return rc, out


class Triangulate(_BatchHandle):
    """cs_triangulate handle: keeps its stream and device buffers between run() calls."""

    _SYM = "cs_triangulate"

    def run(self, batch, params=None):
        """-> dict: X, normal (N, 3), min_distance, max_distance (N), status, route (N, uint8), ran (n, uint8), n_accepted (n)."""
        rc, out = _triangulate_call(lib().cs_triangulate_run, (self.h,), batch, params)
        _chk(rc, "cs_triangulate_run")
        return out


def triangulate_pairs(batch, params=None, device=0):
    """cs_triangulate_pairs: the one-shot form."""
    rc, out = _triangulate_call(lib().cs_triangulate_pairs, (int(device),), batch, params)
    _chk(rc, "cs_triangulate_pairs")
    return out


def triangulate_inspect(batch, params=None, device=0):
    """cs_triangulate_inspect: triangulate_pairs' outputs plus cos3 (N, 3) = cosRays, cosS1, cosS2 of every match."""
    rc, out = _triangulate_call(lib().cs_triangulate_inspect, (int(device),), batch, params, inspect=True)
    _chk(rc, "cs_triangulate_inspect")
    return out


# ------------------------------------------------------------------ guided ORB matching by projection, batched -----------------
class CsOrbSearchParams(C.Structure):
    _fields_ = [("min_dist_factor", C.c_double), ("max_dist_factor", C.c_double), ("view_cos", C.c_double), ("chi2_mono", C.c_double), ("chi2_stereo", C.c_double),
                ("grid_cols", C.c_int), ("grid_rows", C.c_int)]


DECLARED_SYMBOLS += ["cs_orb_search_default_params", "cs_orb_search_create", "cs_orb_search_destroy", "cs_orb_search_set_frames", "cs_orb_search_run",
                     "cs_orb_search_last_timing", "cs_orb_search_jobs", "cs_orb_search_inspect", "cs_orb_search_mutual"]

# cs_orb_search_status / cs_orb_search_flags
ORB_STATUS = {"OK": 0, "SKIPPED": 1, "BEHIND": 2, "OUT_OF_IMAGE": 3, "OUT_OF_RANGE": 4, "VIEW_ANGLE": 5, "NO_CANDIDATE": 6, "TOO_FAR": 7}
ORB_FLAGS = {"CHECK_VIEW": 1, "CHECK_REPROJ": 2}


def orb_search_default_params(**kw):
    """cs_orb_search_default_params with overrides."""
    return _default_params(CsOrbSearchParams, "cs_orb_search_default_params", kw)


def _u8(a, shape):
    return np.ascontiguousarray(np.asarray(a, np.uint8).reshape(shape))


def _orb_frame_inputs(batch):
    """The frames of a batch dict (synth_orb_search layout: kp_ptr, kp, octave, desc, cam, bounds, scale_factor, n_levels) as C arguments."""
    cam = _f64(batch["cam"], (-1, 5)); n = len(cam)
    bounds, sf, nl = _f64(batch["bounds"], (n, 4)), _f64(batch["scale_factor"], (n,)), _i32(batch["n_levels"])
    ptr = _i32(batch["kp_ptr"])
    if len(ptr) != n + 1 or len(nl) != n:
        raise ValueError("kp_ptr must hold n_frames + 1 entries and n_levels n_frames")
    N = int(ptr[-1]) if n else 0
    kp, octave, desc = _f64(batch["kp"], (N, 3)), _i32(batch["octave"]), _u8(batch["desc"], (N, 32))
    if len(octave) != N:
        raise ValueError("octave must hold one entry per keypoint")
    keep = (ptr, kp, octave, desc, cam, bounds, sf, nl)
    return n, N, keep, (_ip(ptr), _dp(kp), _ip(octave), _u8p(desc), _dp(cam), _dp(bounds), _dp(sf), _ip(nl))


def _orb_job_inputs(batch):
    """The jobs of a batch dict (frame_of_job, pose8, th, max_hamming, flags, query_ptr, X, normal, dist_range, qdesc, skip) as C arguments."""
    pose = _f64(batch["pose8"], (-1, 8)); n = len(pose)
    fj, th, mh, fl, ptr = _i32(batch["frame_of_job"]), _f64(batch["th"], (n,)), _i32(batch["max_hamming"]), _i32(batch["flags"]), _i32(batch["query_ptr"])
    if len(ptr) != n + 1 or len(fj) != n or len(mh) != n or len(fl) != n:
        raise ValueError("query_ptr must hold n_jobs + 1 entries; frame_of_job, max_hamming and flags n_jobs")
    Q = int(ptr[-1]) if n else 0
    X, nrm, dr, qd, skip = _f64(batch["X"], (Q, 3)), _f64(batch["normal"], (Q, 3)), _f64(batch["dist_range"], (Q, 2)), _u8(batch["qdesc"], (Q, 32)), _u8(batch["skip"], (Q,))
    keep = (fj, pose, th, mh, fl, ptr, X, nrm, dr, qd, skip)
    return n, Q, keep, (_ip(fj), _dp(pose), _dp(th), _ip(mh), _ip(fl), _ip(ptr), _dp(X), _dp(nrm), _dp(dr), _u8p(qd), _u8p(skip))


def _orb_outputs(n, Q, inspect=False):
    out = dict(status=np.zeros(Q, np.uint8), best_idx=np.zeros(Q, np.int32), best_dist=np.zeros(Q, np.int32), level=np.zeros(Q, np.uint8), n_ok=np.zeros(n, np.int32))
    args = (_u8p(out["status"]), _ip(out["best_idx"]), _ip(out["best_dist"]), _u8p(out["level"]), _ip(out["n_ok"]))
    if inspect:
        out.update(insp5=np.zeros((Q, 5)), n_window=np.zeros(Q, np.int32), n_candidates=np.zeros(Q, np.int32))
        args += (_dp(out["insp5"]), _ip(out["n_window"]), _ip(out["n_candidates"]))
    return out, args


class OrbSearch(_BatchHandle):
    """cs_orb_search handle: keeps its stream, its buffers and a set of frames on the device between run() calls."""

    _SYM = "cs_orb_search"

    def set_frames(self, batch, params=None):
        """Checks, packs (each frame's grid is built here) and uploads the frames of `batch`; they replace the set the handle held."""
        p = params if params is not None else orb_search_default_params()
        n, N, keep, args = _orb_frame_inputs(batch)
        _chk(lib().cs_orb_search_set_frames(self.h, C.byref(p), n, *args), "cs_orb_search_set_frames")

    def run(self, batch):
        """The jobs of `batch` against the handle's frames -> dict: status, level (Q, uint8), best_idx, best_dist (Q), n_ok (n_jobs)."""
        n, Q, keep, args = _orb_job_inputs(batch)
        out, outs = _orb_outputs(n, Q)
        _chk(lib().cs_orb_search_run(self.h, n, *args, *outs), "cs_orb_search_run")
        return out


def _orb_one_shot(name, batch, params, device, inspect):
    p = params if params is not None else orb_search_default_params()
    nf, N, keep_f, fargs = _orb_frame_inputs(batch)
    nj, Q, keep_j, jargs = _orb_job_inputs(batch)
    out, outs = _orb_outputs(nj, Q, inspect)
    _chk(getattr(lib(), name)(int(device), C.byref(p), nf, *fargs, nj, *jargs, *outs), name)
    return out


def orb_search_jobs(batch, params=None, device=0):
    """cs_orb_search_jobs: the one-shot form, frames and jobs in one call."""
    return _orb_one_shot("cs_orb_search_jobs", batch, params, device, False)


def orb_search_inspect(batch, params=None, device=0):
    """cs_orb_search_inspect: orb_search_jobs' outputs plus insp5 (Q, 5) = u v ur dist radius, n_window and n_candidates of every query."""
    return _orb_one_shot("cs_orb_search_inspect", batch, params, device, True)


def orb_search_mutual(best12, status12, best21, status21):
    """cs_orb_search_mutual -> match12 (n1): j where i -> j and j -> i are both OK, -1 otherwise; runs without a device."""
    b12, b21, s12, s21 = _i32(best12), _i32(best21), _u8(status12, (-1,)), _u8(status21, (-1,))
    if len(b12) != len(s12) or len(b21) != len(s21):
        raise ValueError("one status per best index")
    out, n = np.zeros(len(b12), np.int32), C.c_int()
    _chk(lib().cs_orb_search_mutual(len(b12), _ip(b12), _u8p(s12), len(b21), _ip(b21), _u8p(s21), _ip(out), C.byref(n)), "cs_orb_search_mutual")
    assert n.value == int((out >= 0).sum())
    return out


DECLARED_SYMBOLS += ["cs_pgo_create", "cs_pgo_destroy", "cs_pgo_set_vertices", "cs_pgo_set_estimates", "cs_pgo_set_edges", "cs_pgo_set_lm_params", "cs_pgo_chi2",
                     "cs_pgo_linearize_edges", "cs_pgo_edge_terms", "cs_pgo_optimize", "cs_pgo_get_vertices", "cs_pgo_get_se3", "cs_pgo_correct_points", "cs_pgo_solver_path", "cs_pgo_last_timing"]


def _u8p(a):
    return a.ctypes.data_as(C.POINTER(C.c_ubyte)) if a is not None else None


class PoseGraph:
    """cs_pgo handle: Sim(3) keyframe vertices, EdgeSim3 links, Levenberg-Marquardt (Optimizer::OptimizeEssentialGraph's graph).
    States are qx qy qz qw tx ty tz s, world-to-keyframe."""

    def __init__(self, sim8, fixed=None, fix_scale=None, device=0):
        self.h = C.c_void_p()
        _chk(lib().cs_pgo_create(int(device), C.byref(self.h)), "cs_pgo_create")
        self.nv = self.ne = 0
        self.hist = None
        self.set_vertices(sim8, fixed, fix_scale)

    def set_vertices(self, sim8, fixed=None, fix_scale=None):
        s = _f64(sim8, (-1, 8))
        fx = np.ascontiguousarray(np.asarray(fixed, np.uint8).ravel()) if fixed is not None else None
        fs = np.ascontiguousarray(np.asarray(fix_scale, np.uint8).ravel()) if fix_scale is not None else None
        if (fx is not None and len(fx) != len(s)) or (fs is not None and len(fs) != len(s)):
            raise ValueError("one flag per vertex")
        _chk(lib().cs_pgo_set_vertices(self.h, len(s), _dp(s), _u8p(fx), _u8p(fs)), "cs_pgo_set_vertices")
        self.nv, self.ne = len(s), 0

    def set_estimates(self, sim8):
        s = _f64(sim8, (self.nv, 8))
        _chk(lib().cs_pgo_set_estimates(self.h, _dp(s)), "cs_pgo_set_estimates")

    def set_edges(self, vi, vj, meas8, info49=None):
        vi, vj, m = _i32(vi), _i32(vj), _f64(meas8, (-1, 8))
        w = _f64(info49, (-1, 49)) if info49 is not None else None
        if len(vj) != len(vi) or len(m) != len(vi) or (w is not None and len(w) != len(vi)):
            raise ValueError("one entry per edge")
        _chk(lib().cs_pgo_set_edges(self.h, len(vi), _ip(vi), _ip(vj), _dp(m), _dp(w) if w is not None else None), "cs_pgo_set_edges")
        self.ne = len(vi)

    def set_lm_params(self, user_lambda_init=0.0, max_trials_after_failure=10):
        _chk(lib().cs_pgo_set_lm_params(self.h, C.c_double(user_lambda_init), int(max_trials_after_failure)), "cs_pgo_set_lm_params")

    def chi2(self, each=False):
        c = C.c_double()
        e = np.zeros(self.ne) if each else None
        _chk(lib().cs_pgo_chi2(self.h, C.byref(c), _dp(e) if each else None), "cs_pgo_chi2")
        return (c.value, e) if each else c.value

    def linearize_edges(self):
        """err (E, 7), J_i, J_j (E, 7, 7; row = error component) at the current estimates."""
        e, ji, jj = np.zeros((self.ne, 7)), np.zeros((self.ne, 7, 7)), np.zeros((self.ne, 7, 7))
        _chk(lib().cs_pgo_linearize_edges(self.h, _dp(e), _dp(ji), _dp(jj)), "cs_pgo_linearize_edges")
        return e, ji, jj

    def edge_terms(self):
        """Per edge, at the current estimates: dict Hii, Hij, Hjj (E, 7, 7), bi, bj (E, 7), chi2 (E) -- cs_pgo_edge_terms."""
        E = self.ne
        t = dict(Hii=np.zeros((E, 7, 7)), Hij=np.zeros((E, 7, 7)), Hjj=np.zeros((E, 7, 7)), bi=np.zeros((E, 7)), bj=np.zeros((E, 7)), chi2=np.zeros(E))
        _chk(lib().cs_pgo_edge_terms(self.h, *(_dp(t[k]) for k in ("Hii", "Hij", "Hjj", "bi", "bj", "chi2"))), "cs_pgo_edge_terms")
        return t

    def optimize(self, iters, cap=64):
        done = C.c_int()
        chi, lam, tr = np.zeros(cap), np.zeros(cap), np.zeros(cap, np.int32)
        _chk(lib().cs_pgo_optimize(self.h, int(iters), C.byref(done), _dp(chi), _dp(lam), _ip(tr), cap), "cs_pgo_optimize")
        k = min(done.value, cap)
        self.hist = (chi[:k], lam[:k], tr[:k])
        return done.value

    def history(self):
        """chi2, lambda, LM trials of every iteration of the last optimize()."""
        return self.hist

    def vertices(self):
        s = np.zeros((self.nv, 8))
        _chk(lib().cs_pgo_get_vertices(self.h, _dp(s)), "cs_pgo_get_vertices")
        return s

    def se3(self):
        t = np.zeros((self.nv, 7))
        _chk(lib().cs_pgo_get_se3(self.h, _dp(t)), "cs_pgo_get_se3")
        return t

    def correct_points(self, ref_vertex, xyz):
        r, x = _i32(ref_vertex), _f64(xyz, (-1, 3))
        if len(r) != len(x):
            raise ValueError("one reference vertex per point")
        out = np.zeros_like(x)
        _chk(lib().cs_pgo_correct_points(self.h, len(x), _ip(r), _dp(x), _dp(out)), "cs_pgo_correct_points")
        return out

    def solver_path(self):
        p, f = C.c_int(), C.c_double()
        _chk(lib().cs_pgo_solver_path(self.h, C.byref(p), C.byref(f)), "cs_pgo_solver_path")
        return {0: "dense", 2: "sparse"}[p.value], f.value

    def timing(self):
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        _chk(lib().cs_pgo_last_timing(self.h, C.byref(a), C.byref(b), C.byref(c)), "cs_pgo_last_timing")
        return dict(linearize_ms=a.value, solve_ms=b.value, total_ms=c.value)

    def close(self):
        if getattr(self, "h", None):
            lib().cs_pgo_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def pose_graph_from_dict(g, device=0):
    """A PoseGraph from synth_pgo.ring()'s dict."""
    G = PoseGraph(g["sim8"], g["fixed"], g["fix_scale"], device=device)
    G.set_edges(g["vi"], g["vj"], g["meas8"], g.get("info49"))
    return G
