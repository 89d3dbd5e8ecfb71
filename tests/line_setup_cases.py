"""Inputs for the line setup's table test (cs_check_line_setup: one frame's segments against a set of expanded ROIs), and a plain
float64 statement of merge_break_lines (object_3d_util.cpp:431-543) that says what each case promises: the segments inside every ROI,
the size class that picks the kernel instance, the merges and -- for the cases that place a merge on a boundary of the kernels' data
layout -- the (as, bs, last) triple of every round.  The statement decides with math.atan2 and sqrt where the library decides with its
own exact atan2, so it speaks only for inputs whose every pair keeps clear of the three thresholds: all cases but those marked
clear=False, which are built to sit on them and are compared device against host only.

Layout.  Segments that must not merge are 36 px long, one per slot of a vertical strip, slots 60 px apart, directions 6 degrees apart
(merge_break_lines merges below 5 degrees and below a 20 px gap: two slots' end points are at least 24 px apart).  A pair that must merge
is two collinear 40 px pieces 5 px apart in one slot.  Input order and slot order are the same, so a ROI over the strip's upper part holds
a prefix of the input; segments meant to lie outside every ROI go to a second strip 1000 px to the right."""
import math

import numpy as np

LS_SMALL, LS_MID, LS_CAP = 128, 256, 512      # rows of the three kernel instances (csrc/line_setup_kernels.hip)
DIST_THRE, ANGLE_THRE_DEG, LEN_THRE = 20.0, 5.0, 30.0
MAX_MERGES = 400      # the host stops after 500 rounds, the device after CAP: the cases stay below both


def size_class(n_in):
    return "small" if n_in <= LS_SMALL else ("mid" if n_in <= LS_MID else "big")


def inside(lines, roi):
    """Mask of the segments with both end points inside the inclusive bounds (left, top, right, bottom)."""
    L = np.asarray(lines, np.float64).reshape(-1, 4)
    el, et, er, eb = roi
    return (el <= L[:, 0]) & (L[:, 0] <= er) & (et <= L[:, 1]) & (L[:, 1] <= eb) & (el <= L[:, 2]) & (L[:, 2] <= er) & (et <= L[:, 3]) & (L[:, 3] <= eb)


def _angle(s):
    return math.atan2(s[3] - s[1], s[2] - s[0])


def _pair_merges(A, B, ang_a, ang_b, dist_thre, athre):
    """The three tests for rows A, B (A the lower index): the merged row, or None."""
    diff = abs(ang_a - ang_b)
    if not min(diff, math.pi - diff) < athre:
        return None
    d_ab = math.sqrt((A[2] - B[0]) ** 2 + (A[3] - B[1]) ** 2)
    d_ba = math.sqrt((B[2] - A[0]) ** 2 + (B[3] - A[1]) ** 2)
    if not (d_ab < dist_thre or d_ba < dist_thre):
        return None
    s = A[0:2] if A[0] < B[0] else B[0:2]      # (a tie goes to B)
    e = A[2:4] if A[2] > B[2] else B[2:4]
    t = abs(ang_a - math.atan2(e[1] - s[1], e[0] - s[0]))
    if not min(t, math.pi - t) < athre:
        return None
    return [s[0], s[1], e[0], e[1]]


def merge_break_lines(lines, dist_thre=DIST_THRE, angle_thre_deg=ANGLE_THRE_DEG, len_thre=LEN_THRE):
    """merge_break_lines on n x 4 rows: (the rows left, longer than len_thre, in order; the rounds' (as, bs, last) triples)."""
    L = [list(map(float, s)) for s in np.asarray(lines, np.float64).reshape(-1, 4)]
    ang = [_angle(s) for s in L]
    athre = angle_thre_deg / 180.0 * math.pi
    rounds = []
    merged = True
    while merged:
        merged = False
        for a in range(len(L) - 1):
            for b in range(a + 1, len(L)):
                m = _pair_merges(L[a], L[b], ang[a], ang[b], dist_thre, athre)
                if m is None:
                    continue
                rounds.append((a, b, len(L) - 1))
                L[a], ang[a] = m, _angle(m)
                L[b], ang[b] = L[-1], ang[-1]      # the last row moves into b
                L.pop(); ang.pop()
                merged = True
                break
            if merged:
                break
    kept = [s for s in L if not len_thre > 0 or math.sqrt((s[2] - s[0]) ** 2 + (s[3] - s[1]) ** 2) > len_thre]
    return np.asarray(kept, np.float64).reshape(-1, 4), rounds


# ---- building blocks
X_IN, X_OUT, Y0, PITCH = 200.0, 1200.0, 100.0, 60.0
ROI_RIGHT = 400      # a ROI over the inside strip: left 0, right 400


def _slot_y(slot):
    return Y0 + PITCH * slot


def _separate(slot, q, cx=X_IN):
    a = np.deg2rad(6.0 * (q % 30) - 87.0)      # (x1 < x2: cos > 0 on -87..87)
    y = _slot_y(slot)
    return [cx - 18 * np.cos(a), y - 18 * np.sin(a), cx + 18 * np.cos(a), y + 18 * np.sin(a)]


def _piece(slot, which):
    """One half of a pair that merges: collinear, horizontal, 5 px apart."""
    y = _slot_y(slot)
    return [X_IN - 42.5, y, X_IN - 2.5, y] if which == 0 else [X_IN + 2.5, y, X_IN + 42.5, y]


def _prefix_roi(n_slots):
    """The ROI over the first n_slots slots of the inside strip."""
    return [0, 0, ROI_RIGHT, int(_slot_y(n_slots - 1) + PITCH / 2) if n_slots > 0 else 10]


def strip(n, pairs=(), outside=()):
    """n input segments: separate ones, except that pairs = [(i, j), ...] puts the two pieces of a merging pair at input positions i < j
    (one slot for both, the slot of i) and the positions in `outside` go to the strip outside every ROI."""
    piece = {}
    for i, j in pairs:
        assert i < j and i not in piece and j not in piece
        piece[i], piece[j] = (i, 0), (i, 1)
    out = set(outside)
    assert not out & set(piece)
    return np.array([_piece(*piece[q]) if q in piece else _separate(q, q, X_OUT if q in out else X_IN) for q in range(n)])


def _case(name, lines, rois, yt=None, clear=True, rounds=None, len_thre=LEN_THRE):
    rois = np.asarray(rois, np.int32).reshape(-1, 4)
    yt = np.ones((len(rois), 2), np.int32) if yt is None else np.asarray(yt, np.int32)
    return {"name": name, "lines": np.asarray(lines, np.float64).reshape(-1, 4), "rois": rois, "yt": yt, "clear": clear,
            "dist_thre": DIST_THRE, "angle_thre_deg": ANGLE_THRE_DEG, "len_thre": len_thre, "rounds": rounds, "promise": {}}


# ---- the cases
INSIDE_COUNTS = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512]


def case_counts():
    """No merge at all; every inside count at which the instance or a lane's row count changes, the classes mixed in one call, and two
    jobs the sweep skips (no yaw samples / no top-edge samples) between them."""
    c = _case("counts", strip(512), [_prefix_roi(k) for k in INSIDE_COUNTS] + [_prefix_roi(300), _prefix_roi(40)])
    c["yt"][-2] = (0, 1); c["yt"][-1] = (1, 0)
    c["promise"] = {"n_in": INSIDE_COUNTS + [300, 40], "merges": [0] * (len(INSIDE_COUNTS) + 2), "skipped": [len(INSIDE_COUNTS), len(INSIDE_COUNTS) + 1]}
    return c


def boundary_scenarios(N):
    """(pairs at input positions, the rounds they must produce) for a job of N rows, N - 1 > 80: merges on the 64-row word boundary."""
    last = N - 1
    return {
        "as<64<=bs": ([(10, 70)], [(10, 70, last)]),
        "both>=64": ([(70, 80)], [(70, 80, last)]),
        "bs==last": ([(10, last)], [(10, last, last)]),
        "bs==63": ([(10, 63)], [(10, 63, last)]),
        "bs==62": ([(10, 62)], [(10, 62, last)]),
        # the old last row is the second pair's far piece: it moves to bs and ...
        "moved,partner-behind-62": ([(10, 62), (63, last)], [(10, 62, last), (62, 63, last - 1)]),      # ... meets its partner in the row behind it
        "moved,partner-behind-63": ([(10, 63), (80, last)], [(10, 63, last), (63, 80, last - 1)]),      # ... across the word boundary
        "moved,partner-behind-30": ([(10, 30), (50, last)], [(10, 30, last), (30, 50, last - 1)]),
        "moved,partner-before,word0": ([(10, 30), (20, last)], [(10, 30, last), (20, 30, last - 1)]),   # ... its partner's bit follows it
        "moved,partner-before,word1": ([(10, 70), (20, last)], [(10, 70, last), (20, 70, last - 1)]),
    }


def cases_boundary():
    """One ROI per call, one or two merges, at 100 rows (the register instance), 200 rows (the 256-row instance) and, for the total that
    falls onto a multiple of 64, 65 and 193 rows; one pair in the last word of a 512-row job."""
    out = []
    for N in (100, 200):
        for name, (pairs, rounds) in boundary_scenarios(N).items():
            out.append(_case("boundary-%d-%s" % (N, name), strip(N, pairs), [_prefix_roi(N)], rounds=[rounds]))
    for N in (65, 193):      # the last row of the last word goes: 65 -> 64 rows, 193 -> 192
        out.append(_case("boundary-%d-total-onto-word" % N, strip(N, [(10, 30)]), [_prefix_roi(N)], rounds=[[(10, 30, N - 1)]]))
    out.append(_case("boundary-512-last-word", strip(512, [(460, 500)]), [_prefix_roi(512)], rounds=[[(460, 500, 511)]]))
    for c in out:
        c["promise"] = {"n_in": [len(c["lines"])], "merges": [len(c["rounds"][0])]}
    return out


def cases_late_partner():
    """A row BEFORE `as` that is a partner of the merged row only: U (row 5) is 36 px behind S (row 10) and fails the third test with T
    (row 30) alone -- the would-be merged segment turns 6.5 degrees --, but passes all three with S + T (3.5 degrees)."""
    out = []
    for N in (100, 200):
        L = strip(N)
        y = _slot_y(5)
        L[5] = [X_IN + 40, y, X_IN + 80, y]             # U
        L[10] = [X_IN - 50, y + 8, X_IN + 5, y + 8]     # S
        L[30] = [X_IN + 10, y + 8, X_IN + 35, y + 8]    # T
        # (the slots of rows 10 and 30 stay empty, the neighbours of slot 5 are 60 px away)
        c = _case("late-partner-%d" % N, L, [_prefix_roi(N)], rounds=[[(10, 30, N - 1), (5, 10, N - 2)]])
        c["promise"] = {"n_in": [N], "merges": [2]}
        out.append(c)
    return out


def case_chains():
    """Long collinear chains of broken pieces, in shuffled input order, that merge down to one row: 100 pieces (register instance), 150
    (256-row instance), and both beside 150 separate segments (512-row instance: 400 rows, 248 merges)."""
    rng = np.random.default_rng(5)

    def chain(k, y):
        return [[100.0 + 45 * i, y, 140.0 + 45 * i, y] for i in range(k)]
    sep = [_separate(12 + q, q) for q in range(150)]
    rows = chain(100, 100.0) + chain(150, 300.0) + sep
    L = np.array(rows)[rng.permutation(len(rows))]
    c = _case("chains", L, [[0, 50, 8000, 150], [0, 250, 8000, 350], [0, 0, 8000, 12000]])
    c["promise"] = {"n_in": [100, 150, 400], "merges": [99, 149, 248], "m": [1, 1, 152]}
    return c


def case_interleaved():
    """Segments outside the ROI between the inside ones, so that a row's place differs from its input position in every 64-lane chunk; three
    ROIs over prefixes of the strip -- one per instance -- and four merges whose pieces lie in different chunks."""
    outside = [q for q in range(512) if q % 3 == 1 or q % 64 == 0]
    pairs = [(2, 300), (5, 60), (65, 132), (200, 203)]
    L = strip(512, pairs, outside)
    cuts = [150, 300, 512]
    c = _case("interleaved", L, [_prefix_roi(k) for k in cuts])
    slot = {q: q for q in range(512) if q not in set(outside)}
    slot.update({j: i for i, j in pairs})      # (a pair's second piece lies in the slot of the first: inside with it, rows later in the input)
    c["promise"] = {"n_in": [sum(1 for s in slot.values() if s < k) for k in cuts], "merges": [sum(1 for i, _ in pairs if i < k) for k in cuts]}
    return c


def case_many_jobs():
    """More crowded jobs than the listed kernels' grid of 1 024 workgroups: 1 040 ROIs of 129 .. 136 rows with one merge each, four of the
    512-row class and four small ones in the same call."""
    L = strip(300, [(3, 100)])
    ks = [129 + (q % 8) for q in range(1040)] + [257, 280, 299, 300] + [0, 1, 64, 128]
    c = _case("many-jobs", L, [_prefix_roi(k) for k in ks])
    # (the pair's second piece, input position 100, lies in slot 3 with the first)
    c["promise"] = {"n_in": [k + (1 if 3 < k <= 100 else 0) for k in ks], "merges": [1 if k > 3 else 0 for k in ks]}
    return c


def _threshold_rows():
    """Groups of two or three rows, 200 px apart, each on one of the thresholds (or special values)."""
    eps, groups = 1e-6, []
    a5 = np.deg2rad(5.0)
    for d in (-eps, +eps):      # angle difference of the pair: 5 degrees -+ 1e-6 rad (the float test's margin is 1.5e-5)
        groups.append([[0, 0, 40, 0], [45, 0, 45 + 40 * np.cos(a5 + d), 40 * np.sin(a5 + d)]])
    for d in (-eps, +eps):      # angle of the merged segment against A's: 5 degrees -+ 1e-6 rad
        groups.append([[0, 0, 40, 0], [45, 85 * np.tan(a5 + d), 85, 85 * np.tan(a5 + d)]])
    for d in (-1e-9, 0.0, +1e-9):      # end-point gap: 20 px -+ 1e-9
        groups.append([[0, 0, 40, 0], [60 + d, 0, 100, 0]])
    groups.append([[0, 0, 40, 0], [45, 0, 45, 0]])              # a zero-length segment (its float angle is NaN) beside a partner
    groups.append([[10, 5, 10, 5], [50, 9, 50, 9]])             # two of them
    groups.append([[0, 0, 35, 0], [0, 2, 15, 2]])               # A.x1 == B.x1: the merged segment starts at B's start
    groups.append([[0, 0, 35, 0], [5, 2, 35, 2]])               # A.x2 == B.x2: it ends at B's end
    up, down = np.nextafter(30.0, 40.0), np.nextafter(30.0, 20.0)
    groups.append([[0, 0, 30, 0], [0, 50, up, 50], [0, 100, down, 100]])      # lengths 30, 30 + ulp, 30 - ulp
    groups.append([[0, 0, 18, 24], [60, 0, 60 + 18, np.nextafter(24.0, 30.0)]])   # 18-24-30: exactly 30, and a hair longer
    rows = []
    for g, grp in enumerate(groups):
        for s in grp:
            rows.append([s[0] + 50, s[1] + 100 + 200 * g, s[2] + 50, s[3] + 100 + 200 * g])
    return rows


def cases_thresholds():
    """Rows on the thresholds -- alone (the register instance), beside 135 separate segments (the 256-row instance) and beside 270 (the
    512-row one); the same with len_thre = 0, which keeps every row.  Device against host only: the statement does not speak here."""
    out = []
    T = _threshold_rows()
    far = int(max(r[3] for r in T)) + 300
    for pad in (0, 135, 270):
        sep = [[s[0], s[1] + far, s[2], s[3] + far] for s in (_separate(q, q) for q in range(pad))]
        rows = T[:7] + sep + T[7:]
        for len_thre in (LEN_THRE, 0.0):
            out.append(_case("thresholds-pad%d-len%g" % (pad, len_thre), rows, [[0, 0, 2000, 100000]], clear=False, len_thre=len_thre))
            out[-1]["promise"] = {"n_in": [len(rows)]}
    return out


def all_cases():
    return [case_counts()] + cases_boundary() + cases_late_partner() + [case_chains(), case_interleaved(), case_many_jobs()] + cases_thresholds()


def statement(case):
    """What the float64 statement says about every ROI of a case: a list of (inside count, rows left (m x 4), rounds); a skipped job has
    no rows.  ROIs that hold the same segments share one evaluation."""
    memo, out = {}, []
    for roi, (Y, T) in zip(case["rois"], case["yt"]):
        mask = inside(case["lines"], roi)
        key = mask.tobytes()
        if key not in memo:
            memo[key] = merge_break_lines(case["lines"][mask], case["dist_thre"], case["angle_thre_deg"], case["len_thre"])
        rows, rounds = memo[key]
        out.append((int(mask.sum()), rows if Y and T else rows[:0], rounds))
    return out
