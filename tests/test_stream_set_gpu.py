"""The detectors of a process share one set of working streams per device (StreamSet, detect_host.cpp): sweeps of different detectors
are queued into the same streams from different host threads.  What a batch computes must not depend on that: every batch that runs
beside the others gives, bit for bit, what the same batch gives alone on a fresh detector -- also with more detectors than the set has
slots, when several host threads enqueue into ONE stream -- and the set's reference count survives detectors that come and go in any order.
"""
import threading

import numpy as np
import pytest

from cube_slam_wu_amd import capi, synth

pytestmark = pytest.mark.gpu

N_DET, DEPTH, STEPS, N_FRAMES = 4, 2, 36, 12
TIME_LIMIT_S = 300.0


def _params(rp=0):
    return capi.default_params(whether_sample_cam_roll_pitch=rp, whether_sample_bbox_height=0, yaw_range_deg=45.0, yaw_step_deg=3.0, host_threads=4)


def _frames(det, bat, n=N_FRAMES):
    """A frame set of its own per (detector, batch): other seeds, other box and segment counts."""
    base = 7000 + 1000 * det + 100 * bat
    return [synth.make_frame(base + i, n_boxes=2 + (i + det) % 4, n_lines=120 + 20 * ((i + bat) % 5)) for i in range(n)]


def _snapshot(bat, n_frames):
    """Counts + every field of every record, as bytes-comparable arrays."""
    out = [bat.counts_bytes()]
    for f in range(n_frames):
        for box in bat.cuboids(f):
            for c in box:
                out.append({k: np.array(v, copy=True) for k, v in c.items()})
    return out


def _same(a, b):
    if len(a) != len(b) or a[0] != b[0]:
        return False
    for x, y in zip(a[1:], b[1:]):
        if x.keys() != y.keys():
            return False
        for k in x:
            xa, ya = np.asarray(x[k]), np.asarray(y[k])
            if xa.shape != ya.shape or not np.array_equal(xa, ya, equal_nan=(xa.dtype.kind == "f")):
                return False
    return True


def _alone(frames, rp=0):
    det = capi.Detector(_params(rp))
    bat = capi.Batch(det, frames)
    bat.run()
    snap = _snapshot(bat, len(frames))
    bat.close(); det.close()
    return snap


def _run_limited(fn):
    """fn on a thread of its own, under the time limit (a sweep that never came back would otherwise hang the suite)."""
    err = []

    def body():
        try:
            fn()
        except BaseException as e:   # surfaced below
            err.append(e)
    t = threading.Thread(target=body, daemon=True)
    t.start()
    t.join(TIME_LIMIT_S)
    if t.is_alive():
        # a sweep that has not come back is a presumed hang of the device: nothing more is started on it, the session ends here
        pytest.exit("test_stream_set_gpu: no result within %.0f s -- ending the session" % TIME_LIMIT_S, returncode=3)
    if err:
        raise err[0]


def _concurrent_equal_alone(N_DET, rp):
    def work():
        n_frames = N_FRAMES if rp == 0 else 4
        steps = STEPS if rp == 0 else 24
        sets = {(d, q): _frames(d, q, n_frames) for d in range(N_DET) for q in range(DEPTH)}
        want = {k: _alone(fr, rp) for k, fr in sets.items()}
        assert len({w[0] for w in want.values()}) > 1      # the frame sets do differ
        dets = [capi.Detector(_params(rp)) for _ in range(N_DET)]
        bats = {k: capi.Batch(dets[k[0]], fr) for k, fr in sets.items()}
        bad, errs = [], []
        start = threading.Barrier(N_DET)

        def drive(d):
            try:
                free, queued = [(d, q) for q in range(DEPTH)], []
                left = steps
                start.wait()
                while True:
                    while free and left > 0:
                        k = free.pop(0)
                        bats[k].submit()
                        queued.append(k)
                        left -= 1
                    if not queued:
                        break
                    k = queued.pop(0)
                    bats[k].collect()
                    if not _same(_snapshot(bats[k], n_frames), want[k]):
                        bad.append(k)
                    free.append(k)
            except BaseException as e:
                errs.append(e)
                start.abort()
        th = [threading.Thread(target=drive, args=(d,)) for d in range(N_DET)]
        [t.start() for t in th]
        [t.join() for t in th]
        for b in bats.values():
            b.close()
        for d in dets:
            d.close()
        if errs:
            raise errs[0]
        assert not bad, "batches that differ from their run alone: %s" % sorted(set(bad))
    _run_limited(work)


@pytest.mark.parametrize("rp", [0, 1])
def test_concurrent_batches_equal_the_same_batches_alone(rp):
    """Four detectors, two batches each, four host threads: a detector per slot of the set."""
    _concurrent_equal_alone(N_DET, rp)


@pytest.mark.parametrize("rp", [0, 1])
def test_more_detectors_than_slots_share_streams(rp):
    """Six detectors: more than the set has slots with four hardware queues and with eight, so two pairs of detectors share a chain stream
    (and the lock around their enqueue blocks) from different host threads."""
    _concurrent_equal_alone(6, rp)


def test_detectors_come_and_go_in_any_order():
    def work():
        frames = [_frames(9, q, 6) for q in range(4)]
        want = [_alone(fr) for fr in frames]       # (every _alone creates and destroys the device's set)

        def check(det, q):
            bat = capi.Batch(det, frames[q])
            bat.run()
            ok = _same(_snapshot(bat, len(frames[q])), want[q])
            bat.close()
            assert ok, q
        a, b = capi.Detector(_params()), capi.Detector(_params())
        check(a, 0); check(b, 1)
        a.close()                                   # the first one goes, the set stays with b
        check(b, 2)
        c = capi.Detector(_params())                # takes the place a left
        check(c, 0); check(b, 3)
        b.close()
        d, e = capi.Detector(_params()), capi.Detector(_params())
        check(e, 1); check(d, 2); check(c, 3)
        e.close(); c.close(); d.close()             # the last one takes the set with it ...
        f = capi.Detector(_params())                # ... and the next one creates it again
        check(f, 0)
        # more live detectors than slots, going in an order of their own: the slots' user counts stay right
        many = [capi.Detector(_params()) for _ in range(6)]
        for i in (5, 0, 3):
            check(many[i], i % 4)
        for i in (1, 4):
            many[i].close()
        g = capi.Detector(_params())
        check(g, 1); check(many[2], 2); check(f, 3)
        for x in (many[0], g, many[5], f, many[3], many[2]):
            x.close()
    _run_limited(work)
