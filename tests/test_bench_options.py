"""bench.py's options without a GPU: what a plain run leaves out and --full keeps, and the layout, size cap and determinism of
--dump-outputs (dump_outputs over a stand-in for capi.Batch whose records are cs_cuboid structs filled with known values)."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_plain_run_leaves_the_other_legs_out_and_full_keeps_them(capsys):
    bench = _bench()
    plain = bench.parse_args(["--steps", "7", "--warmup", "2"])
    assert (plain.steps, plain.warmup, plain.full) == (7, 2, False)
    for k, v in bench.PLAIN_LEGS.items():
        assert getattr(plain, k) == v, k
    assert capsys.readouterr().err == ""
    full = bench.parse_args(["--full", "--latency-calls", "60", "--ba", "C3"])
    assert full.full and full.latency_calls == 60 and full.ba == "C3" and full.steady_steps == 200 and not full.no_cpu_baseline
    assert capsys.readouterr().err == ""
    # an option that asks for a leg is named when a plain run drops it; one that turns a leg off is not
    asked = bench.parse_args(["--latency-calls", "60", "--ba", "C3", "--ba-iters", "4", "--no-edge", "--rp-frames", "0"])
    assert asked.latency_calls == 0 and asked.ba == "none"
    err = capsys.readouterr().err
    assert "--latency-calls" in err and "--ba," in err and "--ba-iters" in err and "--no-edge" not in err and "--rp-frames" not in err
    with pytest.raises(SystemExit):
        bench.parse_args(["--steps", "0"])


class _Batch:
    """n_frames x max_boxes boxes, 0-2 records each; every field of record (f, b, k) holds values derived from (f, b, k)"""

    def __init__(self, n_frames=40, max_boxes=3):
        from cube_slam_wu_amd import capi
        self.capi = capi
        self.n_frames, self.max_boxes = n_frames, max_boxes
        self._counts = np.random.default_rng(5).integers(0, 3, n_frames * max_boxes).astype(np.int32)

    def record(self, f, b, k):
        c = self.capi.CsCuboid()
        base = 1000.0 * f + 10.0 * b + k
        for name, typ in c._fields_:
            field = getattr(c, name)
            if hasattr(field, "__len__"):
                for i in range(len(field)):
                    field[i] = type(field[i])(base + i + 0.25 if isinstance(field[i], float) else int(base) + i)
            else:
                setattr(c, name, base + 0.5)
        return self.capi.cuboid_to_dict(c)

    def cuboids(self, f):
        return [[self.record(f, b, k) for k in range(int(self._counts[f * self.max_boxes + b]))] for b in range(self.max_boxes)]


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_layout(tmp_path):
    bench = _bench()
    bat = _Batch()
    bench.dump_outputs(bat, str(tmp_path / "a"))
    bench.dump_outputs(bat, str(tmp_path / "b"))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)
    fields = [n for n, _ in bat.capi.CsCuboid._fields_]
    assert sorted(a) == sorted(fields + ["frames", "counts", "index"])
    assert all(v.dtype == np.float64 for v in a.values())
    n = int(bat._counts.sum())
    assert np.array_equal(a["frames"], np.arange(bat.n_frames)) and np.array_equal(a["counts"], bat._counts.reshape(bat.n_frames, bat.max_boxes))
    assert a["index"].shape == (n, 3) and all(a[k].shape[0] == n for k in fields)
    for i, (f, bx, k) in enumerate(a["index"].astype(int)):
        rec = bat.record(f, bx, k)
        for name in fields:
            assert np.array_equal(a[name][i], np.asarray(rec[name], dtype=np.float64)), (i, name)


def test_dump_outputs_samples_a_fixed_set_of_frames_above_the_cap(tmp_path, monkeypatch):
    bench = _bench()
    bat = _Batch(n_frames=400)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", (64 << 10) + 60000)
    bench.dump_outputs(bat, str(tmp_path / "a"))
    bench.dump_outputs(bat, str(tmp_path / "b"))
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    total = sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= bench.DUMP_LIMIT_BYTES
    fr = a["frames"].astype(int)
    assert 0 < len(fr) < bat.n_frames and np.all(np.diff(fr) > 0)
    assert np.array_equal(a["counts"], bat._counts.reshape(bat.n_frames, bat.max_boxes)[fr])
    assert set(a["index"][:, 0].astype(int)) <= set(fr) and len(a["index"]) == int(a["counts"].sum())
