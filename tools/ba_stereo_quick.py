"""LM iterations/s of C3- and C4-shaped bundle adjustments with a share of stereo projection edges (synth_ba.make_stereo_problem), beside the
mono graph of the same shape -- the rate of the stereo path, which bench.py does not measure:
   python tools/ba_stereo_quick.py [C3|C4|both] [iterations]
Per share (0, 0.5, 1): it/s of cs_ba_optimize, the wall time per iteration, and the per-iteration device time of the stage split
(cs_ba_set_stage_timing: linearisation, Schur / reduce, solve, ...) on a fresh handle.  One JSON line per graph at the end."""
import json, sys, time, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cube_slam_wu_amd import capi, synth_ba

which = sys.argv[1] if len(sys.argv) > 1 else "both"
iters = int(sys.argv[2]) if len(sys.argv) > 2 else 10
SHAPES = {"C3": (200, 20000, 50), "C4": (1000, 200000, 500)}


def rate(pr):
    P = capi.ba_from_dict(pr)
    P.optimize(1)                                   # structure phase + first (classic) linearisation
    best = 0.0
    for _ in range(3):
        t0 = time.perf_counter()
        n = P.optimize(iters)
        best = max(best, n / (time.perf_counter() - t0))
    layout = P.schur_layout()
    P.close()
    P = capi.ba_from_dict(pr)
    P.stage_timing(True)
    P.optimize(1)
    tb = P.timing()
    n = P.optimize(iters)
    ta = P.timing()
    P.close()
    return best, {k[:-3]: round((ta[k] - tb[k]) / max(1, n), 4) for k in ta if k.endswith("_ms") and k != "total_ms"}, layout


for cfg in (("C3", "C4") if which == "both" else (which,)):
    nc, npt, no = SHAPES[cfg]
    out = {"config": cfg}
    for share in (0.0, 0.5, 1.0):
        pr = synth_ba.make_stereo_problem(stereo_share=share, n_cams=nc, n_points=npt, n_cuboids=no, seed=42)
        its, split, layout = rate(pr)
        out["share_%g" % share] = {"mono_edges": len(pr["e_pt"]), "stereo_edges": len(pr["se_pt"]), "it_per_s": round(its, 1), "ms_per_it": round(1e3 / its, 4), "stage_ms_per_it": split, "fused": layout[0]}
        print("%s stereo share %.1f: %d mono + %d stereo edges, %.1f it/s (%.3f ms/it); stage split per iteration: %s" % (cfg, share, len(pr["e_pt"]), len(pr["se_pt"]), its, 1e3 / its, split), flush=True)
    out["ratio_share_1_over_mono"] = round(out["share_0"]["it_per_s"] / out["share_1"]["it_per_s"], 4)
    print(json.dumps(out), flush=True)
