"""ORB-SLAM2's LocalBundleAdjustment schedule (optimize(5) with Huber kernels, outliers to level 1, kernels off, optimize(10), final classification)
on C3- and C4-shaped graphs with half of the projection edges stereo (synth_ba.make_stereo_problem), two routes on a handle whose structure is final:
   python tools/ba_rounds_quick.py [C3|C4|both] [repetitions] [--rebuild-lib PATH/libcubeslam_hip.so]
  rounds    cs_ba_optimize_rounds: the classification on the device, no structure phase between the rounds;
  rebuild   what a caller did before the edge levels existed: cs_ba_optimize(5), cs_ba_get_state, the classification on the host, a fresh edge
            list of the kept edges without kernels (cs_ba_set_edges_proj / _stereo), cs_ba_optimize(10) -- which runs the structure phase again
            -- cs_ba_get_state and the final classification on the host.  --rebuild-lib: a second build of the library (the parent commit's)
            for this route; default: the library of this tree, whose old entry points do the same.
The routes alternate, repetition by repetition, after one untimed pass of each; a host clock around calls that end in a device synchronise.  The
host classification here is vectorised numpy -- a C++ caller's loop would be faster -- so the rebuild route is reported with and without it.
Also: both routes reach the same decisions (level arrays equal, final chi2 within 1e-6).  One JSON line per graph at the end."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cube_slam_wu_amd import capi, synth_ba

args = [a for a in sys.argv[1:] if not a.startswith("--")]
which = args[0] if args else "both"
reps = int(args[1]) if len(args) > 1 else 7
SHAPES = {"C3": (200, 20000, 50), "C4": (1000, 200000, 500)}
TH = (5.991, 7.815)
HUB = (np.sqrt(TH[0]), np.sqrt(TH[1]))
LOCAL_BA = [(5, True, (TH[0], TH[1], 1, 1)), (10, False, (TH[0], TH[1], 1, 0))]

lib_new = capi.lib()
lib_old = lib_new
if "--rebuild-lib" in sys.argv:
    lib_old = C.CDLL(os.path.abspath(sys.argv[sys.argv.index("--rebuild-lib") + 1]))
    lib_old.cs_last_error.restype = C.c_char_p


def use(lib):
    capi._lib = lib


def host_classify(pr, cams, pts, keep_m, keep_s, sticky):
    """chi2 > threshold or depth not positive, over the mono and the stereo list (float invz / bf of the stereo error as in the library)."""
    def cam_frame(e_pt, e_cam):
        c = cams[e_cam]
        return synth_ba.quat_rot(c[:, 3:], pts[e_pt]) + c[:, :3]
    Xc = cam_frame(pr["e_pt"], pr["e_cam"])
    k = pr["e_intr"]
    e = pr["e_uv"] - np.stack([Xc[:, 0] / Xc[:, 2] * k[:, 0] + k[:, 2], Xc[:, 1] / Xc[:, 2] * k[:, 1] + k[:, 3]], 1)
    i4 = pr["e_info"]
    chi = e[:, 0] * (i4[:, 0] * e[:, 0] + i4[:, 1] * e[:, 1]) + e[:, 1] * (i4[:, 2] * e[:, 0] + i4[:, 3] * e[:, 1])
    out_m = (chi > TH[0]) | ~(Xc[:, 2] > 0)
    Xs = cam_frame(pr["se_pt"], pr["se_cam"])
    k5 = pr["se_intr"]
    invz = (1.0 / Xs[:, 2]).astype(np.float32)
    ul = Xs[:, 0] * invz.astype(np.float64) * k5[:, 0] + k5[:, 2]
    v = Xs[:, 1] * invz.astype(np.float64) * k5[:, 1] + k5[:, 3]
    ur = ul - (k5[:, 4].astype(np.float32) * invz).astype(np.float64)
    es = pr["se_uvr"] - np.stack([ul, v, ur], 1)
    chis = np.einsum("ei,eij,ej->e", es, pr["se_info"].reshape(-1, 3, 3), es)
    out_s = (chis > TH[1]) | ~(Xs[:, 2] > 0)
    if sticky:
        out_m, out_s = out_m | ~keep_m, out_s | ~keep_s
    return out_m, out_s


def set_full(P, pr):
    P.set_edges_proj(pr["e_pt"], pr["e_cam"], pr["e_uv"], pr["e_info"], pr["e_intr"], np.full(len(pr["e_pt"]), HUB[0]))
    P.set_edges_proj_stereo(pr["se_pt"], pr["se_cam"], pr["se_uvr"], pr["se_info"], pr["se_intr"], np.full(len(pr["se_pt"]), HUB[1]))


def route_rounds(P, pr):
    use(lib_new)
    P.set_estimates(pr["cams"], pr["cuboids"], pr["points"])
    P.set_edge_levels(capi.EDGE_PROJ, None); P.set_edge_levels(capi.EDGE_PROJ_STEREO, None)
    P.set_kernels_enabled(capi.EDGE_PROJ, True); P.set_kernels_enabled(capi.EDGE_PROJ_STEREO, True)
    P.compute_errors()                      # (untimed: the stream idle, the structure final)
    s0 = P.timing()["structure_ms"]
    t0 = time.perf_counter()
    done, nout = P.optimize_rounds(LOCAL_BA)
    t = (time.perf_counter() - t0) * 1e3
    lv = (P.edge_levels(capi.EDGE_PROJ).astype(bool), P.edge_levels(capi.EDGE_PROJ_STEREO).astype(bool))
    return dict(total_ms=t, structure_ms=P.timing()["structure_ms"] - s0, done=[int(x) for x in done], levels=lv, chi=float(P.rounds_history()[1][0][-1]))


def route_rebuild(P, pr):
    use(lib_old)
    P.set_estimates(pr["cams"], pr["cuboids"], pr["points"])
    set_full(P, pr)
    P.compute_errors()                      # (untimed: the full graph's structure phase)
    nm, ns = len(pr["e_pt"]), len(pr["se_pt"])
    t = {}
    c = time.perf_counter
    t0 = c(); d1 = P.optimize(5); t["optimize5_ms"] = (c() - t0) * 1e3
    t0 = c(); cams, _, pts = P.state(); t["get_state_ms"] = (c() - t0) * 1e3
    t0 = c(); o_m, o_s = host_classify(pr, cams, pts, np.ones(nm, bool), np.ones(ns, bool), True); t["host_classify_ms"] = (c() - t0) * 1e3
    t0 = c()
    km, ks = ~o_m, ~o_s
    P.set_edges_proj(pr["e_pt"][km], pr["e_cam"][km], pr["e_uv"][km], pr["e_info"][km], pr["e_intr"][km], None)
    P.set_edges_proj_stereo(pr["se_pt"][ks], pr["se_cam"][ks], pr["se_uvr"][ks], pr["se_info"][ks], pr["se_intr"][ks], None)
    t["new_edge_lists_ms"] = (c() - t0) * 1e3
    t0 = c(); d2 = P.optimize(10); t["optimize10_with_structure_ms"] = (c() - t0) * 1e3
    chi = float(P.history()[0][-1])
    t0 = c(); cams, _, pts = P.state(); t["get_state_ms"] += (c() - t0) * 1e3
    t0 = c(); f_m, f_s = host_classify(pr, cams, pts, km, ks, False); t["host_classify_ms"] += (c() - t0) * 1e3
    t["total_ms"] = sum(t.values())
    t["total_without_host_classify_ms"] = t["total_ms"] - t["host_classify_ms"]
    return dict(t, done=[d1, d2], levels=(f_m, f_s), chi=chi)


for cfg in (("C3", "C4") if which == "both" else (which,)):
    nc, npt, no = SHAPES[cfg]
    pr = synth_ba.make_stereo_problem(stereo_share=0.5, n_cams=nc, n_points=npt, n_cuboids=no, seed=42)
    use(lib_new)
    A = capi.BaProblem(pr["cams"], pr["cam_fixed"], pr["cuboids"], pr["cub_fixed"], pr["points"], pr["pt_fixed"])
    set_full(A, pr)
    if len(pr["ce_cam"]):
        A.set_edges_cuboid(pr["ce_cam"], pr["ce_cub"], pr["ce_meas"], pr["ce_info"])
    A.set_edges_odom(pr["oe_i"], pr["oe_j"], pr["oe_meas"], pr["oe_info"])
    use(lib_old)
    B = capi.BaProblem(pr["cams"], pr["cam_fixed"], pr["cuboids"], pr["cub_fixed"], pr["points"], pr["pt_fixed"])
    if len(pr["ce_cam"]):
        B.set_edges_cuboid(pr["ce_cam"], pr["ce_cub"], pr["ce_meas"], pr["ce_info"])
    B.set_edges_odom(pr["oe_i"], pr["oe_j"], pr["oe_meas"], pr["oe_info"])
    ra, rb = route_rounds(A, pr), route_rebuild(B, pr)          # untimed pass of each
    same = bool(np.array_equal(ra["levels"][0], rb["levels"][0]) and np.array_equal(ra["levels"][1], rb["levels"][1]))
    print("%s: %d mono + %d stereo edges; outliers at the end %d + %d; both routes decide alike: %s; final chi2 %.6f / %.6f; iterations %s / %s"
          % (cfg, len(pr["e_pt"]), len(pr["se_pt"]), ra["levels"][0].sum(), ra["levels"][1].sum(), same, ra["chi"], rb["chi"], ra["done"], rb["done"]), flush=True)
    ta, tb = [], []
    for _ in range(reps):
        ta.append(route_rounds(A, pr)); tb.append(route_rebuild(B, pr))
    med = lambda rows, k: float(np.median([r[k] for r in rows]))
    out = {"config": cfg, "repetitions": reps, "rebuild_route_library": "other build" if lib_old is not lib_new else "this build", "same_decisions": same,
           "final_chi2_rel_diff": abs(ra["chi"] - rb["chi"]) / rb["chi"],
           "rounds": {"total_ms_median": med(ta, "total_ms"), "total_ms_min_max": [min(r["total_ms"] for r in ta), max(r["total_ms"] for r in ta)], "structure_ms": med(ta, "structure_ms")},
           "rebuild": {k + "_median": med(tb, k) for k in tb[0] if k.endswith("_ms")}}
    out["rebuild"]["total_ms_min_max"] = [min(r["total_ms"] for r in tb), max(r["total_ms"] for r in tb)]
    out["rebuild_over_rounds"] = out["rebuild"]["total_ms_median"] / out["rounds"]["total_ms_median"]
    out["rebuild_without_host_classify_over_rounds"] = out["rebuild"]["total_without_host_classify_ms_median"] / out["rounds"]["total_ms_median"]
    print(json.dumps(out), flush=True)
    use(lib_new); A.close()
    use(lib_old); B.close()
use(lib_new)
