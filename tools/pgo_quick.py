"""Sim(3) pose-graph optimisation (capi.PoseGraph) on rings of keyframes with 5 % random long links: ms per LM iteration, split into
linearise and solve, and the back end that solved; beside it cs_ba_optimize on the same topology as an SE(3) graph of cameras and
odometry edges, the closest existing path.
   python tools/pgo_quick.py [n ...]      (default 200 1000 2000; CS_PGO_FORCE_DENSE=1 selects rocSOLVER)"""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from cube_slam_wu_amd import capi, synth_pgo

ITER = 5


def se3_of(sim8):
    q = sim8[:, :4] / np.linalg.norm(sim8[:, :4], axis=1, keepdims=True)
    return np.concatenate([sim8[:, 4:7] / sim8[:, 7:8], q], 1)


for n in [int(a) for a in sys.argv[1:]] or [200, 1000, 2000]:
    g = synth_pgo.ring(n, 3, long_links=0.05)
    t0 = time.perf_counter()
    G = capi.pose_graph_from_dict(g)
    t_struct = (time.perf_counter() - t0) * 1e3
    G.optimize(1)                                  # first launches
    G.set_estimates(g["sim8"])
    t0 = time.perf_counter()
    done = G.optimize(ITER)
    wall = (time.perf_counter() - t0) * 1e3
    chi, lam, trials = G.history()
    tm = G.timing()
    path, fill = G.solver_path()
    print("pgo  n %5d edges %5d unknowns %6d  %-6s fill %.4f  structure %.1f ms  %d iterations, trials %s: %.3f ms / iteration (linearise %.3f, solve %.3f; wall %.3f)  chi2 %.4e -> %.4e"
          % (n, len(g["vi"]), 7 * (n - 1), path, fill, t_struct, done, trials.tolist(), tm["total_ms"] / done, tm["linearize_ms"] / done, tm["solve_ms"] / done, wall / done, chi[0], chi[-1]))
    G.close()
    try:
        B = capi.BaProblem(se3_of(g["sim8"]), g["fixed"].astype(np.int32))
        B.set_edges_odom(g["vi"], g["vj"], se3_of(g["meas8"]), np.tile(np.eye(6).ravel(), (len(g["vi"]), 1)))
        B.optimize(1)
        B.set_estimates(cams=se3_of(g["sim8"]))
        t0 = time.perf_counter()
        done = B.optimize(ITER)
        wall = (time.perf_counter() - t0) * 1e3
        print("ba   n %5d edges %5d unknowns %6d  %-6s  %d iterations, trials %s: wall %.3f ms / iteration" % (n, len(g["vi"]), 6 * (n - 1), B.solver_path(), done, B.history()[2].tolist(), wall / done))
        B.close()
    except Exception as ex:      # (cs_ba is a bundle adjustment: a graph without landmarks may be refused)
        print("ba   n %5d: no figure -- %s" % (n, ex))
