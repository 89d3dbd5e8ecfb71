"""Host logic of the bundle adjustment's structure phase (cube_slam_wu_amd/csrc/ba_host.cpp: BlockSolver::buildStructure,
block_solver.hpp:142-295 -- index maps, camera sets, orderings, edge orders, the Schur schedule) WITHOUT a GPU: the library runs under
tools/hostonly/nohip_shim.cpp (device memory is host memory, copies are memcpy, kernels do not run -- nothing is computed), and
cs_ba_structure_digest fingerprints every index table the phase uploads.  Held to each other:
  * the threaded loops (two-level grouping of the edges by landmark, hashed camera sets, per-range counting sorts; from 20 k edges) and the
    same phase on one thread (CS_BA_STRUCT_THREADS=1);
  * a graph grown frame by frame through cs_ba_append_* and the same graph set up at once;
  * the three pose-edge classes (EdgeSE3Cuboid, EdgeSE3CuboidProj, odometry) set at once and grown through their append calls, with kernels, levels
    and a kernel switch on top: tables, cs_ba_dump's bytes, and what cs_ba_load makes of them.
What the tables MEAN is the GPU suite's business (tests/test_ba_gpu.py holds the linear system they produce to the oracle at full C4 size)."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_INC = "/opt/rocm/include"

SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from cube_slam_wu_amd import capi, synth_ba
pr = synth_ba.make_problem(n_cams=200, n_points=20000, n_cuboids=50, seed=42)
P = capi.ba_from_dict(pr)
print("ATONCE", P.reduced_size(), P.schur_layout(), P.structure_digest())
P.close()
# the same graph with its points ordered by the first camera that sees them, set up for the first 196 cameras and grown by four frames
nc = len(pr["cams"])
fp = np.full(len(pr["points"]), nc); np.minimum.at(fp, pr["e_pt"], pr["e_cam"])
order = np.argsort(fp, kind="stable"); rank = np.empty_like(order); rank[order] = np.arange(len(order))
fp = fp[order]; ept = rank[pr["e_pt"]]
pts, ptf = pr["points"][order], pr["pt_fixed"][order]
T0 = nc - 4
def edges(sel_p, sel_c, sel_o):
    return ((ept[sel_p], pr["e_cam"][sel_p], pr["e_uv"][sel_p], pr["e_info"][sel_p], pr["e_intr"][sel_p], pr["e_huber"][sel_p]),
            (pr["ce_cam"][sel_c], pr["ce_cub"][sel_c], pr["ce_meas"][sel_c], pr["ce_info"][sel_c]),
            (pr["oe_i"][sel_o], pr["oe_j"][sel_o], pr["oe_meas"][sel_o], pr["oe_info"][sel_o]))
omax = np.maximum(pr["oe_i"], pr["oe_j"])
n_p = int((fp < T0).sum())
G = capi.BaProblem(pr["cams"][:T0], pr["cam_fixed"][:T0], pr["cuboids"], pr["cub_fixed"], pts[:n_p], ptf[:n_p])
# (2 %% of the early cameras' projection edges are held back and arrive with the last frame: appended edges whose camera sorts BEFORE the
# landmark's existing ones -- the grown graph's camera lists are extended, not rebuilt, and must still come out sorted)
late = (np.random.default_rng(1).random(len(ept)) < 0.02) & (pr["e_cam"] < T0)
ep, ec, eo = edges((pr["e_cam"] < T0) & ~late, pr["ce_cam"] < T0, omax < T0)
G.set_edges_proj(*ep); G.set_edges_cuboid(*ec); G.set_edges_odom(*eo)
G.structure_digest()
parts = [(ep, ec, eo)]
for t in range(T0, nc):
    n_p2 = int((fp < t + 1).sum())
    G.append_vertices(pr["cams"][t:t + 1], pr["cam_fixed"][t:t + 1], None, None, pts[n_p:n_p2], ptf[n_p:n_p2])
    ep, ec, eo = edges((pr["e_cam"] == t) | (late if t == nc - 1 else False), pr["ce_cam"] == t, omax == t)
    G.append_edges_proj(*ep); G.append_edges_cuboid(*ec); G.append_edges_odom(*eo)
    parts.append((ep, ec, eo)); n_p = n_p2
    G.structure_digest()                      # (the structure phase after every frame, as optimize() would run it)
print("GROWN", G.reduced_size(), G.schur_layout(), G.structure_digest())
G.close()
cat = lambda k, q: np.concatenate([p[k][q] for p in parts])
H = capi.BaProblem(pr["cams"], pr["cam_fixed"], pr["cuboids"], pr["cub_fixed"], pts, ptf)
H.set_edges_proj(*[cat(0, q) for q in range(6)]); H.set_edges_cuboid(*[cat(1, q) for q in range(4)]); H.set_edges_odom(*[cat(2, q) for q in range(4)])
print("SAMEORDER", H.reduced_size(), H.schur_layout(), H.structure_digest())
H.close()
"""

# the pose-edge classes of one small graph (48 EdgeSE3Cuboid, 48 EdgeSE3CuboidProj, 11 odometry edges): handle A set at once, handle B from a prefix
# of each class, one structure phase, and the rest appended (the CuboidProj tail is a single edge); the same kernels, levels and switch on both
EDGE_SCRIPT = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
from cube_slam_wu_amd import capi, synth_ba
out = %(out)r
pr = synth_ba.make_problem(n_cams=12, n_points=300, n_cuboids=4, bbox_edges=True)
CLS = ((capi.EDGE_CUBOID, ("ce_cam", "ce_cub", "ce_meas", "ce_info"), 20), (capi.EDGE_CUBOID_PROJ, ("pe_cam", "pe_cub", "pe_meas", "pe_info", "pe_K"), 47),
       (capi.EDGE_ODOM, ("oe_i", "oe_j", "oe_meas", "oe_info"), 5))
assert [len(pr[k[0]]) for _, k, _ in CLS] == [48, 48, 11]
def handle(grown):
    P = capi.BaProblem(pr["cams"], pr["cam_fixed"], pr["cuboids"], pr["cub_fixed"], pr["points"], pr["pt_fixed"])
    P.set_edges_proj(pr["e_pt"], pr["e_cam"], pr["e_uv"], pr["e_info"], pr["e_intr"], pr["e_huber"])
    sets = (P.set_edges_cuboid, P.set_edges_cuboid_proj, P.set_edges_odom)
    for f, (_, keys, cut) in zip(sets, CLS):
        f(*[pr[k][:cut] if grown else pr[k] for k in keys])
    if grown:
        P.structure_digest()
        for f, (_, keys, cut) in zip((P.append_edges_cuboid, P.append_edges_cuboid_proj, P.append_edges_odom), CLS):
            f(*[pr[k][cut:] for k in keys])
    for cls, keys, _ in CLS:
        n = len(pr[keys[0]])
        P.set_robust_kernels(cls, np.arange(n) %% 7, 0.5 + 0.25 * (np.arange(n) %% 5))
        P.set_edge_levels(cls, np.arange(n) %% 3 == 1)
    P.set_kernels_enabled(capi.EDGE_ODOM, False)
    return P
for tag, grown in (("A", False), ("B", True)):
    P = handle(grown)
    print(tag, P.structure_digest())
    P.dump(out + "/" + tag + ".bin")
    P.close()
L = capi.BaProblem.load(out + "/A.bin", (len(pr["cams"]), len(pr["cuboids"]), len(pr["points"]), len(pr["e_pt"])))
print("L", L.structure_digest())
L.dump(out + "/L.bin")
L.close()
"""


def _shim(tmp_path):
    if shutil.which("g++") is None or not os.path.exists(os.path.join(HIP_INC, "hip", "hip_runtime_api.h")):
        pytest.skip("needs g++ and the HIP headers")
    shim = tmp_path / "nohip_shim.so"
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-I" + HIP_INC, os.path.join(ROOT, "tools", "hostonly", "nohip_shim.cpp"), "-o", str(shim)])
    return shim


def _run(shim, threads, script=SCRIPT, tags=("ATONCE", "GROWN", "SAMEORDER"), **fmt):
    # (kernels do not run under the shim: the tables go up by per-table copies; whatever the environment already preloads stays preloaded)
    env = dict(os.environ, LD_PRELOAD=":".join(p for p in (str(shim), os.environ.get("LD_PRELOAD", "")) if p), CS_BA_UPLOAD_KERNEL="0")
    env.pop("CS_BA_STRUCT_THREADS", None)
    if threads:
        env["CS_BA_STRUCT_THREADS"] = str(threads)
    out = subprocess.run([sys.executable, "-c", script % dict(fmt, root=ROOT)], capture_output=True, text=True, timeout=900, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = {l.split(" ", 1)[0]: l.split(" ", 1)[1] for l in out.stdout.splitlines() if l.split(" ", 1)[0] in tags}
    assert set(lines) == set(tags), out.stdout[-2000:]
    return lines


def test_structure_tables_threaded_equal_sequential_and_grown_equals_at_once(tmp_path):
    shim = _shim(tmp_path)
    threaded, sequential = _run(shim, 0), _run(shim, 1)
    assert threaded == sequential                                   # every table of all three builds, threads or not
    assert threaded["GROWN"] == threaded["SAMEORDER"]               # appended frame by frame = set up at once (same vertex and edge order)
    assert "None" not in threaded["ATONCE"]


def test_pose_edge_classes_set_at_once_equal_grown_in_tables_dump_and_load(tmp_path):
    """cs_ba_set_edges_{cuboid,cuboid_proj,odom} against a prefix set, one structure phase, and cs_ba_append_edges_* of the rest (EDGE_SCRIPT): the
    same index tables, byte-identical dumps -- kernels of all seven kinds, levels and the odometry kernels' switch included -- and a load of the dump that
    dumps the same bytes again and builds the same tables."""
    lines = _run(_shim(tmp_path), 0, EDGE_SCRIPT, ("A", "B", "L"), out=str(tmp_path))
    dumps = {t: (tmp_path / (t + ".bin")).read_bytes() for t in ("A", "B", "L")}
    assert len(dumps["A"]) > 48 * 8 * (10 + 81 + 4 + 16 + 9)          # (the payload of the cuboid classes is in there)
    assert lines["A"] == lines["B"] and "None" not in lines["A"]
    assert dumps["A"] == dumps["B"]
    assert dumps["L"] == dumps["A"] and lines["L"] == lines["A"]


def test_pose_edge_class_record_stand_alone():
    """tools/microbench/edge_class_check.cpp: the record behind the six pose-edge entry points on its own -- set, append, append with kernels present,
    set again, bad arguments -- for the three classes' dimensions."""
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    os.makedirs(os.path.join(ROOT, "build_tmp"), exist_ok=True)
    exe = os.path.join(ROOT, "build_tmp", "edge_class_check")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-Wall", os.path.join(ROOT, "tools", "microbench", "edge_class_check.cpp"), "-o", exe])
    assert subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.strip() == "edge_class_check: ok"
