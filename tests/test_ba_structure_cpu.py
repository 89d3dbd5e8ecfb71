"""The passes of the bundle adjustment's structure phase (cube_slam_wu_amd/csrc/ba_structure.h) WITHOUT a GPU and without the library:
tools/hostonly/ba_structure_check.cpp is built against the header alone with the host compiler, under the address and undefined-behaviour
sanitizers, and run.  On a graph of 9 cameras (two fixed), 60 landmarks seen by 0-6 cameras (shared camera sets, one landmark without an edge,
some fixed), 3 cuboids (one fixed, one camera with two edges to a cuboid) and 8 odometry edges it holds, with 1, 3 and 8 threads each,
  * the landmarks' camera lists to a stable sort of the edges by (landmark, camera) -- the two-level threaded grouping also with more ranges than
    landmarks, the grown path (a prefix plus appended edges, some sorting before their landmark's existing ones, and new landmarks) to the
    at-once lists, and a repeated (landmark, camera) pair to being reported;
  * the camera-set groups and their run boundaries to a stable sort by (number of cameras, camera list);
  * rcm_ordering to its properties: the columns pack exactly the free vertices (6 per camera, 9 per cuboid, eliminated cuboids behind n_red), bw
    is the bandwidth of adj, a chain comes out with the chain's bandwidth, the bit and the list form of the adjacency agree;
  * the point-major and camera-major edge orders to sorts by (column, camera id) and by camera, for one rank and for two;
  * the fused Schur schedule (segments, running tile / slot offsets, destination lists, per-camera slots, the eliminated cuboids' slots and
    their edges) and the pair-major schedule to stable sorts of the blocks they stand for;
  * the separator cut on a 60-camera chain to its conditions, and the three owner kinds to a linear scan over the cut.
That ba_host.cpp then uploads these tables unchanged is tests/test_ba_host_cpu.py's and the GPU suite's business."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_structure_passes_hold_their_definitions_stand_alone(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("needs g++")
    exe = tmp_path / "ba_structure_check"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           os.path.join(ROOT, "tools", "hostonly", "ba_structure_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.strip().splitlines()[-1] == "ba_structure_check: ok"
