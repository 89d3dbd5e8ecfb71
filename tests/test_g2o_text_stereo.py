"""The stereo edge tag of the graph driver's g2o text IO (examples/g2o_text.h), no GPU needed: a graph with both projection tags survives
`object_slam_main --g2o in out 0` -- three measurement values and the six entries of the 3 x 3 information's upper triangle per stereo edge,
bf through its CS_STEREO_BF state line, the stereo edges written behind the mono ones."""
import subprocess

import numpy as np

from test_g2o_text import _exe, _rows


def test_round_trip_of_a_graph_with_both_projection_tags(tmp_path):
    src = tmp_path / "in.g2o"
    src.write_text(
        "VERTEX_SE3:EXPMAP 1 0 0 0 0 0 0 1\nFIX 1\nVERTEX_SE3:EXPMAP 2 0.5 0 0 0 0 0 1\n"
        "VERTEX_XYZ 10 0.5 0.25 12\nVERTEX_XYZ 11 -1 0.5 20\n"
        "CS_INTRINSICS 700 710 600 180\nCS_ROBUST_HUBER 2.5\n"
        "EDGE_STEREO_SE3_PROJECT_XYZ:EXPMAP 10 1 629.1 194.8 597.0 1 0.1 0.2 2 0.3 3\n"      # before its CS_STEREO_BF line: dropped with a warning
        "CS_STEREO_BF 385.5\n"
        "EDGE_STEREO_SE3_PROJECT_XYZ:EXPMAP 10 2 600.1 194.9 568.0 1 0.1 0.2 2 0.3 3\n"
        "EDGE_SE3_PROJECT_XYZ:EXPMAP 11 1 565.0 197.7 1 0 1\n"
        "EDGE_STEREO_SE3_PROJECT_XYZ:EXPMAP 11 2 547.5 197.8 528.2 4 0 0 4 0 4\n"
        "EDGE_STEREO_SE3_PROJECT_XYZ:EXPMAP 11 7 547.5 197.8 528.2 4 0 0 4 0 4\n")
    out = subprocess.run([_exe(), "--g2o", str(src), str(tmp_path / "out.g2o"), "0"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "2 points, 1 camera-point edges, 2 stereo camera-point edges" in out.stdout
    assert "CS_STEREO_BF lines before the edges" in out.stderr and "edge EDGE_STEREO_SE3_PROJECT_XYZ:EXPMAP 11 7" in out.stderr
    rows = _rows(tmp_path / "out.g2o")
    edges = [r for r in rows if r[0].startswith(("EDGE", "CS_"))]
    assert [r[0] for r in edges] == ["CS_INTRINSICS", "CS_ROBUST_HUBER", "EDGE_SE3_PROJECT_XYZ:EXPMAP", "CS_STEREO_BF",
                                     "EDGE_STEREO_SE3_PROJECT_XYZ:EXPMAP", "EDGE_STEREO_SE3_PROJECT_XYZ:EXPMAP"]
    assert edges[3][1] == [385.5]
    assert edges[4][1] == [10, 2, 600.1, 194.9, 568.0, 1, 0.1, 0.2, 2, 0.3, 3] and len(edges[5][1]) == 11      # 2 ids + 3 + 6: no fourth measurement entry
    # and the written file reads back to the same file
    out2 = subprocess.run([_exe(), "--g2o", str(tmp_path / "out.g2o"), str(tmp_path / "out2.g2o"), "0"], capture_output=True, text=True, timeout=120)
    assert out2.returncode == 0 and open(tmp_path / "out.g2o").read() == open(tmp_path / "out2.g2o").read()
