"""Time of the batched guided ORB matcher (cs_orb_search_set_frames / cs_orb_search_run) on one keyframe's LocalMapping::SearchInNeighbors,
beside the host build of the same header (tools/hostonly/orb_search_host_check.cpp, g++ -O2, one core: cs::orb_pack_frame and
cs::orb_search_job_serial) over the same batch.

    python tools/orb_search_quick.py [--frames 20] [--keypoints 2000] [--queries 1000] [--repeat 21] [--out profiles/orb_search_quick.txt]

The work: --frames neighbour keyframes of --keypoints keypoints each in the resident set; the first call fuses about --queries map points
of the current keyframe into every neighbour (Fuse's flags, th = 3, TH_LOW), the second call, over the SAME resident frames, fuses as
many points per neighbour in the other direction (modelled as a second, different set of jobs over the same frames).  It prints, and
writes to --out, the median and the range (min .. max) over --repeat rounds, after two warm-up rounds, of set_frames (host clock: checks,
the grid build while packing, one upload), of each run's kernel time (hipEvents on the handle's stream) and whole call (host clock:
checking, packing, the two copies and the kernel), the traffic the walk causes (from the inspection outputs: keypoint records read,
descriptors read), and the serial worker's grid build and pass; the two must hand out the same results."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cube_slam_wu_amd import capi, synth_orb_search as so  # noqa: E402


def host_pass(exe, batch, p, repeat):
    """-> (the host check's `time` line, its status / best_idx / best_dist / level rows)."""
    with tempfile.TemporaryDirectory() as d:
        dump = os.path.join(d, "batch.txt")
        so.write_dump(dump, batch, [p.min_dist_factor, p.max_dist_factor, p.view_cos, p.chi2_mono, p.chi2_stereo, p.grid_cols, p.grid_rows])
        timed = subprocess.check_output([exe, "time", str(repeat), dump], text=True).splitlines()[0]
        rows = [[int(x) for x in line.split()[2:6]] for line in subprocess.check_output([exe, "run", dump], text=True).splitlines() if line.startswith("q ")]
        return timed, np.array(rows).reshape(-1, 4)


def stats(v):
    return "%.4f ms (%.4f .. %.4f)" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--repeat", type=int, default=21)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orb_search_quick.txt"))
    a = ap.parse_args()
    if capi.lib().cs_device_count() < 1:
        raise SystemExit("orb_search_quick needs a HIP device")
    tmp = tempfile.TemporaryDirectory()
    exe = os.path.join(tmp.name, "orb_search_host_check")
    try:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", os.path.join(ROOT, "tools", "hostonly", "orb_search_host_check.cpp"), "-o", exe])
    except (OSError, subprocess.CalledProcessError):
        exe = None
    p = capi.orb_search_default_params()
    jobs = [dict(frame=f, count=a.queries, flags=so.FUSE, th=3.0, max_hamming=so.TH_LOW) for f in range(a.frames)] * 2
    both = so.synth_orb_search([a.keypoints] * a.frames, jobs, 1, n_points=max(2 * a.queries, a.keypoints), families=("good", "good", "good", "far", "good", "alone", "good", "view"))
    there, back = so.take_jobs(both, range(a.frames)), so.take_jobs(both, range(a.frames, 2 * a.frames))
    h = capi.OrbSearch()
    t_set, kern, host, wall = [], ([], []), ([], []), ([], [])
    for r in range(a.repeat + 2):                          # two warm-up rounds: code object, buffers of this size
        t0 = time.perf_counter()
        h.set_frames(both, p)
        t1 = time.perf_counter()
        outs = []
        for k, b in enumerate((there, back)):
            t2 = time.perf_counter()
            outs.append(h.run(b))
            t3 = time.perf_counter()
            if r >= 2:
                t = h.timing()
                kern[k].append(t["kernel_ms"]); host[k].append(t["host_ms"]); wall[k].append((t3 - t2) * 1e3)
        if r >= 2:
            t_set.append((t1 - t0) * 1e3)
    h.close()
    insp = capi.orb_search_inspect(both, p)
    Q = len(insp["status"])
    n_kp = int(both["kp_ptr"][-1])
    lines = ["orb_search_quick: SearchInNeighbors of one keyframe: %d resident frames x %d keypoints (64 x 48 grid), %d queries per job, Fuse's flags, th 3, both directions; median (min .. max) of %d rounds after 2 warm-up rounds"
             % (a.frames, a.keypoints, a.queries, a.repeat),
             "  set_frames (checks, grid build while packing, one upload of %.2f MB), python call: %s" % ((n_kp * (32 + 4 + 32) + a.frames * (64 * 48 + 1) * 4) / 1e6, stats(t_set))]
    for k, name in enumerate(("first direction ", "second direction")):
        kk = float(np.median(kern[k]))
        lines.append("  %s: kernel %s: %.2f ns per query   host call %s   python call %.3f ms" % (name, stats(kern[k]), kk * 1e6 / (Q / 2), stats(host[k]), np.median(wall[k])))
    walked = np.isin(insp["status"], (0, 6, 7))
    lines.append("  per query that reaches the walk (%d of %d): %.2f keypoints inside its window, %.2f descriptors read (32 bytes each); a frame's descriptors are %d bytes"
                 % (walked.sum(), Q, insp["n_window"][walked].mean(), insp["n_candidates"][walked].mean(), a.keypoints * 32))
    lines.append("  statuses OK / SKIPPED / BEHIND / OUT_OF_IMAGE / OUT_OF_RANGE / VIEW_ANGLE / NO_CANDIDATE / TOO_FAR %s" % np.bincount(insp["status"], minlength=8).tolist())
    if exe is None:
        lines.append("  host build of cs_orb_search.h: no figure recorded (no g++ here)")
    else:
        timed, rows = host_pass(exe, both, p, max(1, a.repeat // 3))
        same = np.array_equal(rows, np.stack([insp[k] for k in ("status", "best_idx", "best_dist", "level")], 1)) and all(
            np.array_equal(np.concatenate([outs[0][k], outs[1][k]]), insp[k]) for k in ("status", "best_idx", "best_dist", "level"))
        lines.append("  cs_orb_search.h with g++ -O2, both directions in one pass -- " + timed + ("; same results as the device" if same else "; RESULTS DIFFER FROM THE DEVICE'S"))
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
