#!/usr/bin/env python3
"""tests/golden/ba_edge_blocks.npz -- an exact-quotient pin for the three numeric-Jacobian edge classes of path B.

A from-scratch mpmath restatement (60 digits) of what the reference evaluates for EdgeSE3Cuboid, EdgeSE3CuboidProj and EdgeSE3Expmap,
written against the reference's sources only.  For the mathematics this script imports nothing from oracle/ or cube_slam_wu_amd/csrc
and consults neither (cube_slam_wu_amd.synth_ba is used as a workload helper for float64 pose products when the INPUTS are drawn; the
CPU oracle is run at the very end, only to measure ITS deviation from the values computed here).  Sources (paths below object_slam/):

  SE3Quat product / inverse / ctor  Thirdparty/g2o/g2o/types/se3quat.h:58-70, :110-134, :346-351 (normalizeRotation: w >= 0, unit)
  SE3Quat::log                      se3quat.h:230-267 (d > 0.99999: small-angle branch), se3_ops.hpp:28-48 (skew, deltaR)
  SE3Quat::exp                      se3quat.h:275-323 (theta < 0.00001: R = I + Omega + Omega^2, V = R; SE3Quat(Quaterniond(R), V upsilon))
  VertexSE3Expmap::oplusImpl        Thirdparty/g2o/g2o/types/types_six_dof_expmap.h:73-76 (exp(update) * estimate)
  EdgeSE3Expmap::computeError       types_six_dof_expmap.h:90-99 (log(C * T1 * T2^-1))
  cuboid::exp_update                include/object_slam/g2o_Object.h:57-63 (pose * exp(update[0:6]), scale + update[6:9]), :210-213
  cuboid::cube_log_error            g2o_Object.h:66-73
  cuboid::min_log_error             g2o_Object.h:76-101 (yaw -90, 0, 90, 180 degrees; minCoeff: first minimum, strict <)
  cuboid::rotate_cuboid             g2o_Object.h:104-114 (x/y half sizes swapped at +-90 degrees)
  projectOntoImageBbox              g2o_Object.h:154-197 (similarityTransform, compute3D_BoxCorner, projectOntoImageRect)
  EdgeSE3Cuboid::computeError       g2o_Object.h:250-259;  EdgeSE3CuboidProj::computeError  g2o_Object.h:279-290
  numeric Jacobian                  Thirdparty/g2o/g2o/core/base_binary_edge.hpp:130-205 (central differences, delta = 1e-9)
  quadratic form, robust kernels    base_binary_edge.hpp:54-120, core/robust_kernel_impl.cpp:78-162 (formed in float64 by
                                    tests/edge_blocks_ref.py from the e and J stored here)
Eigen's quaternion product, quaternion * vector, toRotationMatrix and Quaterniond(Matrix3d) are restated from the published algorithms.
No text of the reference is copied.

Per edge the script evaluates the error e and the EXACT central-difference quotient J[:, d] = (e(x + delta e_d) - e(x - delta e_d)) / 2 delta
with the reference's branch rules.  That quotient is the quantity g2o defines; at 60 digits it carries no cancellation noise, so in a
comparison the only noise is that of the side under test.  Every evaluation records the branches it took (log's small-angle / acos
branch, the winning yaw candidate, the extreme corners of the box); the script asserts that all perturbed evaluations of an edge take
the unperturbed one's -- an edge for which they do not has no well-defined quotient and is not a usable input.

Input families (each edge belongs to exactly one; the property that names the family is asserted below).  All classes: dense SPD
information A A^T + I scaled to the class's usual magnitude (condition <= 1e3, exactly symmetric), cameras of arbitrary orientation, a
quarter of the edges with a Huber / Cauchy / Tukey / DCS kernel whose width puts every other one in the outlier regime, per class two
edges with the first vertex fixed and two with the second.
  EdgeSE3Cuboid      generic; cand0 .. cand3 (that yaw candidate wins by > 1e-2 (1 + norm)); near_tie (lead within [1e-5, 5e-4] (1 + norm));
                     log_small (logged angle 1e-3, 3e-3), log_acos (6e-3, 1e-2)
  EdgeSE3CuboidProj  generic (depth 4 - 40 m, fx != fy, skew, every extreme corner leads by > 1e-3 px); off_image
  EdgeSE3Expmap      log_small, log_acos, moderate (0.1 - 1 rad), large (2.0 - 2.6 rad); translations up to 50 m; half the edges i > j
Left out on purpose, because the reference's result there rests on undefined or unspecified behaviour: an exact tie between yaw
candidates, a box corner at depth ~ 0, the log of an exact 180 degree rotation (0 / 0).

Run in the build container:  python tools/make_edge_golden.py
"""
import math
import os
import sys

import mpmath as mp
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

mp.mp.dps = 60
DELTA = mp.mpf(1e-9)                    # the double the reference steps by
OUT = os.path.join(ROOT, "tests", "golden", "ba_edge_blocks.npz")
NEAR_TIE_LEAD = (1e-5, 5e-4)
CLEAR_LEAD = 1e-2


# ---------------------------------------------------------------- SE(3) at 60 digits: a pose is (t[3], q[4] = x y z w)
def _v(a):
    return [mp.mpf(float(x)) for x in a]


def cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
            aw * bw - ax * bx - ay * by - az * bz]


def qrot(q, v):
    """Eigen's quaternion * vector: v + w (2 qv x v) + qv x (2 qv x v) -- the form it keeps for a quaternion that is not exactly unit."""
    uv = [2 * x for x in cross(q[:3], v)]
    c2 = cross(q[:3], uv)
    return [v[i] + q[3] * uv[i] + c2[i] for i in range(3)]


def qnormalized(q):
    """normalizeRotation (se3quat.h:346-351)."""
    if q[3] < 0:
        q = [-x for x in q]
    n = mp.sqrt(sum(x * x for x in q))
    return [x / n for x in q]


def pmul(a, b):
    return ([a[0][i] + r for i, r in enumerate(qrot(a[1], b[0]))], qnormalized(qmul(a[1], b[1])))


def pinv(a):
    qc = [-a[1][0], -a[1][1], -a[1][2], a[1][3]]
    return (qrot(qc, [-x for x in a[0]]), qc)


def rotmat(q):
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def quat_from_R(R):
    """Eigen's Quaterniond(Matrix3d) -- also for the not quite orthonormal I + Omega + Omega^2 of exp's small-angle branch."""
    t = R[0][0] + R[1][1] + R[2][2]
    if t > 0:
        s = mp.sqrt(t + 1)
        w = s / 2
        s = 1 / (2 * s)
        return [(R[2][1] - R[1][2]) * s, (R[0][2] - R[2][0]) * s, (R[1][0] - R[0][1]) * s, w]
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    s = mp.sqrt(R[i][i] - R[j][j] - R[k][k] + 1)
    q = [mp.mpf(0)] * 4
    q[i] = s / 2
    s = 1 / (2 * s)
    q[3] = (R[k][j] - R[j][k]) * s
    q[j] = (R[j][i] + R[i][j]) * s
    q[k] = (R[k][i] + R[i][k]) * s
    return q


def skew(v):
    return [[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]]


def mm(A, B):
    return [[sum(A[i][k] * B[k][j] for k in range(3)) for j in range(3)] for i in range(3)]


def mv(A, v):
    return [sum(A[i][k] * v[k] for k in range(3)) for i in range(3)]


def plog(T, trace, formula=None):
    """SE3Quat::log -> [omega, upsilon].  formula: None = the reference's branch rule, "small" / "acos" = that formula regardless."""
    R = rotmat(T[1])
    d = (R[0][0] + R[1][1] + R[2][2] - 1) / 2
    dR = [R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]]
    small = d > mp.mpf(0.99999)
    trace.append(("log", bool(small), mp.acos(d)))
    if formula is not None:
        small = formula == "small"
    if small:
        omega = [x / 2 for x in dR]
        c = mp.mpf(1) / 12
    else:
        theta = mp.acos(d)
        omega = [theta / (2 * mp.sqrt(1 - d * d)) * x for x in dR]
        c = (1 - theta / (2 * mp.tan(theta / 2))) / (theta * theta)
    Om = skew(omega)
    Om2 = mm(Om, Om)
    Vinv = [[(1 if i == j else 0) - Om[i][j] / 2 + c * Om2[i][j] for j in range(3)] for i in range(3)]
    return omega + mv(Vinv, T[0])


def pexp(u):
    omega, ups = u[:3], u[3:6]
    theta = mp.sqrt(sum(x * x for x in omega))
    Om = skew(omega)
    Om2 = mm(Om, Om)
    if theta < mp.mpf(0.00001):
        R = [[(1 if i == j else 0) + Om[i][j] + Om2[i][j] for j in range(3)] for i in range(3)]
        V = R
    else:
        a, b, c = mp.sin(theta) / theta, (1 - mp.cos(theta)) / (theta * theta), (theta - mp.sin(theta)) / theta ** 3
        R = [[(1 if i == j else 0) + a * Om[i][j] + b * Om2[i][j] for j in range(3)] for i in range(3)]
        V = [[(1 if i == j else 0) + b * Om[i][j] + c * Om2[i][j] for j in range(3)] for i in range(3)]
    return (mv(V, ups), qnormalized(quat_from_R(R)))


def pose_in(v7, normalize):
    """A pose from its float64 7-vector x y z qx qy qz qw: SE3Quat(Vector7d) normalises (se3quat.h:67-70), fromVector does not (:157-160)."""
    q = _v(v7[3:7])
    return (_v(v7[:3]), qnormalized(q) if normalize else q)


def cam_oplus(T, u):
    return pmul(pexp(u), T)


def cub_oplus(c, u):
    return (pmul(c[0], pexp(u[:6])), [c[1][i] + u[6 + i] for i in range(3)])


def cube_in(v10):
    return (pose_in(v10[:7], False), _v(v10[7:10]))


# ---------------------------------------------------------------- the three errors
# rotate_cuboid's quaternions: cos / sin of half of angle * M_PI / 2 are doubles in the reference (the C library's values of double arguments)
YAW = [a * math.pi / 2.0 for a in (-1.0, 0.0, 1.0, 2.0)]
YAW_ROT = [([mp.mpf(0)] * 3, qnormalized([mp.mpf(0), mp.mpf(0), mp.mpf(math.sin(a * 0.5)), mp.mpf(math.cos(a * 0.5))])) for a in YAW]
YAW_SWAP = [a == math.pi / 2.0 or a == -math.pi / 2.0 or a == 3 * math.pi / 2.0 for a in YAW]


def cube_log_error(self, other, trace, formula=None):
    return plog(pmul(pinv(other[0]), self[0]), trace, formula) + [self[1][i] - other[1][i] for i in range(3)]


def cuboid_edge_error(T, cube, meas, trace, pick=None, formula=None, norms_out=None):
    """EdgeSE3Cuboid::computeError.  pick: return that yaw candidate's error instead of the winner's (the runner-up guard)."""
    esti = (pmul(pinv(T), meas[0]), meas[1])
    errs, norms, traces = [], [], []
    for i in range(4):
        s = esti[1]
        rc = (pmul(esti[0], YAW_ROT[i]), [s[1], s[0], s[2]] if YAW_SWAP[i] else list(s))
        tr = []
        e = cube_log_error(cube, rc, tr, formula)
        errs.append(e); traces.append(tr)
        norms.append(mp.sqrt(sum(x * x for x in e)))
    m = 0
    for i in range(1, 4):
        if norms[i] < norms[m]:
            m = i
    if norms_out is not None:
        norms_out[:] = norms
    use = m if pick is None else pick
    trace.append(("win", m))
    trace.extend(traces[use])
    return errs[use]


CORNERS = [(1, 1, -1), (1, -1, -1), (-1, -1, -1), (-1, 1, -1), (1, 1, 1), (1, -1, 1), (-1, -1, 1), (-1, 1, 1)]     # the columns of compute3D_BoxCorner's matrix


def box_pixels(T, cube, K):
    Ro, Rc = rotmat(cube[0][1]), rotmat(T[1])
    uv, depth = [], []
    for c in CORNERS:
        Xw = [sum(Ro[i][j] * cube[1][j] * c[j] for j in range(3)) + cube[0][0][i] for i in range(3)]
        Xc = [sum(Rc[i][j] * Xw[j] for j in range(3)) + T[0][i] for i in range(3)]
        p = mv(K, Xc)
        uv.append((p[0] / p[2], p[1] / p[2])); depth.append(Xc[2])
    return uv, depth


def _argext(vals, sign):
    m = 0
    for i in range(1, len(vals)):
        if (vals[i] > vals[m]) if sign > 0 else (vals[i] < vals[m]):
            m = i
    return m


def cuboid_proj_error(T, cube, K, meas4, trace):
    uv, _ = box_pixels(T, cube, K)
    us, vs = [p[0] for p in uv], [p[1] for p in uv]
    ix = (_argext(us, -1), _argext(vs, -1), _argext(us, 1), _argext(vs, 1))
    trace.append(("ext", ix))
    x1, y1, x2, y2 = us[ix[0]], vs[ix[1]], us[ix[2]], vs[ix[3]]
    return [(x2 + x1) / 2 - meas4[0], (y2 + y1) / 2 - meas4[1], (x2 - x1) - meas4[2], (y2 - y1) - meas4[3]]


def odom_edge_error(T1, T2, C, trace, formula=None):
    return plog(pmul(pmul(C, T1), pinv(T2)), trace, formula)


def _branches(trace):
    """The branch decisions of an evaluation (without the angles recorded next to them)."""
    return [t[:2] for t in trace]


def numeric_jacobian(err, xa, xb, oplus_a, oplus_b, NA, NB):
    """(e, J as D x (NA + NB), trace of the unperturbed evaluation); asserts that no perturbed evaluation takes another branch."""
    tr0 = []
    e0 = err(xa, xb, tr0)
    cols = []
    for side, N in ((0, NA), (1, NB)):
        for d in range(N):
            ev = []
            for s in (DELTA, -DELTA):
                u = [mp.mpf(0)] * N
                u[d] = s
                tr = []
                ev.append(err(oplus_a(xa, u), xb, tr) if side == 0 else err(xa, oplus_b(xb, u), tr))
                assert _branches(tr) == _branches(tr0), "a perturbed evaluation changes branch: not a usable input"
            cols.append([(p - m) / (2 * DELTA) for p, m in zip(ev[0], ev[1])])
    D = len(e0)
    return e0, [[cols[c][r] for c in range(NA + NB)] for r in range(D)], tr0


def _f(x):
    return np.array([[float(v) for v in row] for row in x]) if isinstance(x[0], list) else np.array([float(v) for v in x])


def evaluate_edge(fx, cls, k, pick=None, formula=None):
    """e, J (float64 roundings of the 60-digit values) and details of edge k of a class, from the inputs stored in the fixture dict fx."""
    Ta = pose_in(fx["cams"][fx[cls + "/a"][k]], True)
    info = {}
    if cls == "odo":
        Tb, C = pose_in(fx["cams"][fx["odo/b"][k]], True), pose_in(fx["odo/meas"][k], True)
        e, J, tr = numeric_jacobian(lambda a, b, t: odom_edge_error(a, b, C, t, formula), Ta, Tb, cam_oplus, cam_oplus, 6, 6)
        info["angle"] = float(tr[0][2])
    elif cls == "cub":
        cube, meas = cube_in(fx["cuboids"][fx["cub/b"][k]]), cube_in(fx["cub/meas"][k])
        norms = [None] * 4
        cuboid_edge_error(Ta, cube, meas, [], norms_out=norms)
        e, J, tr = numeric_jacobian(lambda a, b, t: cuboid_edge_error(a, b, meas, t, pick, formula), Ta, cube, cam_oplus, cub_oplus, 6, 9)
        order = sorted(range(4), key=lambda i: (norms[i], i))
        info.update(win=order[0], runner=order[1], lead=float((norms[order[1]] - norms[order[0]]) / (1 + norms[order[0]])), angle=float(tr[1][2]))
        assert tr[0] == ("win", order[0])
    else:
        cube, K, m4 = cube_in(fx["cuboids"][fx["box/b"][k]]), [_v(r) for r in fx["box/K"][k].reshape(3, 3)], _v(fx["box/meas"][k])
        e, J, tr = numeric_jacobian(lambda a, b, t: cuboid_proj_error(a, b, K, m4, t), Ta, cube, cam_oplus, cub_oplus, 6, 9)
        uv, depth = box_pixels(Ta, cube, K)
        lead = []
        for axis, sign in ((0, -1), (1, -1), (0, 1), (1, 1)):
            vals = sorted(float(p[axis]) * sign for p in uv)
            lead.append(vals[-1] - vals[-2])
        info.update(lead_px=np.array(lead), depth=np.array([float(z) for z in depth]), uv=np.array([[float(p[0]), float(p[1])] for p in uv]))
    return _f(e), _f(J), info


# ---------------------------------------------------------------- inputs (float64, numpy)
IMG_W, IMG_H = 640.0, 480.0


def _unit(v):
    return v / np.linalg.norm(v)


def _axis_angle_pose(rng, angle, trans_sigma):
    ax = _unit(rng.normal(size=3))
    return np.concatenate([rng.normal(0, trans_sigma, 3), np.sin(angle / 2) * ax, [np.cos(angle / 2)]])


def _rz(a):
    return np.array([0, 0, 0, 0, 0, np.sin(a / 2), np.cos(a / 2)])


def _spd(rng, D, scale):
    A = rng.normal(size=(D, D))
    M = A @ A.T + np.eye(D)
    M = 0.5 * (M + M.T)
    M *= scale / np.mean(np.diag(M))
    assert np.array_equal(M, M.T) and np.linalg.cond(M) <= 1e3
    return M.ravel()


def draw_pool(rng):
    from scipy.spatial.transform import Rotation
    from cube_slam_wu_amd import synth_ba as S
    NC, NO = 14, 12
    cams = np.zeros((NC, 7))
    for c in range(NC):
        pos = _unit(rng.normal(size=3)) * rng.uniform(8, 35)
        aim = rng.uniform(-4, 4, 3)
        z = _unit(aim - pos)
        x = _unit(np.cross(z, rng.normal(size=3)))
        if c >= 8:                       # aimed past the cuboids, by about the half field of view: boxes that leave the image
            z = _unit(z + math.tan(math.radians(rng.uniform(20, 30))) * x)
            x = _unit(np.cross(z, rng.normal(size=3)))
        y = np.cross(z, x)
        q = Rotation.from_matrix(np.stack([x, y, z], 1)).as_quat()
        cams[c] = S.pose_inv(np.concatenate([pos, q if q[3] >= 0 else -q]))
        if cams[c, 6] < 0:
            cams[c, 3:] *= -1
    cubs = np.zeros((NO, 10))
    for o in range(NO):
        q = Rotation.from_euler("ZYX", [rng.uniform(-np.pi, np.pi), rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5)]).as_quat()
        half = np.array([rng.uniform(1.5, 2.4), rng.uniform(0.7, 1.0), rng.uniform(0.5, 0.76)])
        if o >= 9:                       # near-square footprints for the near ties
            half[0] = rng.uniform(0.8, 1.2)
            half[1] = half[0] + rng.uniform(-0.01, 0.01)
        cubs[o] = np.concatenate([rng.uniform(-5, 5, 3), q if q[3] >= 0 else -q, half])
    cam_fixed, cub_fixed = np.zeros(NC, np.int32), np.zeros(NO, np.int32)
    cam_fixed[0] = cub_fixed[0] = 1
    return cams, cam_fixed, cubs, cub_fixed


def _cub_meas(S, cam7, cub10, noise7, off, swap, scale_noise):
    local = S.pose_mul(cam7, cub10[:7])
    pose = S.pose_mul(S.pose_mul(local, noise7), _rz(off))
    half = cub10[7:10].copy()
    if swap:
        half[[0, 1]] = half[[1, 0]]
    return np.concatenate([pose, half + scale_noise])


def draw_cuboid_edges(rng, fx):
    from cube_slam_wu_amd import synth_ba as S
    plan = [("generic", 0, 1), ("generic", 0, 2), ("generic", 1, 0), ("generic", 2, 0)]      # first / second vertex fixed
    plan += [("generic", int(rng.integers(1, 14)), int(rng.integers(1, 9))) for _ in range(4)]
    for i in range(4):
        plan += [("cand%d" % i, int(rng.integers(1, 14)), int(rng.integers(1, 9))) for _ in range(6)]
    plan += [("near_tie", int(rng.integers(1, 14)), 9 + j % 3) for j in range(8)]
    plan += [("log_small", int(rng.integers(1, 14)), int(rng.integers(1, 9))) for _ in range(6)]
    plan += [("log_acos", int(rng.integers(1, 14)), int(rng.integers(1, 9))) for _ in range(6)]
    n = len(plan)
    fx["cub/a"] = np.array([p[1] for p in plan], np.int32)
    fx["cub/b"] = np.array([p[2] for p in plan], np.int32)
    fx["cub/family"] = np.array([p[0] for p in plan])
    fx["cub/meas"] = np.zeros((n, 10))
    fx["cub/info"] = np.stack([_spd(rng, 9, (2 * rng.uniform(0.5, 1.0)) ** 2) for _ in range(n)])
    small_i = acos_i = tie_i = 0
    for k, (fam, c, o) in enumerate(plan):
        cam7, cub10 = fx["cams"][c], fx["cuboids"][o]
        noise = S.small_pose(rng, 1, 0.05, 0.05)[0]           # as synth_ba draws a cuboid observation
        sn = rng.normal(0, 0.05, 3)
        if fam == "generic":
            fx["cub/meas"][k] = _cub_meas(S, cam7, cub10, noise, 0.0, False, sn)
        elif fam.startswith("cand"):
            i = int(fam[4])
            fx["cub/meas"][k] = _cub_meas(S, cam7, cub10, noise, -YAW[i], YAW_SWAP[i], sn)
        elif fam in ("log_small", "log_acos"):
            if fam == "log_small":
                ang = (1e-3, 3e-3)[small_i % 2]; small_i += 1
            else:
                ang = (6e-3, 1e-2)[acos_i % 2]; acos_i += 1
            fx["cub/meas"][k] = _cub_meas(S, cam7, cub10, _axis_angle_pose(rng, ang, 0.05), 0.0, False, sn)
        else:
            # near tie between candidates i and i + 1: the measurement's yaw offset runs from candidate i's (-YAW[i]) a quarter turn on;
            # the tie is found by bisection on the exact norms, then left by the offset that gives the wanted lead
            i = tie_i % 4; tie_i += 1
            j = (i + 1) % 4
            target = math.exp(rng.uniform(math.log(3e-5), math.log(3e-4)))

            def gap(s):
                m = _cub_meas(S, cam7, cub10, noise, -YAW[i] - s * math.pi / 2, False, sn)
                norms = [None] * 4
                cuboid_edge_error(pose_in(cam7, True), cube_in(cub10), cube_in(m), [], norms_out=norms)
                return m, float(norms[j] - norms[i]), float(1 + min(norms))
            lo, hi = 0.2, 0.8
            assert gap(lo)[1] > 0 > gap(hi)[1]
            for _ in range(50):
                mid = 0.5 * (lo + hi)
                if gap(mid)[1] > 0:
                    lo = mid
                else:
                    hi = mid
            side = 1 if (tie_i - 1) // 4 % 2 == 0 else -1     # candidate i or candidate i + 1 ends up in front: every candidate wins twice
            step = 1e-4
            for _ in range(6):
                m, g, one_n = gap(lo - side * step)
                step *= target / (abs(g) / one_n)
            fx["cub/meas"][k] = m


def draw_box_edges(rng, fx):
    NC, NO = len(fx["cams"]), len(fx["cuboids"])
    cand = {"generic": [], "off_image": []}
    Ks = {}
    for c in range(NC):
        for o in range(NO):
            if c == 0 and o == 0:
                continue
            fxl = rng.uniform(450, 750)
            K = np.array([[fxl, rng.choice([-1, 1]) * rng.uniform(0.5, 3.0), IMG_W / 2 + rng.uniform(-15, 15)],
                          [0, fxl * rng.choice([rng.uniform(0.85, 0.95), rng.uniform(1.05, 1.15)]), IMG_H / 2 + rng.uniform(-15, 15)], [0, 0, 1.0]])
            uv, depth = box_pixels(pose_in(fx["cams"][c], True), cube_in(fx["cuboids"][o]), [_v(r) for r in K])
            uv, depth = np.array([[float(p[0]), float(p[1])] for p in uv]), np.array([float(z) for z in depth])
            inside = (uv[:, 0] >= 0) & (uv[:, 0] < IMG_W) & (uv[:, 1] >= 0) & (uv[:, 1] < IMG_H)
            Ks[(c, o)] = K
            if depth.min() >= 4 and depth.max() <= 40 and inside.all():
                cand["generic"].append((c, o))
            elif depth.min() >= 2 and depth.max() <= 40 and inside.any() and not inside.all():
                cand["off_image"].append((c, o))
    gen, off = cand["generic"], cand["off_image"]
    fixed_first = [p for p in gen if p[0] == 0][:2]
    fixed_second = [p for p in gen if p[1] == 0][:2]
    assert len(fixed_first) == 2 and len(fixed_second) == 2, "the fixed camera / cuboid see too little"
    rest = [p for p in gen if p[0] != 0 and p[1] != 0]
    rest = [rest[i] for i in rng.permutation(len(rest))[:32]]
    offs = [p for p in off if p[0] != 0 and p[1] != 0]
    offs = [offs[i] for i in rng.permutation(len(offs))[:10]]
    assert len(rest) == 32 and len(offs) == 10, "too few usable camera / cuboid pairs: %d generic, %d off-image" % (len(rest), len(offs))
    plan = [("generic",) + p for p in fixed_first + fixed_second + rest] + [("off_image",) + p for p in offs]
    n = len(plan)
    fx["box/a"] = np.array([p[1] for p in plan], np.int32)
    fx["box/b"] = np.array([p[2] for p in plan], np.int32)
    fx["box/family"] = np.array([p[0] for p in plan])
    fx["box/K"] = np.stack([Ks[(p[1], p[2])].ravel() for p in plan])
    fx["box/info"] = np.stack([_spd(rng, 4, 0.25) for _ in range(n)])
    fx["box/meas"] = np.zeros((n, 4))
    for k, (_, c, o) in enumerate(plan):
        z = [mp.mpf(0)] * 4
        e = cuboid_proj_error(pose_in(fx["cams"][c], True), cube_in(fx["cuboids"][o]), [_v(r) for r in Ks[(c, o)]], z, [])
        fx["box/meas"][k] = np.array([float(v) for v in e]) + rng.normal(0, 2.0, 4)     # the detection noise synth_ba draws


def draw_odom_edges(rng, fx):
    from cube_slam_wu_amd import synth_ba as S
    NC = len(fx["cams"])
    fams = ["moderate"] * 4 + ["log_small"] * 6 + ["log_acos"] * 6 + ["moderate"] * 10 + ["large"] * 12
    pairs = [(0, 3), (0, 7), (5, 0), (9, 0)]                 # first / second vertex fixed
    while len(pairs) < len(fams):
        i, j = (int(v) for v in rng.choice(np.arange(1, NC), 2, replace=False))
        pairs.append((i, j))
    n = len(fams)
    fx["odo/a"] = np.array([p[0] for p in pairs], np.int32)
    fx["odo/b"] = np.array([p[1] for p in pairs], np.int32)
    fx["odo/family"] = np.array(fams)
    fx["odo/info"] = np.stack([_spd(rng, 6, 1.0) for _ in range(n)])
    fx["odo/meas"] = np.zeros((n, 7))
    cnt = {"log_small": 0, "log_acos": 0}
    for k, fam in enumerate(fams):
        if fam in cnt:
            ang = {"log_small": (1e-3, 3e-3), "log_acos": (6e-3, 1e-2)}[fam][cnt[fam] % 2]; cnt[fam] += 1
            E = _axis_angle_pose(rng, ang, 0.01)
        elif fam == "moderate":
            E = _axis_angle_pose(rng, rng.uniform(0.1, 1.0), 0.3)
        else:
            E = _axis_angle_pose(rng, rng.uniform(2.0, 2.6), 0.3)
        T1, T2 = fx["cams"][pairs[k][0]], fx["cams"][pairs[k][1]]
        fx["odo/meas"][k] = S.pose_mul(E, S.pose_mul(T2, S.pose_inv(T1)))       # error = log(C T1 T2^-1) = log(E)


def draw_kernels(fx, cls):
    """Every fourth edge of a class gets a kernel, the kinds in turn, the widths alternately above and below the edge's chi."""
    import edge_blocks_ref as EB
    D = EB.DIMS[cls][0]
    n = len(fx[cls + "/a"])
    kind, delta = np.zeros(n, np.int32), np.zeros(n)
    q = 0
    for k in range(1, n, 4):
        e, info = fx[cls + "/e"][k], fx[cls + "/info"][k].reshape(D, D)
        chi = float(e @ info @ e)
        kd = (EB.RK_HUBER, EB.RK_CAUCHY, EB.RK_TUKEY, EB.RK_DCS)[q % 4]
        outlier = (q // 4 + q) % 2 == 1
        kind[k] = kd
        delta[k] = chi * (0.4 if outlier else 2.0) if kd == EB.RK_DCS else math.sqrt(chi) * (0.55 if outlier else 1.5)
        q += 1
    fx[cls + "/rk_kind"], fx[cls + "/rk_delta"] = kind, delta


# ---------------------------------------------------------------- evaluation, family assertions, the oracle's own noise
def evaluate_all(fx):
    import edge_blocks_ref as EB
    for cls in EB.CLASSES:
        D, NA, NB = EB.DIMS[cls]
        n = len(fx[cls + "/a"])
        fx[cls + "/e"], fx[cls + "/J"] = np.zeros((n, D)), np.zeros((n, D, NA + NB))
        fx[cls + "/fixed_a"] = fx["cam_fixed"][fx[cls + "/a"]].astype(np.int32)
        fx[cls + "/fixed_b"] = (fx["cam_fixed"] if cls == "odo" else fx["cub_fixed"])[fx[cls + "/b"]].astype(np.int32)
        assert int(fx[cls + "/fixed_a"].sum()) == 2 and int(fx[cls + "/fixed_b"].sum()) == 2
        if cls == "cub":
            fx["cub/win"], fx["cub/runner"], fx["cub/lead"] = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n)
            fx["cub/e_runner"], fx["cub/J_runner"] = np.zeros((n, D)), np.zeros((n, D, NA + NB))
        if cls == "box":
            fx["box/lead_px"] = np.zeros((n, 4))
        if cls != "box":
            fx[cls + "/angle"] = np.zeros(n)
            fx[cls + "/e_alt"], fx[cls + "/J_alt"] = np.zeros((n, D)), np.zeros((n, D, NA + NB))
        for k in range(n):
            fam = str(fx[cls + "/family"][k])
            e, J, info = evaluate_edge(fx, cls, k)
            fx[cls + "/e"][k], fx[cls + "/J"][k] = e, J
            if cls != "box":
                ang = fx[cls + "/angle"][k] = info["angle"]
                # d > 0.99999 <=> angle < 4.47e-3; a 1e-9 step moves the angle by ~1e-9
                if fam == "log_small":
                    assert min(abs(ang - 1e-3), abs(ang - 3e-3)) < 1e-4
                    fx[cls + "/e_alt"][k], fx[cls + "/J_alt"][k] = evaluate_edge(fx, cls, k, formula="acos")[:2]     # the other formula, for the guard
                elif fam == "log_acos":
                    assert min(abs(ang - 6e-3), abs(ang - 1e-2)) < 1e-4
                elif cls == "odo":
                    assert (0.1 <= ang <= 1.0) if fam == "moderate" else (2.0 <= ang <= 2.6)
                else:
                    assert ang > 6e-3
            if cls == "cub":
                fx["cub/win"][k], fx["cub/runner"][k], fx["cub/lead"][k] = info["win"], info["runner"], info["lead"]
                if fam == "near_tie":
                    assert NEAR_TIE_LEAD[0] <= info["lead"] <= NEAR_TIE_LEAD[1], info["lead"]
                    half = fx["cuboids"][fx["cub/b"][k], 7:9]
                    assert abs(half[0] - half[1]) <= 0.011
                else:
                    assert info["lead"] > CLEAR_LEAD, (fam, info["lead"])
                    half = fx["cuboids"][fx["cub/b"][k], 7:9]
                    assert abs(half[0] - half[1]) > 0.4
                if fam.startswith("cand"):
                    assert info["win"] == int(fam[4])
                elif fam != "near_tie":
                    assert info["win"] == 1
                if fam.startswith("cand") or fam == "near_tie":
                    fx["cub/e_runner"][k], fx["cub/J_runner"][k] = evaluate_edge(fx, cls, k, pick=info["runner"])[:2]
            if cls == "box":
                fx["box/lead_px"][k] = info["lead_px"]
                assert info["lead_px"].min() > 1e-3 and info["depth"].min() >= 2 and info["depth"].max() <= 40
                K = fx["box/K"][k]
                assert K[0] != K[4] and K[1] != 0
                uv = info["uv"]
                inside = (uv[:, 0] >= 0) & (uv[:, 0] < IMG_W) & (uv[:, 1] >= 0) & (uv[:, 1] < IMG_H)
                assert (inside.all() and info["depth"].min() >= 4) if fam == "generic" else (inside.any() and not inside.all())
        draw_kernels(fx, cls)
    fams = fx["cub/family"].astype(str)
    assert all((fams == "cand%d" % i).sum() >= 6 for i in range(4)) and (fams == "near_tie").sum() >= 8
    assert sorted(set(fx["cub/win"][fams == "near_tie"])) == [0, 1, 2, 3]
    assert (fx["odo/a"] > fx["odo/b"]).sum() >= 8 and (fx["odo/a"] < fx["odo/b"]).sum() >= 8
    assert np.abs(fx["cams"][:, :3]).max() <= 50


def measure_oracle(fx):
    """The CPU oracle (the float64 restatement: the reference's own noise) on the disjoint graph -> oracle_dev/... entries."""
    import edge_blocks_ref as EB
    pr, ends = EB.layout(fx, EB.CLASSES, shared=False)
    P = EB.oracle_problem(pr)
    P.compute_errors()
    Hpp, _, _, b = P.build_system()
    P.close()
    tab = EB.family_table(fx, EB.edge_devs(fx, pr, ends, Hpp, b))
    for cls in tab:
        for fam in tab[cls]:
            for kd, v in tab[cls][fam].items():
                fx["oracle_dev/%s/%s/%s" % (cls, fam, kd)] = np.float64(v)
        pc, _ = EB.layout(fx, (cls,), shared=False)
        Q = EB.oracle_problem(pc)
        chi = Q.compute_errors()[0]
        Q.close()
        want = EB.chi2_ref(fx, (cls,))
        fx["oracle_dev/%s/chi2" % cls] = np.float64(abs(chi - want) / want)
    return tab


def print_table(fx, tab):
    import edge_blocks_ref as EB
    print("oracle_dev: worst max|B - B_ref| / max|B_ref| of the CPU oracle per class, family and block kind")
    print("  %-5s %-10s %3s  %s" % ("class", "family", "n", "  ".join("%-8s" % k for k in EB.KINDS)))
    for cls in EB.CLASSES:
        fams = fx[cls + "/family"].astype(str)
        for fam in tab[cls]:
            print("  %-5s %-10s %3d  %s" % (cls, fam, (fams == fam).sum(), "  ".join("%-8.2e" % tab[cls][fam][k] for k in EB.KINDS)))
        print("  %-5s chi2 %.2e" % (cls, float(fx["oracle_dev/%s/chi2" % cls])))


def main():
    rng = np.random.default_rng(90517)
    fx = {}
    fx["cams"], fx["cam_fixed"], fx["cuboids"], fx["cub_fixed"] = draw_pool(rng)
    draw_cuboid_edges(rng, fx)
    draw_box_edges(rng, fx)
    draw_odom_edges(rng, fx)
    evaluate_all(fx)
    tab = measure_oracle(fx)
    print_table(fx, tab)
    worst = max(float(v) for k, v in fx.items() if k.startswith("oracle_dev/") and not k.endswith("chi2"))
    assert worst <= 1e-5, "a family is badly conditioned (oracle_dev %.3g > 1e-5): change its inputs" % worst
    np.savez_compressed(OUT, **fx)
    size = os.path.getsize(OUT)
    assert size < 400 * 1024, size
    print("wrote %s: %d + %d + %d edges, %d bytes" % (OUT, len(fx["cub/a"]), len(fx["box/a"]), len(fx["odo/a"]), size))


if __name__ == "__main__":
    main()
