"""Synthetic essential graphs for the Sim(3) pose-graph optimisation (capi.PoseGraph): keyframes on a ring, odometry and short
loop links with noisy relative Sim(3) measurements, a drifted start.  float64 numpy; states are qx qy qz qw tx ty tz s, world-to-keyframe."""
import numpy as np


def _rotate(q, v):
    qv = q[:3]
    uv = 2.0 * np.cross(qv, v)
    return v + q[3] * uv + np.cross(qv, uv)


def mul(a, b):
    ax, ay, az, aw = a[:4]
    bx, by, bz, bw = b[:4]
    q = [aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz]
    return np.concatenate([q, a[7] * _rotate(a[:4], b[4:7]) + a[4:7], [a[7] * b[7]]])


def inv(a):
    qc = np.array([-a[0], -a[1], -a[2], a[3]])
    return np.concatenate([qc, _rotate(qc, -a[4:7] / a[7]), [1.0 / a[7]]])


def exp(u):
    """Sim(3) exponential of [omega, upsilon, sigma]: the consistent closed form (a noise generator: not g2o's branches)."""
    w, ups, sigma = np.asarray(u[:3], float), np.asarray(u[3:6], float), float(u[6])
    th = float(np.linalg.norm(w))
    s = np.exp(sigma)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0.0]])
    if th < 1e-8:
        q = np.array([0.5 * w[0], 0.5 * w[1], 0.5 * w[2], 1.0])
    else:
        q = np.concatenate([np.sin(0.5 * th) * w / th, [np.cos(0.5 * th)]])
    q = q / np.linalg.norm(q)
    # W = A K + B K^2 + C I (the series where an angle or sigma vanishes)
    if abs(sigma) < 1e-9:
        C = 1.0
        A, B = ((1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3) if th >= 1e-6 else (0.5, 1.0 / 6.0)
    else:
        C = (s - 1) / sigma
        if th < 1e-6:
            A, B = ((sigma - 1) * s + 1) / sigma ** 2, ((0.5 * sigma ** 2 - sigma + 1) * s - 1) / sigma ** 3
        else:
            a, b, c = s * np.sin(th), s * np.cos(th), th ** 2 + sigma ** 2
            A, B = (a * sigma + (1 - b) * th) / (th * c), (C - ((b - 1) * sigma + a * th) / c) / th ** 2
    W = A * K + B * (K @ K) + C * np.eye(3)
    return np.concatenate([q, W @ ups, [s]])


def ring(n, seed, noise_rot=0.03, noise_trans=0.05, noise_scale=0.02, drift_rot=0.01, drift_trans=0.05, drift_scale=0.01, fix_scale=False, long_links=0.0, radius=5.0):
    """n keyframes on a ring of `radius` metres, keyframe k turned by about 0.3 of its angle on the ring.  Edges k -> k + 1 (closing the
    ring) and k -> k + 3 for every fourth k, plus a fraction `long_links` of n random long links; an edge's measurement is the true
    S_j S_i^-1 left-multiplied by exp(noise) (rad, m, log-scale sigmas).  The start is the odometry integrated from vertex 0 with a per-step
    drift exp(drift); vertex 0 is fixed.  fix_scale: every vertex has _fix_scale (pass noise_scale = drift_scale = 0 with it)."""
    rng = np.random.default_rng(seed)
    true = np.zeros((n, 8))
    for k in range(n):
        a = 2 * np.pi * k / n
        Swc = exp(np.concatenate([0.3 * a * np.array([0.1, -0.15, 1.0]) + 0.05 * rng.standard_normal(3), np.zeros(4)]))
        Swc[4:7] = [radius * np.cos(a), radius * np.sin(a), 0.2 * np.sin(3 * a)]
        true[k] = inv(Swc)

    def noise(r, t, s):
        return exp(np.concatenate([r * rng.standard_normal(3), t * rng.standard_normal(3), [s * rng.standard_normal()]]))

    pairs = [(k, (k + 1) % n) for k in range(n)] + [(k, (k + 3) % n) for k in range(0, n, 4) if n > 6]
    seen = {(min(p), max(p)) for p in pairs}
    for _ in range(int(round(long_links * n))):
        i, j = (int(v) for v in rng.integers(0, n, 2))
        if i != j and (min(i, j), max(i, j)) not in seen:
            seen.add((min(i, j), max(i, j)))
            pairs.append((i, j))
    vi = np.array([p[0] for p in pairs], np.int32)
    vj = np.array([p[1] for p in pairs], np.int32)
    meas = np.stack([mul(noise(noise_rot, noise_trans, noise_scale), mul(true[j], inv(true[i]))) for i, j in pairs])
    start = np.zeros((n, 8))
    start[0] = true[0]
    for k in range(n - 1):
        start[k + 1] = mul(noise(drift_rot, drift_trans, drift_scale), mul(mul(true[k + 1], inv(true[k])), start[k]))
    fixed = np.zeros(n, np.uint8)
    fixed[0] = 1
    return dict(sim8=start, sim8_true=true, fixed=fixed, fix_scale=np.full(n, 1 if fix_scale else 0, np.uint8), vi=vi, vj=vj, meas8=meas, info49=None)
