"""The numeric-Jacobian edge classes against tests/golden/ba_edge_blocks.npz (test infrastructure, not a test file; numpy only).

The fixture (tools/make_edge_golden.py) holds, per EdgeSE3Cuboid ("cub"), EdgeSE3CuboidProj ("box") and EdgeSE3Expmap ("odo") edge, the
inputs as float64 and the error e and the exact central-difference quotient J (delta = 1e-9) evaluated at 60 digits.  This module forms
what g2o's constructQuadraticForm makes of them (base_binary_edge.hpp:54-120: H_aa = Ja^T W Ja, H_ab = Ja^T W Jb, H_bb = Jb^T W Jb,
b = -J^T W e with W = rho' Omega; a fixed vertex gets no block) in float64 numpy, wires the edges into graphs and compares a system
(dense H_pp in g2o order, b) with the sums of those blocks.

Layouts.  "shared": the fixture's vertex pool, vertices shared between edges (only the vertices the chosen classes touch).  "disjoint":
every edge gets copies of its two vertices, so every block of H_pp is one edge's block.

Bounds.  The side under test evaluates the quotient in float64, so each of its blocks carries noise of about ulp * |intermediate| / 2 delta.
The generator measured that noise for the CPU oracle per class, family and block kind (oracle_dev/...: worst max|B - B_ref| / max|B_ref|
over the family's edges).  A block that is the sum of several edges' blocks may deviate by the sum of its parts' allowances:
    max|B - B_ref| <= factor * sum_k oracle_dev[class_k, family_k, kind_k] * max|B_ref,k|
which for a single contribution is the relative bound factor * oracle_dev of that block, relative to that block alone.  A block whose
reference is exactly zero (a fixed end, rho' = 0 of a Tukey outlier, no edge between two vertices) must be exactly zero.
"""
import math
import os

import numpy as np

import ba_numpy_ref as ref

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ba_edge_blocks.npz")
CLASSES = ("cub", "box", "odo")
DIMS = {"cub": (9, 6, 9), "box": (4, 6, 9), "odo": (6, 6, 6)}            # error dimension, tangent dimensions of the two vertices
EDGE_CLASS = {"cub": 1, "box": 2, "odo": 3}                               # enum cs_edge_class / ba_oracle_set_robust_kernels
KINDS = ("H_aa", "H_bb", "H_ab", "b_a", "b_b")
RK_HUBER, RK_CAUCHY, RK_DCS, RK_TUKEY = 1, 3, 5, 6


def clear_lead_threshold():
    """The kernel's near-tie threshold, read from the one place that names it (csrc/cs_se3.h: CUBE_CLEAR_LEAD)."""
    import re
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "cube_slam_wu_amd", "csrc", "cs_se3.h")
    with open(hdr) as f:
        m = re.findall(r"constexpr\s+double\s+CUBE_CLEAR_LEAD\s*=\s*([0-9.eE+-]+)\s*;", f.read())
    assert len(m) == 1, "CUBE_CLEAR_LEAD not found in cs_se3.h"
    return float(m[0])


def load(path=FIXTURE):
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


# ---- robust kernels (core/robust_kernel_impl.cpp:78-162; Huber's dsqr and Tukey's squares are `float` members of the vendored g2o,
# robust_kernel_impl.h:86,107-108; Tukey's width is handed over as delta: deltaSqr = delta^2, inv = 1 / delta^2) ----------------------
def robustify(kind, delta, c):
    """(rho, rho') of the squared error c."""
    if kind == 0:
        return c, 1.0
    if kind == RK_HUBER:
        dsqr = float(np.float32(delta * delta))
        if c <= dsqr:
            return c, 1.0
        s = math.sqrt(c)
        return 2 * s * delta - dsqr, delta / s
    if kind == RK_CAUCHY:
        dsqr = delta * delta
        aux = c / dsqr + 1.0
        return dsqr * math.log(aux), 1.0 / aux
    if kind == RK_DCS:
        s = min(1.0, 2.0 * delta / (delta + c))
        return s * c * s, s * s
    if kind == RK_TUKEY:
        dsqr, inv = float(np.float32(delta * delta)), float(np.float32(1.0 / (delta * delta)))
        if c <= dsqr:
            d = 1 - c * inv
            return dsqr * (1 - d * d * d), 3 * d * d
        return dsqr, 0.0
    raise ValueError(kind)


def edge_blocks(e, J, info, NA, w=1.0, fixed_a=False, fixed_b=False):
    """(H_aa, H_bb, H_ab, b_a, b_b) of one edge: J is D x (NA + NB), info D x D, w = rho'."""
    W = w * info
    Ja, Jb = J[:, :NA] * (0.0 if fixed_a else 1.0), J[:, NA:] * (0.0 if fixed_b else 1.0)
    r = W @ e
    return Ja.T @ W @ Ja, Jb.T @ W @ Jb, Ja.T @ W @ Jb, -(Ja.T @ r), -(Jb.T @ r)


def fixture_edge_blocks(fx, cls, k, e=None, J=None, info=None):
    """The reference blocks of edge k of a class (optionally with e / J / info replaced: the guards), and its chi2 term rho(e^T Omega e)."""
    D, NA, _ = DIMS[cls]
    e = fx[cls + "/e"][k] if e is None else e
    J = fx[cls + "/J"][k] if J is None else J
    info = fx[cls + "/info"][k].reshape(D, D) if info is None else info
    c = float(e @ info @ e)
    rho, w = robustify(int(fx[cls + "/rk_kind"][k]), float(fx[cls + "/rk_delta"][k]), c)
    return edge_blocks(e, J, info, NA, w, bool(fx[cls + "/fixed_a"][k]), bool(fx[cls + "/fixed_b"][k])), rho


def chi2_ref(fx, classes):
    return math.fsum(fixture_edge_blocks(fx, c, k)[1] for c in classes for k in range(len(fx[c + "/a"])))


def rel_dev(B, Bref):
    """max|B - B_ref| / max|B_ref|; for an exactly zero reference: 0 if B is exactly zero, else inf."""
    s = float(np.abs(Bref).max())
    if s == 0.0:
        return 0.0 if not np.any(B) else np.inf
    return float(np.abs(B - Bref).max()) / s


# ---- graphs ----------------------------------------------------------------------------------------------------------------------------
def layout(fx, classes, shared):
    """A problem dict (the keys of synth_ba.make_problem that capi.ba_from_dict and the oracle read) carrying the edges of the given
    classes, and per class the (first vertex, second vertex) indices of every edge in that dict's numbering."""
    cams, cam_fixed, cubs, cub_fixed = [], [], [], []
    ends = {}
    if shared:
        used_c = sorted({int(v) for c in classes for v in fx[c + "/a"]} | ({int(v) for v in fx["odo/b"]} if "odo" in classes else set()))
        used_o = sorted({int(v) for c in classes if c != "odo" for v in fx[c + "/b"]})
        cmap, omap = {v: i for i, v in enumerate(used_c)}, {v: i for i, v in enumerate(used_o)}
        cams, cam_fixed = [fx["cams"][v] for v in used_c], [fx["cam_fixed"][v] for v in used_c]
        cubs, cub_fixed = [fx["cuboids"][v] for v in used_o], [fx["cub_fixed"][v] for v in used_o]
        for c in classes:
            bm = cmap if c == "odo" else omap
            ends[c] = (np.array([cmap[int(v)] for v in fx[c + "/a"]], np.int32), np.array([bm[int(v)] for v in fx[c + "/b"]], np.int32))
    else:
        for c in classes:
            ia, ib = [], []
            for a, b in zip(fx[c + "/a"], fx[c + "/b"]):
                ia.append(len(cams)); cams.append(fx["cams"][a]); cam_fixed.append(fx["cam_fixed"][a])
                if c == "odo":
                    ib.append(len(cams)); cams.append(fx["cams"][b]); cam_fixed.append(fx["cam_fixed"][b])
                else:
                    ib.append(len(cubs)); cubs.append(fx["cuboids"][b]); cub_fixed.append(fx["cub_fixed"][b])
            ends[c] = (np.array(ia, np.int32), np.array(ib, np.int32))
    z = np.zeros(0, np.int32)
    pr = dict(cams=np.array(cams).reshape(-1, 7), cam_fixed=np.array(cam_fixed, np.int32), cuboids=np.array(cubs).reshape(-1, 10),
              cub_fixed=np.array(cub_fixed, np.int32), points=np.zeros((0, 3)), pt_fixed=z,
              e_pt=z, e_cam=z, e_uv=np.zeros((0, 2)), e_info=np.zeros((0, 4)), e_intr=np.zeros((0, 4)), e_huber=np.zeros(0),
              ce_cam=z, ce_cub=z, ce_meas=np.zeros((0, 10)), ce_info=np.zeros((0, 81)),
              pe_cam=z, pe_cub=z, pe_meas=np.zeros((0, 4)), pe_info=np.zeros((0, 16)), pe_K=np.zeros((0, 9)),
              oe_i=z, oe_j=z, oe_meas=np.zeros((0, 7)), oe_info=np.zeros((0, 36)), robust={})
    for c in classes:
        p = {"cub": "ce", "box": "pe", "odo": "oe"}[c]
        pr[p + ("_i" if c == "odo" else "_cam")], pr[p + ("_j" if c == "odo" else "_cub")] = ends[c]
        pr[p + "_meas"], pr[p + "_info"] = fx[c + "/meas"], fx[c + "/info"]
        if c == "box":
            pr["pe_K"] = fx["box/K"]
        pr["robust"][EDGE_CLASS[c]] = (fx[c + "/rk_kind"].astype(np.int32), fx[c + "/rk_delta"].astype(np.float64))
    return pr, ends


def oracle_problem(pr, cuboids_first=False):
    from oracle import ba_oracle_py as O
    P = O.Problem(pr["cams"], pr["cam_fixed"], pr["cuboids"], pr["cub_fixed"], pr["points"], pr["pt_fixed"], cuboids_first=cuboids_first)
    if len(pr["ce_cam"]):
        P.set_edges_cuboid(pr["ce_cam"], pr["ce_cub"], pr["ce_meas"], pr["ce_info"])
    if len(pr["pe_cam"]):
        P.set_edges_cuboid_proj(pr["pe_cam"], pr["pe_cub"], pr["pe_meas"], pr["pe_info"], pr["pe_K"])
    if len(pr["oe_i"]):
        P.set_edges_odom(pr["oe_i"], pr["oe_j"], pr["oe_meas"], pr["oe_info"])
    for cls, (kind, delta) in pr["robust"].items():
        P.set_robust_kernels(cls, kind, delta)
    return P


def _columns(pr, ends, cls, cuboids_first):
    """g2o columns (-1: fixed) of the two ends of every edge of a class."""
    cam_g, cub_g = ref.pose_columns(pr, cuboids_first)
    ia, ib = ends[cls]
    return cam_g[ia], (cam_g if cls == "odo" else cub_g)[ib]


def oracle_dev(fx, cls, family, kind):
    return float(fx["oracle_dev/%s/%s/%s" % (cls, family, kind)])


def reference_system(fx, pr, ends, cuboids_first=False, dev=oracle_dev):
    """(H_ref, b_ref, A_H, A_b): the sums of the per-edge reference blocks in g2o order, and next to every entry the allowance
    sum_k dev_k * max|B_ref,k| of the blocks that were added there (zero where nothing, or only exact zeros, were added)."""
    n = 6 * int((pr["cam_fixed"] == 0).sum()) + 9 * int((pr["cub_fixed"] == 0).sum())
    H, b, AH, Ab = np.zeros((n, n)), np.zeros(n), np.zeros((n, n)), np.zeros(n)
    for cls in ends:
        _, NA, NB = DIMS[cls]
        ca, cb = _columns(pr, ends, cls, cuboids_first)
        for k in range(len(ca)):
            (Haa, Hbb, Hab, ba, bb), _ = fixture_edge_blocks(fx, cls, k)
            fam = str(fx[cls + "/family"][k])
            d = {kd: dev(fx, cls, fam, kd) for kd in KINDS}
            a, c = int(ca[k]), int(cb[k])
            if a >= 0:
                H[a:a + NA, a:a + NA] += Haa; AH[a:a + NA, a:a + NA] += d["H_aa"] * np.abs(Haa).max()
                b[a:a + NA] += ba; Ab[a:a + NA] += d["b_a"] * np.abs(ba).max()
            if c >= 0:
                H[c:c + NB, c:c + NB] += Hbb; AH[c:c + NB, c:c + NB] += d["H_bb"] * np.abs(Hbb).max()
                b[c:c + NB] += bb; Ab[c:c + NB] += d["b_b"] * np.abs(bb).max()
            if a >= 0 and c >= 0:
                H[a:a + NA, c:c + NB] += Hab; AH[a:a + NA, c:c + NB] += d["H_ab"] * np.abs(Hab).max()
                H[c:c + NB, a:a + NA] += Hab.T; AH[c:c + NB, a:a + NA] += d["H_ab"] * np.abs(Hab).max()
    return H, b, AH, Ab


def check_system(fx, pr, ends, H, b, cuboids_first=False, factor=8.0, what=""):
    """Every entry of (H, b) within factor * allowance of the reference; entries with no allowance exactly zero.  Returns the worst
    ratio |deviation| / (factor * allowance) seen."""
    Hr, br, AH, Ab = reference_system(fx, pr, ends, cuboids_first)
    assert H.shape == Hr.shape and b.shape == br.shape, "%s: system size %s, reference %s" % (what, H.shape, Hr.shape)
    worst = 0.0
    for name, X, Xr, A in (("H_pp", H, Hr, AH), ("b", b, br, Ab)):
        zero = A == 0
        assert not np.any(X[zero]) and not np.any(Xr[zero]), "%s: %s has entries where the reference has none" % (what, name)
        ratio = np.abs(X - Xr)[~zero] / (factor * A[~zero])
        if ratio.size:
            i = int(np.argmax(ratio))
            assert ratio[i] <= 1.0, "%s: %s deviates by %.3g of its allowance (entry %s)" % (what, name, ratio[i], np.argwhere(~zero)[i])
            worst = max(worst, float(ratio[i]))
    return worst


def edge_devs(fx, pr, ends, H, b, cuboids_first=False):
    """Per class an (n_edges, 5) array of max|B - B_ref| / max|B_ref| per block kind, for a DISJOINT layout (every block one edge's)."""
    out = {}
    for cls in ends:
        _, NA, NB = DIMS[cls]
        ca, cb = _columns(pr, ends, cls, cuboids_first)
        D = np.zeros((len(ca), 5))
        for k in range(len(ca)):
            Bref, _ = fixture_edge_blocks(fx, cls, k)
            a, c = int(ca[k]), int(cb[k])
            za, zc = np.zeros((NA, NA)), np.zeros((NB, NB))
            got = (H[a:a + NA, a:a + NA] if a >= 0 else za, H[c:c + NB, c:c + NB] if c >= 0 else zc,
                   H[a:a + NA, c:c + NB] if a >= 0 and c >= 0 else np.zeros((NA, NB)), b[a:a + NA] if a >= 0 else np.zeros(NA), b[c:c + NB] if c >= 0 else np.zeros(NB))
            D[k] = [rel_dev(g, r) for g, r in zip(got, Bref)]
        out[cls] = D
    return out


def family_table(fx, devs):
    """{class: {family: {kind: worst deviation}}} of edge_devs()' output."""
    tab = {}
    for cls, D in devs.items():
        fams = fx[cls + "/family"].astype(str)
        tab[cls] = {f: {kd: float(D[fams == f, j].max()) for j, kd in enumerate(KINDS)} for f in sorted(set(fams))}
    return tab
