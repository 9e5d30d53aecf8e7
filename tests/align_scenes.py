"""Seeded curve scenes for the edge-alignment tests (tests/test_align_oracle.py, tests/test_gpu_align.py, tools/): 3-D straight
segments and arcs seen by the rigs of tests/pose_scenes.py (their R21 / T21, the focal length scaled to a 200 x 120 image,
K_right := K_left so that the quad-based refit can be run on the same scene) under its planted motion.

The keyframe mates are the curves sampled at one set of parameters and projected into the keyframe's two cameras; the
current frame's TOED edge lists are the SAME curves sampled at OTHER parameters, about 0.5 px apart, seen through the planted
motion.  No point-to-point correspondence exists between the two frames: only the curves agree.  Clutter edges are scattered
uniformly, and every current-frame edge is moved by N(0, sigma) across its edge (along its normal)."""
import math

import numpy as np

from tests import oracle as orc
from tests import oracle_pose as op
from tests import pose_scenes as ps

W, H = 200, 120
BORDER = 10.0          # TOED keeps nothing nearer than 10 px to the border
RIGS = ("kitti", "euroc")

# Fixed point (tests/test_align_oracle.py::test_fixed_point): the largest movement of the pose, max(|R - R_gt|, |t - t_gt|)
# over the entries, that the oracle shows over FIXED_POINT started at the planted pose.  Measured with tests/oracle_align.py;
# the test asserts 10 x this.
FIXED_POINT = tuple((rig, seed) for rig in RIGS for seed in (0, 1, 2))
FIXED_POINT_MEASURED = 1.4432899320127035e-15   # kitti seeds 0 and 1; the largest normal distance at the planted pose is 2.1e-13 px

# Recovery: (rig, seed, kind, sigma px, clutter edges); every scene is started from PERTURB applied to the planted pose
NOISY = tuple((rig, seed, kind, sigma, clutter) for rig in RIGS for seed in (0, 1) for kind, sigma, clutter in
              (("segments", 0.2, 400), ("mixed", 0.2, 400), ("mixed", 0.4, 1000)))
PERTURB = dict(axis=(0.5, -1.0, 0.3), angle=0.006, dt=(0.015, -0.01, 0.02))


def calib(rig_name, true_right=False):
    """(K_left, K_right := K_left, R21, T21), K as 3 x 3, for a W x H image.  true_right (the parity cases): a right camera
    of its own, so that a K_right := K_left anywhere in the stage would show."""
    K0, _, R21, T21 = ps.rig(rig_name)
    f = K0[0, 0] * W / (2.0 * K0[0, 2])
    K = np.array([[f, 0.0, W / 2.0], [0.0, f, H / 2.0], [0.0, 0.0, 1.0]])
    Kr = K.copy()
    if true_right:
        Kr = np.array([[1.004 * f, 0.0, W / 2.0 + 0.8], [0.0, 0.997 * f, H / 2.0 - 0.5], [0.0, 0.0, 1.0]])
    return K, Kr, R21, T21


def perturbed(R, t, axis=PERTURB["axis"], angle=PERTURB["angle"], dt=PERTURB["dt"]):
    return op.rot(axis, angle) @ R, np.asarray(t, dtype=np.float64) + np.asarray(dt)


def _curve(rng, kind, K):
    """a 3-D curve in the keyframe's left camera: callable s -> (points, unit tangents), its length and the length that one
    pixel spans at its depth, in metres"""
    z = rng.uniform(3.0, 12.0)
    u, v = rng.uniform(0.15 * W, 0.85 * W), rng.uniform(0.15 * H, 0.85 * H)
    P = np.array([(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z])
    D = rng.normal(size=3)
    D[2] *= 1.5                                   # spread in depth along the curve
    D /= np.linalg.norm(D)
    px = z / K[0, 0]                              # metres per pixel at the curve's depth
    if kind == "segment":
        L = rng.uniform(40.0, 110.0) * px
        return (lambda s: (P + np.outer(s - L / 2, D), np.tile(D, (len(s), 1)))), L, px
    N = np.cross(D, rng.normal(size=3))
    N /= np.linalg.norm(N)
    rad = rng.uniform(25.0, 70.0) * px
    span = rng.uniform(0.8, 2.2)                  # radians of arc
    C = P - rad * N

    def arc(s):
        a = s / rad - span / 2
        return (C + rad * (np.outer(np.cos(a), N) + np.outer(np.sin(a), D)), -np.outer(np.sin(a), N) + np.outer(np.cos(a), D))
    return arc, rad * span, px


def _see(K, X, D):
    e = op._edge(K, X, D)
    ok = (X[:, 2] > 0.5) & (e["x"] > BORDER) & (e["x"] < W - BORDER) & (e["y"] > BORDER) & (e["y"] < H - BORDER)
    return e, ok


def scene(rig_name, seed, kind="mixed", sigma=0.0, clutter=0, n_curves=40, kf_px=1.0, cf_px=0.5, true_right=False):
    """dict: calib, R_gt, t_gt, kf_left / kf_right (+ kf_curve), edges_left / edges_right of the current frame, and for the
    quad comparison cf_left_all / cf_right_all (every current-frame sample in both images, NaN where not seen) with cf_curve."""
    K, Kr, R21, T21 = calib(rig_name, true_right)
    R21 = np.asarray(R21, dtype=np.float64).reshape(3, 3)
    rng = np.random.default_rng(7000 + 131 * seed + (0 if rig_name == "kitti" else 17))
    Rg, tg = ps.R_GT, ps.T_GT
    kf, cf, taken = [], [], [np.zeros((0, 3)), np.zeros((0, 3))]
    tries = 0
    while len(kf) < n_curves and tries < 40 * n_curves:
        tries += 1
        k = "segment" if kind == "segments" or (kind == "mixed" and rng.random() < 0.5) else "arc"
        f, L, step = _curve(rng, k, K)
        s_kf = np.arange(0.0, L, kf_px * step)
        s_cf = np.arange(0.37 * cf_px * step, L, cf_px * step)
        Xk, Dk = f(s_kf)
        Xc, Dc = f(s_cf)
        Xc, Dc = Xc @ Rg.T + tg, Dc @ Rg.T
        eL, okL = _see(K, Xk, Dk)
        eR, okR = _see(Kr, Xk @ R21.T + T21, Dk @ R21.T)
        cL, vL = _see(K, Xc, Dc)
        cR, vR = _see(Kr, Xc @ R21.T + T21, Dc @ R21.T)
        # mates whose triangulation returns the sampled point and whose tangent is away from the epipolar planes
        fin = orc.finalize_pairs(K, Kr, R21, T21, eL, eR)
        good = okL & okR & (np.abs(fin[:, 6:9] - Xk).max(axis=1) < 1e-6) & (np.abs(np.einsum("ij,ij->i", fin[:, 9:12], Dk)) > 0.999)
        if good.sum() < 20 or vL.sum() < 20:
            continue
        # keep the association unambiguous: no earlier curve within 6 px at an orientation within 25 degrees, in either
        # current-frame image (crossings at a wider angle are welcome)
        # (every fourth sample, 2 px apart, is enough for a 6 px test)
        mine = [np.stack([e["x"][v], e["y"][v], e["theta"][v]], axis=1)[::4] for e, v in ((cL, vL), (cR, vR))]
        clash = False
        for own, old in zip(mine, taken):
            if len(old) and len(own):
                d = np.hypot(own[:, None, 0] - old[None, :, 0], own[:, None, 1] - old[None, :, 1])
                a = np.abs(np.degrees(own[:, None, 2] - old[None, :, 2])) % 180.0
                clash = clash or bool(((d < 6.0) & (np.minimum(a, 180.0 - a) < 25.0)).any())
        if clash:
            continue
        taken = [np.concatenate([old, own]) for old, own in zip(taken, mine)]
        kf.append((eL[good], eR[good]))
        cf.append((cL, vL, cR, vR))
    cid = len(kf)
    kf_left, kf_right = np.concatenate([a for a, _ in kf]), np.concatenate([b for _, b in kf])
    kf_curve = np.concatenate([np.full(len(a), i) for i, (a, _) in enumerate(kf)])
    cf_curve = np.concatenate([np.full(len(c[0]), i) for i, c in enumerate(cf)])
    cL, vL = np.concatenate([c[0] for c in cf]), np.concatenate([c[1] for c in cf])
    cR, vR = np.concatenate([c[2] for c in cf]), np.concatenate([c[3] for c in cf])
    if sigma > 0:                                  # across the edge: along n = (sin theta, -cos theta)
        for e in (cL, cR):
            d = rng.normal(0.0, sigma, len(e))
            e["x"] += d * np.sin(e["theta"])
            e["y"] -= d * np.cos(e["theta"])
    lists = []
    for e, v in ((cL, vL), (cR, vR)):
        c = np.zeros(clutter, dtype=orc.EDGE_DTYPE)
        c["x"], c["y"] = rng.uniform(BORDER, W - BORDER, clutter), rng.uniform(BORDER, H - BORDER, clutter)
        c["theta"] = rng.uniform(-math.pi, math.pi, clutter)
        both = np.concatenate([e[v], c])
        both = both[rng.permutation(len(both))]    # no order to lean on
        both["index"] = np.arange(len(both))
        lists.append(both)
    for e, v in ((cL, vL), (cR, vR)):
        e["x"][~v] = np.nan
        e["y"][~v] = np.nan
    return dict(calib=(K, Kr, R21, np.asarray(T21, dtype=np.float64)), R_gt=Rg, t_gt=tg, kf_left=kf_left, kf_right=kf_right,
                kf_curve=kf_curve, edges_left=lists[0], edges_right=lists[1], cf_left_all=cL, cf_right_all=cR, cf_curve=cf_curve,
                n_curves=cid, w=W, h=H)


def nearest_sample_quads(sc):
    """(kf_left, kf_right, row_ptr, cf_left, cf_right): every mate paired with the nearest current-frame sample of ITS OWN curve
    (under the planted motion, in the left image) that both current-frame images see -- up to half a sample spacing of
    along-edge error per quad.  Mates without such a sample have an empty row."""
    K, Kr, R21, T21 = sc["calib"]
    fin = orc.finalize_pairs(K, Kr, R21, T21, sc["kf_left"], sc["kf_right"])
    Xc = fin[:, 6:9] @ sc["R_gt"].T + sc["t_gt"]
    qx, qy = K[0, 0] * Xc[:, 0] / Xc[:, 2] + K[0, 2], K[1, 1] * Xc[:, 1] / Xc[:, 2] + K[1, 2]
    cL, cR = sc["cf_left_all"], sc["cf_right_all"]
    seen = np.isfinite(cL["x"]) & np.isfinite(cR["x"])
    pick = np.full(len(fin), -1)
    for c in range(sc["n_curves"]):
        m, s = np.flatnonzero(sc["kf_curve"] == c), np.flatnonzero((sc["cf_curve"] == c) & seen)
        if not len(s) or not len(m):
            continue
        d = np.hypot(qx[m, None] - cL["x"][None, s], qy[m, None] - cL["y"][None, s])
        k = d.argmin(axis=1)
        near = d[np.arange(len(m)), k] < 2.0
        pick[m[near]] = s[k[near]]
    has = pick >= 0
    row_ptr = np.concatenate([[0], np.cumsum(has)]).astype(np.int32)
    return sc["kf_left"], sc["kf_right"], row_ptr, cL[pick[has]].copy(), cR[pick[has]].copy()
