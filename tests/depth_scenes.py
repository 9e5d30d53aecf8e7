"""Seeded multi-frame curve scenes for the inverse-depth filter (tests/test_depth_oracle.py, tools/): the curves, rigs and
sampling of tests/align_scenes.py (imported, not edited), seen by a keyframe and by FRAMES later frames along a planted
trajectory -- the planted motion of tests/pose_scenes.py applied k times for frame k.

The keyframe mates are the curves sampled at one set of parameters; N(0, sigma_disp) px of disparity noise is planted on the
right mate's x, so that the triangulated depth of mate i is lambda*_i times the true one.  Every later frame's TOED edge lists
are the same curves sampled at other parameters, moved by N(0, sigma) across the edge, plus uniform clutter: no
point-to-point correspondence exists, only the curves agree."""
import math

import numpy as np

from tests import align_scenes as asc
from tests import oracle as orc
from tests import pose_scenes as ps

W, H = asc.W, asc.H
FRAMES = 4

# Fixed point: noise-free scenes (no disparity noise, no edge noise, no clutter) fused at the planted poses
FIXED_POINT = tuple((rig, seed) for rig in asc.RIGS for seed in (0, 1))
# Recovery and feedback: (rig, seed, kind, sigma px across the edge, clutter edges); every scene class of tests/align_scenes.py
NOISY = asc.NOISY
SIGMA_DISP = 0.25


def poses(frames=FRAMES):
    """[(R_k, t_k)], k = 1 .. frames: the planted motion composed k times (Gc_k = R_k Gamma + t_k)"""
    out, R, t = [], np.eye(3), np.zeros(3)
    for _ in range(frames):
        R, t = ps.R_GT @ R, ps.R_GT @ t + ps.T_GT
        out.append((R.copy(), t.copy()))
    return out


def scene(rig_name, seed, kind="mixed", sigma=0.0, clutter=0, sigma_disp=0.0, frames=FRAMES, n_curves=24, kf_px=1.0, cf_px=0.5):
    """dict: calib, poses, kf_left / kf_right (the right mates carry the disparity noise), kf_right_true, lambda_true (the
    triangulated depth over the true one per mate), frames: [(edges_left, edges_right)] per later frame"""
    K, Kr, R21, T21 = asc.calib(rig_name, True)
    R21 = np.asarray(R21, dtype=np.float64).reshape(3, 3)
    T21 = np.asarray(T21, dtype=np.float64)
    rng = np.random.default_rng(9100 + 131 * seed + (0 if rig_name == "kitti" else 17))
    P = poses(frames)
    kf, cf = [], [[] for _ in P]
    taken = [[np.zeros((0, 3)), np.zeros((0, 3))] for _ in P]
    tries = 0
    while len(kf) < n_curves and tries < 40 * n_curves:
        tries += 1
        k = "segment" if kind == "segments" or (kind == "mixed" and rng.random() < 0.5) else "arc"
        f, L, step = asc._curve(rng, k, K)
        Xk, Dk = f(np.arange(0.0, L, kf_px * step))
        eL, okL = asc._see(K, Xk, Dk)
        eR, okR = asc._see(Kr, Xk @ R21.T + T21, Dk @ R21.T)
        fin = orc.finalize_pairs(K, Kr, R21, T21, eL, eR)
        good = okL & okR & (np.abs(fin[:, 6:9] - Xk).max(axis=1) < 1e-6) & (np.abs(np.einsum("ij,ij->i", fin[:, 9:12], Dk)) > 0.999)
        if good.sum() < 20:
            continue
        Xs, Ds = f(np.arange(0.37 * cf_px * step, L, cf_px * step))
        seen, clash = [], False
        for (Rg, tg), old in zip(P, taken):
            Xc, Dc = Xs @ Rg.T + tg, Ds @ Rg.T
            cL, vL = asc._see(K, Xc, Dc)
            cR, vR = asc._see(Kr, Xc @ R21.T + T21, Dc @ R21.T)
            seen.append((cL[vL], cR[vR]))
            # the association stays unambiguous, as in tests/align_scenes.py: no earlier curve within 6 px at an orientation
            # within 25 degrees, in either image of any frame
            for own, prev in zip(seen[-1], old):
                own = np.stack([own["x"], own["y"], own["theta"]], axis=1)[::4]
                if len(prev) and len(own):
                    d = np.hypot(own[:, None, 0] - prev[None, :, 0], own[:, None, 1] - prev[None, :, 1])
                    a = np.abs(np.degrees(own[:, None, 2] - prev[None, :, 2])) % 180.0
                    clash = clash or bool(((d < 6.0) & (np.minimum(a, 180.0 - a) < 25.0)).any())
        if clash or len(seen[0][0]) < 20:
            continue
        for s, old, lst in zip(seen, taken, cf):
            for c in range(2):
                old[c] = np.concatenate([old[c], np.stack([s[c]["x"], s[c]["y"], s[c]["theta"]], axis=1)[::4]])
            lst.append(s)
        kf.append((eL[good], eR[good]))
    kf_left, kf_true = np.concatenate([a for a, _ in kf]), np.concatenate([b for _, b in kf])
    kf_right = kf_true.copy()
    if sigma_disp > 0:
        kf_right["x"] += rng.normal(0.0, sigma_disp, len(kf_right))
    with np.errstate(all="ignore"):
        z_noisy = orc.finalize_pairs(K, Kr, R21, T21, kf_left, kf_right)[:, 8]
        z_true = orc.finalize_pairs(K, Kr, R21, T21, kf_left, kf_true)[:, 8]
    lists = []
    for lst in cf:
        pair = []
        for c in range(2):
            e = np.concatenate([s[c] for s in lst]).copy()
            if sigma > 0:                          # across the edge: along n = (sin theta, -cos theta)
                d = rng.normal(0.0, sigma, len(e))
                e["x"] += d * np.sin(e["theta"])
                e["y"] -= d * np.cos(e["theta"])
            cl = np.zeros(clutter, dtype=orc.EDGE_DTYPE)
            cl["x"], cl["y"] = rng.uniform(asc.BORDER, W - asc.BORDER, clutter), rng.uniform(asc.BORDER, H - asc.BORDER, clutter)
            cl["theta"] = rng.uniform(-math.pi, math.pi, clutter)
            both = np.concatenate([e, cl])
            both = both[rng.permutation(len(both))]
            both["index"] = np.arange(len(both))
            pair.append(both)
        lists.append(tuple(pair))
    return dict(calib=(K, Kr, R21, T21), poses=P, kf_left=kf_left, kf_right=kf_right, kf_right_true=kf_true, lambda_true=z_noisy / z_true,
                frames=lists, w=W, h=H)


def fuse(sc, frames=None, **params):
    """the oracle's filter over the scene's frames at their planted poses, each associated on Gamma / lambda with the current
    lambda: [(lambda, info, n_obs, record)] after every frame"""
    from tests import oracle_depth as od
    state, out = None, []
    for (R, t), (E0, E1) in list(zip(sc["poses"], sc["frames"]))[:frames]:
        lam = None if state is None else state[0]
        a = od.associate(sc["kf_left"], sc["kf_right"], lam, E0, E1, W, H, sc["calib"], R, t)
        r = od.update(sc["kf_left"], sc["kf_right"], E0, E1, a[0], a[1], W, H, sc["calib"], R, t, state=state, **params)
        state = (r["lambda_"], r["info"], r["n_obs"])
        out.append(state + (r,))
    return out
