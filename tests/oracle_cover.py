"""CPU restatement of the keyframe coverage (ebvo_keyframe_cover_edges / ebvo_temporal_keyframe_cover), of the switch policy
(ebvo_keyframe_decide) and of the pose bookkeeping of the frame step -- the checker of the device kernels (test
infrastructure).  The contract is written once in include/ebvo_hip.h; this file follows it operation by operation, one numpy
ufunc per arithmetic operation (IEEE double, no FMA).  Gamma per mate, the scaling by lambda, the projection, the mapped
orientation, the association and the residual are tests/oracle_align.py's and tests/oracle_depth.py's, camera 0 only.
"""
from __future__ import annotations

import math

import numpy as np

from tests import oracle_align as oa
from tests import oracle_depth as od
from tests import oracle_tgt as ot

DEFAULTS = dict(radius=4.0, orient_thr_deg=10.0, img_margin=10.0, inlier_px=1.0, bin_px=1.0, cell_size=4, cover_cell=32,
                min_cell_edges=4, min_cell_explained=2)
POLICY = dict(min_assoc=50, max_disp_bins=30, min_in_frame_share=0.7, min_assoc_share=0.5, min_cell_cover=0.6)
DEAD, IN_FRAME, ASSOCIATED, INLIER = 1, 2, 4, 8
LOST, LOW_OVERLAP, LOW_ASSOC, NEW_CONTENT, PARALLAX = 1, 2, 4, 8, 16
BINS = 64
INT_FIELDS = ("n_kf", "n_dead", "n_in_frame", "n_assoc", "n_inliers", "n_edges", "n_explained", "cw", "ch", "n_cells_cur",
              "n_cells_covered", "disp_median_bin")
ARRAYS = ("flags", "assoc", "disp", "explained", "cell_edges", "cell_explained", "hist")


def coarse_cells(E, img_w, img_h, cell):
    """(cw, ch, c): the coarse cell cy * cw + cx of every edge by grid_cell's rule, -1 for an edge in no cell"""
    cw, ch = (img_w + cell - 1) // cell, (img_h + cell - 1) // cell
    x, y = np.asarray(E["x"], dtype=np.float64), np.asarray(E["y"], dtype=np.float64)
    with np.errstate(all="ignore"):
        ok = (x > -float(cell)) & (x < float(cw) * float(cell)) & (y > -float(cell)) & (y < float(ch) * float(cell))
    xi = np.trunc(np.where(ok, x, 0.0)).astype(np.int64)          # (int)v: towards zero
    yi = np.trunc(np.where(ok, y, 0.0)).astype(np.int64)
    cx = np.where(xi < 0, 0, xi // cell)                          # C division: (-cell, 0] / cell = 0
    cy = np.where(yi < 0, 0, yi // cell)
    return cw, ch, np.where(ok, cy * cw + cx, -1)


def median_bin(hist, n_in_frame):
    if n_in_frame <= 0:
        return -1
    run = 0
    for b in range(BINS):
        run += int(hist[b])
        if 2 * run >= n_in_frame:
            return b
    return -1


def cover(kf_left, kf_right, lambda_, edges_left, img_w, img_h, calib, R, t, **params):
    """The coverage on host arrays.  calib = (K_left, K_right, R21, T21); lambda_: None or one double per mate.  Returns the
    fields of ebvo_keyframe_cover, the six output arrays, `residual` (r per mate, NaN where not associated) and `assoc_raw` (the
    alignment's association before the dead mates are taken out)."""
    p = dict(DEFAULTS, **params)
    ap = dict(oa.DEFAULTS, radius=p["radius"], cell_size=p["cell_size"], orient_thr_deg=p["orient_thr_deg"], img_margin=p["img_margin"],
              cameras=1)
    sc = od.DepthScene(kf_left, kf_right, edges_left, None, img_w, img_h, calib, ap, lambda_=lambda_)
    n, E = sc.n, sc.E[0]
    n0 = len(E)
    cw, ch, cell_of = coarse_cells(E, img_w, img_h, p["cover_cell"])
    out = dict(n_kf=n, n_dead=0, n_in_frame=0, n_assoc=0, n_inliers=0, n_edges=n0, n_explained=0, cw=cw, ch=ch, n_cells_cur=0,
               n_cells_covered=0, disp_median_bin=-1, hist=np.zeros(BINS, dtype=np.int32), flags=np.zeros(n, dtype=np.uint8),
               assoc=np.full(n, -1, dtype=np.int32), disp=np.full(n, np.nan), explained=np.zeros(n0, dtype=np.uint8),
               cell_edges=np.zeros(cw * ch, dtype=np.int32), cell_explained=np.zeros(cw * ch, dtype=np.int32),
               residual=np.full(n, np.nan), assoc_raw=np.full(n, -1, dtype=np.int32))
    if n == 0 or n0 == 0:                                         # nothing launched
        return out
    Rt = tuple(float(v) for v in np.asarray(R, dtype=np.float64).reshape(9))
    tt = tuple(float(v) for v in np.asarray(t, dtype=np.float64).reshape(3))
    dead = ~od.live_mates(sc.G0)
    m, x_max, y_max = float(p["img_margin"]), float(img_w) - float(p["img_margin"]), float(img_h) - float(p["img_margin"])
    with np.errstate(all="ignore"):
        pr = ot.project(sc.kfL, sc.kfR, np.array(Rt).reshape(3, 3), np.array(tt), sc.calib, img_w, img_h, kf_gamma=sc.G,
                        img_margin=p["img_margin"])
        q = pr["proj_left"]
        X = ot._mv(ot._m(np.array(Rt).reshape(3, 3)), sc.G)
        z = X[:, 2] + tt[2]
        in_frame = ~dead & (q[:, 0] > m) & (q[:, 1] > m) & (q[:, 0] < x_max) & (q[:, 1] < y_max) & (z > 0.0)
        raw = sc.associate(Rt, tt)[0]
        a = np.where(in_frame, raw, -1).astype(np.int32)          # a dead mate takes no part; a live one is associated in frame only
        r, _, rho, _ = sc._camera(0, Rt, tt, [a, None])
        has = a >= 0
        inl = has & (rho < float(p["inlier_px"]))
        dx, dy = q[:, 0] - sc.kfL["x"], q[:, 1] - sc.kfL["y"]
        d = np.sqrt(np.add(dx * dx, dy * dy))
        b = d / float(p["bin_px"])
        bins = np.where(b >= 63.0, 63, np.trunc(np.where(b >= 63.0, 0.0, b))).astype(np.int64)
    out["flags"] = (np.where(dead, DEAD, 0) | np.where(in_frame, IN_FRAME, 0) | np.where(has, ASSOCIATED, 0) |
                    np.where(inl, INLIER, 0)).astype(np.uint8)
    out["assoc"] = a
    out["assoc_raw"] = raw                                        # what the alignment's association alone says (dead mates included)
    out["disp"] = np.where(in_frame, d, np.nan)
    out["residual"] = np.where(has, r, np.nan)
    out["hist"] = np.bincount(bins[in_frame], minlength=BINS).astype(np.int32)
    out["explained"][a[has]] = 1
    inc = cell_of >= 0
    out["cell_edges"] = np.bincount(cell_of[inc], minlength=cw * ch).astype(np.int32)
    out["cell_explained"] = np.bincount(cell_of[inc & (out["explained"] != 0)], minlength=cw * ch).astype(np.int32)
    cur = out["cell_edges"] >= p["min_cell_edges"]
    out.update(n_dead=int(dead.sum()), n_in_frame=int(in_frame.sum()), n_assoc=int(has.sum()), n_inliers=int(inl.sum()),
               n_explained=int(out["explained"].sum()), n_cells_cur=int(cur.sum()),
               n_cells_covered=int((cur & (out["cell_explained"] >= p["min_cell_explained"])).sum()))
    out["disp_median_bin"] = median_bin(out["hist"], out["n_in_frame"])
    return out


def decide(c, **policy):
    """(decision, reasons) of ebvo_keyframe_decide on a record (a dict of its integers)"""
    p = dict(POLICY, **policy)
    r = 0
    if c["n_assoc"] < p["min_assoc"]:
        r |= LOST
    if float(c["n_in_frame"]) < p["min_in_frame_share"] * float(c["n_kf"] - c["n_dead"]):
        r |= LOW_OVERLAP
    if float(c["n_assoc"]) < p["min_assoc_share"] * float(c["n_in_frame"]):
        r |= LOW_ASSOC
    if float(c["n_cells_covered"]) < p["min_cell_cover"] * float(c["n_cells_cur"]):
        r |= NEW_CONTENT
    if c["disp_median_bin"] >= p["max_disp_bins"]:
        r |= PARALLAX
    return (2 if r & LOST else 1 if r else 0), r


def compose(R, t, Rk, tk):
    """(R Rk, mv3(R, tk) + t) with the sums written out in mv3's order: (a b + c d) + e f per entry, no matrix product"""
    R, Rk = np.asarray(R, dtype=np.float64).reshape(3, 3), np.asarray(Rk, dtype=np.float64).reshape(3, 3)
    t, tk = np.asarray(t, dtype=np.float64).reshape(3), np.asarray(tk, dtype=np.float64).reshape(3)
    Ro, to = np.zeros((3, 3)), np.zeros(3)
    for i in range(3):
        for j in range(3):
            Ro[i, j] = np.float64(np.float64(np.float64(R[i, 0] * Rk[0, j]) + np.float64(R[i, 1] * Rk[1, j])) + np.float64(R[i, 2] * Rk[2, j]))
        to[i] = np.float64(np.float64(np.float64(R[i, 0] * tk[0]) + np.float64(R[i, 1] * tk[1])) + np.float64(R[i, 2] * tk[2])) + t[i]
    return Ro, to
