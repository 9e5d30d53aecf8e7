"""Inputs of the temporal ground-truth tests (tests/test_tgt_oracle.py, tests/test_gpu_tgt.py) and their oracle side
(tests/oracle_tgt.py).  Everything here runs on the CPU.

Host-array scenes: oracle_pose.synthetic_quads of the known motion of tests/pose_scenes.py; the keyframe mates are the rows,
the current-frame mates are the quads' edges (one mate per quad).  Border scenes: a hand-made rig and an identity pose, so
that a keyframe mate projects onto itself and the current-frame mates can be placed around it.
Resident scenes: the frames of tests/temporal_cases.py.  Frame k is frame 0 moved k px along x at a constant disparity of
9 px, i.e. a camera translation of k * baseline / 9 along -x of the scene; POSE_SHIFT_PX chooses how much of it the pose
given to the device accounts for (found on the CPU so that the counts in EXPECTED hold).
"""
import functools
import math

import numpy as np

from tests import oracle as orc
from tests import oracle_chain
from tests import oracle_gt as og
from tests import oracle_pose as op
from tests import oracle_tgt as ot
from tests import pose_scenes as ps
from tests import temporal_cases as tc

# name: (n_kf, rig, cell size).  kitti: 1214 x 370 px -> 2025 cells of 15 px (more than a block's 256 threads), 52 cells
# of 100 px (fewer); euroc: 734 x 496 -> 1650 / 40 cells
HOST_CASES = {
    "kf1": (1, "kitti", 15),
    "kf3": (3, "euroc", 100),
    "kf63": (63, "kitti", 100),
    "kf64": (64, "euroc", 15),
    "kf65": (65, "kitti", 15),
    "kf257": (257, "euroc", 100),
    "kf257-fine": (257, "kitti", 15),
}


@functools.lru_cache(maxsize=None)
def host_scene(name):
    n_kf, rig, cell = HOST_CASES[name]
    K, _, R21, T21 = ps.rig(rig)
    calib = (K, K, R21, T21)
    for n_quads in range(n_kf, 2 * n_kf + 2):       # rows hold one or two quads: the first n_quads that gives n_kf rows
        q = op.synthetic_quads(n_quads, 0.3, (K, R21, T21), ps.R_GT, ps.T_GT, seed=n_kf)
        if len(q[2]) - 1 == n_kf:
            break
    kfL, kfR, row_ptr, cfL, cfR, inl = q
    assert len(kfL) == n_kf
    w, h = int(round(2 * K[0, 2])), int(round(2 * K[1, 2]))
    return dict(kfL=kfL, kfR=kfR, row_ptr=row_ptr, cfL=cfL, cfR=cfR, inl=inl, calib=calib, w=w, h=h, cell=cell, R=ps.R_GT, t=ps.T_GT)


@functools.lru_cache(maxsize=None)
def host_reference(name):
    s = host_scene(name)
    return ot.build_veridical_quads(s["kfL"], s["kfR"], s["cfL"], s["cfR"], s["R"], s["t"], s["calib"], s["w"], s["h"],
                                    cell=s["cell"])


# ---- border scenes -----------------------------------------------------------------------------------------------------
B_W, B_H, B_CELL = 200, 120, 15
B_K = np.array([[100.0, 0, 100.0], [0, 100.0, 60.0], [0, 0, 1.0]])
B_CALIB = (B_K, B_K, np.eye(3), np.array([-0.5, 0.0, 0.0]))     # disparity 10 px at depth 5
B_R, B_T = np.eye(3), np.zeros(3)


def _mate(x, y, theta, disp=10.0):
    l, r = np.zeros(1, dtype=orc.EDGE_DTYPE), np.zeros(1, dtype=orc.EDGE_DTYPE)
    l["x"], l["y"], l["theta"] = x, y, theta
    r["x"], r["y"], r["theta"] = x - disp, y, theta
    return l, r


def _stack(mates):
    return np.concatenate([m[0] for m in mates]), np.concatenate([m[1] for m in mates])


def _wrap(a):
    return math.atan2(math.sin(a), math.cos(a))


@functools.lru_cache(maxsize=None)
def border_scene(which):
    """margin: keyframe mates whose projections straddle the 10 px margin on every side of both cameras;
    cells: projections on both sides of a cell border, current-frame mates in the next cells; with a wide tp_dist the cell
           sets alone decide, and one current-frame mate is in the left cell set only;
    orient: current-frame mates at the projection with orientation offsets around 0, 180 and 360 degrees."""
    if which == "margin":
        xs = [(20.4, 60.0), (20.6, 60.0), (19.9, 60.0), (50.0, 9.7), (50.0, 10.3), (189.6, 60.0), (190.4, 60.0), (50.0, 109.7),
              (50.0, 110.3), (100.0, 60.0)]         # the right projection is 10 px to the left: x = 20.x puts it on the margin
        kf = [_mate(x, y, 1.2) for x, y in xs]
        cf = [_mate(x + 0.3, y - 0.2, 1.2) for x, y in xs]
        return dict(kf=_stack(kf), cf=_stack(cf), params={})
    if which == "cells":
        kf = [_mate(59.9, 45.1, 1.0), _mate(60.1, 44.9, 1.0), _mate(120.5, 75.5, 1.0)]
        cf = [_mate(x, y, 1.0) for x in (14.0, 29.9, 30.0, 59.0, 89.9, 90.0, 105.0, 151.0) for y in (14.9, 15.0, 44.0, 74.9, 75.0, 106.0)]
        l, r = _mate(61.0, 46.0, 1.0)
        r["x"] = 150.0                              # left edge next to the first projections, right edge ten cells away
        cf.append((l, r))
        return dict(kf=_stack(kf), cf=_stack(cf), params=dict(tp_dist=1000.0))
    assert which == "orient"
    spots = ((80.0, 50.0, 3.1), (120.0, 70.0, -0.4), (60.0, 90.0, 0.04))   # the third maps next to -pi: offsets wrap past 360
    kf = [_mate(*sp) for sp in spots]
    degs = (0.0, 5.0, 9.9, 10.1, 15.0, -5.0, -9.9, -10.1, 165.0, 170.1, 175.0, 180.0, 185.0, 189.9, 190.1, -175.0, 90.0)
    cf = [_mate(x + 0.5, y, _wrap(th + math.radians(d))) for (x, y, th) in spots for d in degs]
    return dict(kf=_stack(kf), cf=_stack(cf), params={})


@functools.lru_cache(maxsize=None)
def border_reference(which):
    s = border_scene(which)
    return ot.build_veridical_quads(*s["kf"], *s["cf"], B_R, B_T, B_CALIB, B_W, B_H, cell=B_CELL, **s["params"])


# ---- resident scenes ---------------------------------------------------------------------------------------------------
# name: (keyframe, current frame, px of the 2 px image motion the pose accounts for)
RESIDENT = {
    "small": ("small0", "small2", 1.25),
    "euroc-half": ("kf", "cf2", 1.25),
}


# The half-scale EuRoC rig does not describe these synthetic frames (they move along x only), so the keyframe's mates lie 6 to
# 38 px from the GT location of the constant-disparity map and the reference's 1 px (DIST_TO_GT_THRESH, :1645) would mark none
# of them: the kf_is_tp bytes given to the feature are formed with 12 px, which marks about half and so exercises the gate.
KF_TP_DIST = 12.0


def resident_pose(px):
    """camera motion that moves a point at the scene's depth (disparity 9) by `px` along x in the image"""
    _, calib = tc.rig()
    b = -float(np.asarray(calib[3])[0])
    return np.eye(3), np.array([px * b / 9.0, 0.0, 0.0])


@functools.lru_cache(maxsize=None)
def keyframe_gt(kf):
    """kf_gamma / kf_is_tp of the keyframe's mates as the reference forms them (src/Stereo_Matches.cpp:186, :1638, :1645) from
    a constant-disparity map: Find_Stereo_GT_Locations at the mate's left edge (tests/oracle_gt.py).  The reference's mates
    are focused rows; the half-scale EuRoC rig is not rectified while the frames move along x only, so no row of these frames
    is focused (no right edge within 0.5 px of a slanted epipolar line AND 1 px of the GT location): the rows with a VALID
    GT location are used instead; the others get (-1, -1, -1) / 0, the fill values of ebvo_gt_locate."""
    l, _ = tc.images(kf)
    _, calib = tc.rig()
    L, Rm = tc.oracle_mates(kf)
    disp = og.disparity_map(*l.shape, 9)
    loc = og.find_gt_locations(L, disp, calib[0], calib[2], calib[3])
    dx, dy = Rm["x"] - loc["gt_xy"][:, 0], Rm["y"] - loc["gt_xy"][:, 1]
    is_tp = ((loc["valid"] != 0) & (np.sqrt(dx * dx + dy * dy) <= KF_TP_DIST)).astype(np.uint8)
    return dict(disp=disp, loc=loc, gamma=np.ascontiguousarray(loc["gamma_left"]), is_tp=is_tp)


@functools.lru_cache(maxsize=None)
def resident_reference(name, stages, with_gt):
    """the oracle's veridical quads and the three stage evaluations of a resident case"""
    kf, cf, px = RESIDENT[name]
    h, w = tc.FRAMES[cf][:2]
    _, calib = tc.rig()
    R, t = resident_pose(px)
    (kfL, kfR), (cfL, cfR) = tc.oracle_mates(kf), tc.oracle_mates(cf)
    ref = tc.reference(kf, cf, None, bool(stages))
    g = keyframe_gt(kf) if with_gt else None
    ver = ot.build_veridical_quads(kfL, kfR, cfL, cfR, R, t, calib, w, h, kf_gamma=g["gamma"] if g else None)
    on = ot.row_on(ver["ver_row_ptr"], g["is_tp"] if g else None)
    rp, col, keep = ref["row_ptr"], ref["col_idx"], ref["keep"].astype(bool)
    out = {ot.ORIENTATION: ot.evaluate_stage(rp, cfL[col], cfR[col], on, ver),
           ot.NCC: ot.evaluate_stage(oracle_chain.filter_rows(rp, keep), cfL[col[keep]], cfR[col[keep]], on, ver)}
    if stages:
        f = ref["final"]
        out[ot.CLUSTER] = ot.evaluate_stage(f["row_ptr"], f["left"], f["right"], on, ver)
    return dict(ver=ver, on=on, stages=out, R=R, t=t, calib=calib, gt=g, ref=ref)


def resident_counts(name, with_gt):
    r = resident_reference(name, 1, with_gt)
    fl = r["stages"][ot.CLUSTER][1]
    return dict(n_kf=len(r["on"]), n_rows=int((np.diff(r["ver"]["ver_row_ptr"]) > 0).sum()), n_on=int(r["on"].sum()),
                n_veridical=int(r["ver"]["ver_row_ptr"][-1]), final_tp=int(fl.sum()), final_not_tp=int(len(fl) - fl.sum()))


# what the oracle gives for the poses above, as tests/test_tgt_oracle.py recomputes it
EXPECTED = {
    ("small", False): dict(n_kf=1175, n_rows=573, n_on=573, n_veridical=1314, final_tp=462, final_not_tp=303),
    ("small", True): dict(n_kf=1175, n_rows=95, n_on=82, n_veridical=194, final_tp=55, final_not_tp=710),
    ("euroc-half", False): dict(n_kf=4884, n_rows=2298, n_on=2298, n_veridical=5656, final_tp=1938, final_not_tp=1367),
    ("euroc-half", True): dict(n_kf=4884, n_rows=444, n_on=404, n_veridical=970, final_tp=282, final_not_tp=3023),
}
