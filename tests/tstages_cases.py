"""Inputs of the stage-trail tests (tests/test_tstages_oracle.py, tests/test_gpu_tstages.py) and their oracle side
(tests/oracle_tstages.py, tests/oracle_tgt.py).  Everything here runs on the CPU.

Resident scenes: those of tests/tgt_cases.py (the frames of tests/temporal_cases.py, the pose of tgt_cases.RESIDENT) under
two parameter sets -- the defaults, at which BNB-NCC reorders rows but removes nothing, and a bnb_ncc at which it removes
quads -- plus the parameter sets that leave a stage empty.
Grid scenes: hand-made mates on a 200 x 120 frame with cells of 15 px (14 x 8 cells) for ebvo_tgt_grid_rows.
"""
import functools

import numpy as np

from tests import oracle as orc
from tests import oracle_tgt as ot
from tests import oracle_tstages as ots
from tests import temporal_cases as tc
from tests import tgt_cases as cases

INTERIOR = (ot.SIFT, ot.BNB_NCC, ot.BNB_SIFT, ot.REFINE)
TRAIL_COUNT = {ot.SIFT: "n_sift", ot.BNB_NCC: "n_bnb_ncc", ot.BNB_SIFT: "n_bnb_sift", ot.REFINE: "n_bnb_sift"}
CELL, RADIUS = 15, 30.0          # ebvo_temporal_params' defaults

# name: parameters of the match (ebvo_temporal_params' names).  tight-bnb-ncc: tests/test_tstages_oracle.py asserts that the
# oracle's BNB-NCC removes quads from the evaluated rows at this value (it removes none at the default 0.8)
PARAMS = {"default": {}, "tight-bnb-ncc": dict(bnb_ncc=0.95)}
ORACLE_NAME = dict(sift_thr="sift_thr", bnb_ncc="bnb_ncc", bnb_sift="bnb_sift", ncc_thr="ncc_thr")


@functools.lru_cache(maxsize=None)
def chain(name, pset):
    """(final, trail) of oracle_tstages.temporal_edge_pairs_trail for a resident case under a parameter set"""
    kf, cf, _ = cases.RESIDENT[name]
    kw = {ORACLE_NAME[k]: v for k, v in PARAMS[pset].items()}
    ref = tc.reference(kf, cf, None, False, **({"ncc_thr": kw["ncc_thr"]} if "ncc_thr" in kw else {}))
    kw.pop("ncc_thr", None)
    return ots.temporal_edge_pairs_trail(*tc.oracle_mates(kf), *tc.oracle_mates(cf), tc.triple(kf)[1:], tc.triple(cf)[1:],
                                         ref["row_ptr"], ref["col_idx"], ref["sim_left"], ref["keep"], **kw)


@functools.lru_cache(maxsize=None)
def resident_reference(name, pset, stages, with_gt):
    """The oracle's evaluation of every stage a match with the trail on reports: stages[k] = (n_tp, flags or None, metrics).
    ver / on / R / t / calib / gt are tgt_cases.resident_reference's (they do not depend on the chain's parameters)."""
    base = cases.resident_reference(name, 0, with_gt)
    kf, cf, _ = cases.RESIDENT[name]
    h, w = tc.FRAMES[cf][:2]
    (kfL, kfR), (cfL, cfR) = tc.oracle_mates(kf), tc.oracle_mates(cf)
    ver, on = base["ver"], base["on"]
    out = dict(base["stages"])                                    # ORIENTATION, NCC
    g = ots.grid_rows(kfL, kfR, cfL, cfR, w, h, CELL, RADIUS, on, ver["proj_left"], ver["proj_right"])
    out[ot.GRID] = (g, None, ot.metrics(g, on))
    trail = None
    if stages:
        final, trail = chain(name, pset)
        for k in INTERIOR:
            t = trail[k]
            out[k] = ot.evaluate_stage(t["row_ptr"], t["left"], t["right"], on, ver)
        out[ot.CLUSTER] = ot.evaluate_stage(final["row_ptr"], final["left"], final["right"], on, ver)
    return dict(base, stages=out, trail=trail)


def empty_reference(name, n_kf):
    """what every stage from an empty one on reports: the rows that are on, all empty -- the four zeros"""
    on = cases.resident_reference(name, 0, False)["on"]
    return on, ot.metrics(np.zeros((n_kf, 2), dtype=np.int32), on)


# ---- grid scenes -------------------------------------------------------------------------------------------------------
G_W, G_H = 200, 120
G_GW, G_GH = 14, 8
POPULATIONS = {(2, 2): 1, (4, 2): 15, (6, 2): 16, (8, 2): 17, (10, 2): 33, (0, 0): 2, (13, 7): 3, (2, 5): 4}   # left cell: mates


def _edges(xy, theta=0.5):
    e = np.zeros(len(xy), dtype=orc.EDGE_DTYPE)
    if len(xy):
        a = np.asarray(xy, dtype=np.float64)
        e["x"], e["y"], e["theta"] = a[:, 0], a[:, 1], theta
    return e


def _current_frame():
    """mates filling the cells of POPULATIONS (quarter-pixel coordinates: every difference below is exact), the right edge
    10 px to the left (in the same cell row; the corner cell's right edges stay at x >= 0.25)"""
    left, right = [], []
    for (cx, cy), pop in POPULATIONS.items():
        for k in range(pop):
            x, y = cx * CELL + 0.25 + (k % 8) * 1.75, cy * CELL + 0.5 + (k // 8) * 2.5
            left.append((x, y))
            right.append((max(x - 10.0, 0.25 + k), y))
    return left, right


def grid_scene(name):
    """dict(kfL, kfR, cfL, cfR, on, pl, pr, radius, tp_dist) on the G_W x G_H frame, cells of CELL px"""
    return dict(_grid_scene(name))


@functools.lru_cache(maxsize=None)
def _grid_scene(name):
    left, right = _current_frame()
    radius, tp_dist = RADIUS, 2.0
    if name.startswith("kf"):                                     # kf1 ... kf65: keyframe mates over the populated cells in turn
        n_kf = int(name[2:])
        spots = list(POPULATIONS)
        first = {c: sum(p for cc, p in list(POPULATIONS.items())[:k]) for k, (c, _) in enumerate(POPULATIONS.items())}
        kl, kr, pl, pr = [], [], [], []
        for i in range(n_kf):
            c = spots[i % len(spots)]
            j = first[c] + (i // len(spots)) % POPULATIONS[c]     # the mate the row's projections sit next to
            kl.append((c[0] * CELL + 7.0 + 0.25 * (i % 5), c[1] * CELL + 6.0))
            kr.append((max(kl[-1][0] - 10.0, 0.5), kl[-1][1]))
            pl.append((left[j][0] + 0.5, left[j][1] - 0.25))
            pr.append((right[j][0] + 0.5, right[j][1] - 0.25))
        on = np.ones(n_kf, dtype=np.uint8)
        if n_kf > 2:
            on[2] = 0                                             # a row that is off
        return _scene(kl, kr, left, right, on, pl, pr, radius, tp_dist)
    if name in ("radius0", "radius-wide"):
        s = dict(_grid_scene("kf17"))
        s["radius"] = 0.0 if name == "radius0" else 5000.0
        return tuple(s.items())
    if name == "no-cf":
        s = dict(_grid_scene("kf5"))
        s["cfL"] = s["cfR"] = _edges([])
        return tuple(s.items())
    if name == "no-kf":
        s = dict(_grid_scene("kf5"))
        s["kfL"] = s["kfR"] = _edges([])
        s["on"], s["pl"], s["pr"] = np.zeros(0, dtype=np.uint8), np.zeros((0, 2)), np.zeros((0, 2))
        return tuple(s.items())
    assert name == "edges"
    left = left + [(100.5, 50.5), (101.5, 50.5), (120.0, 70.0), (130.0, 130.0)]
    right = right + [(90.5, 50.5), (91.5, 50.5), (-20.0, 70.0), (120.0, 70.0)]
    #             exactly tp_dist away / inside it; right edge outside the right grid; left edge outside the left grid
    rows = [
        # keyframe left, right, projection left, right
        ((1.0, 1.0), (0.5, 1.0), (0.75, 0.75), (0.75, 0.75)),                  # 0 a corner cell
        ((199.0, 119.0), (189.0, 119.0), (196.0, 110.0), (186.0, 110.0)),      # 1 the opposite corner
        ((300.0, 50.0), (290.0, 50.0), (100.0, 50.0), (90.0, 50.0)),           # 2 query cell 20: clipped to nothing at sr = 2
        ((-50.0, 50.0), (-60.0, 50.0), (100.0, 50.0), (90.0, 50.0)),           # 3 query cell -3: clipped to nothing
        ((215.0, 110.0), (205.0, 110.0), (196.0, 110.0), (186.0, 110.0)),      # 4 query cell 14 = gw: reaches cells 12, 13
        ((100.0, 50.0), (90.0, 50.0), (98.5, 50.5), (88.5, 50.5)),             # 5 a mate at exactly tp_dist, one at 3
        ((100.0, 50.0), (90.0, 50.0), (99.5, 50.5), (89.5, 50.5)),             # 6 the same mates at 1 and 2: one true positive
        ((100.0, 50.0), (90.0, 50.0), (np.nan, 50.5), (89.5, 50.5)),           # 7 a NaN projection: counted, never a true positive
        ((100.0, 50.0), (90.0, 50.0), (99.5, 50.5), (89.5, 50.5)),             # 8 off
        ((120.0, 70.0), (110.0, 70.0), (120.0, 70.0), (110.0, 70.0)),          # 9 next to the mate whose right edge is outside
        ((130.0, 115.0), (120.0, 115.0), (130.0, 130.0), (120.0, 70.0)),       # 10 next to the mate whose left edge is outside
    ]
    on = np.ones(len(rows), dtype=np.uint8)
    on[8] = 0
    return _scene([r[0] for r in rows], [r[1] for r in rows], left, right, on, [r[2] for r in rows], [r[3] for r in rows], radius,
                  tp_dist)


def _scene(kl, kr, left, right, on, pl, pr, radius, tp_dist):
    return tuple(dict(kfL=_edges(kl), kfR=_edges(kr), cfL=_edges(left), cfR=_edges(right), on=on,
                      pl=np.asarray(pl, dtype=np.float64).reshape(-1, 2), pr=np.asarray(pr, dtype=np.float64).reshape(-1, 2),
                      radius=radius, tp_dist=tp_dist).items())


GRID_SCENES = ["kf1", "kf3", "kf4", "kf5", "kf15", "kf16", "kf17", "kf65", "radius0", "radius-wide", "edges", "no-cf", "no-kf"]


@functools.lru_cache(maxsize=None)
def grid_reference(name):
    s = grid_scene(name)
    n_tp = ots.grid_rows(s["kfL"], s["kfR"], s["cfL"], s["cfR"], G_W, G_H, CELL, s["radius"], s["on"], s["pl"], s["pr"], s["tp_dist"])
    return n_tp, ot.metrics(n_tp, s["on"])


def left_cell_populations(cfL):
    cx, cy = tc.cells_of(cfL["x"], CELL), tc.cells_of(cfL["y"], CELL)
    ok = (cx >= 0) & (cx < G_GW) & (cy >= 0) & (cy < G_GH)
    return np.bincount((cy * G_GW + cx)[ok], minlength=G_GW * G_GH)
