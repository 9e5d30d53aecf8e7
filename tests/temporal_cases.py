"""The frames of the temporal edge tests (tests/test_gpu_temporal_edges.py, tests/test_temporal_cases.py) and their oracle
side: the EuRoC-half scene of tests/test_gpu_temporal.py at several sizes, blanked or cropped so that the mate counts and
the cell populations fall on the work units of the temporal kernels.  Everything here runs on the CPU (tests/oracle.py,
tests/oracle_chain.py); the mates of a frame are the oracle's stereo chain, which the device's stereo chain is pinned to by
the other GPU files."""
import functools

import numpy as np

from edge_based_visual_odometry_amd import synth
from tests import oracle as orc
from tests import oracle_chain

H, W = 240, 376          # the scene of tests/test_gpu_temporal.py
SMALL = (120, 200)       # the second frame size of the size tests


def rig():
    """(F, calib) of the half-scale EuRoC rig, no undistortion"""
    ce = synth.CALIB["euroc"]
    K, Kr = tuple(v / 2 for v in ce["K"]), tuple(v / 2 for v in ce["K_right"])
    F = synth.fundamental_21(K, Kr, ce["R21"], ce["T21"])
    calib = ([K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1], [Kr[0], 0, Kr[2], 0, Kr[1], Kr[3], 0, 0, 1], ce["R21"], ce["T21"])
    return F, calib


# name: (h, w, frame index k, box (y0, y1, x0, x1) kept or None).  Frame k of SURVEY 8(d) config 3: scene 7, noise seeds
# (2k + 1, 2k + 2), k px of global motion; outside the box both images are flat 128 (no edge, no mate).
# The boxes were searched on the CPU (tools/search_temporal_cases.py) for the counts in EXPECTED.
FRAMES = {
    "kf": (H, W, 0, None),
    "cf2": (H, W, 2, None),
    "cf3": (H, W, 3, None),
    "small0": (*SMALL, 0, None),
    "small2": (*SMALL, 2, None),
    "sq0": (160, 160, 0, None),
    "sq2": (160, 160, 2, None),
    # keyframes: n_kf = 80 (0 mod 16), 209 (1 mod 16), 239 (15 mod 16, 3 mod 4), 66 (2 mod 4), 3 and 1 (less than one wave's four)
    "k80": (*SMALL, 0, (0, 120, 0, 26)),
    "k209": (*SMALL, 0, (0, 120, 0, 52)),
    "k239": (*SMALL, 0, (0, 120, 0, 62)),
    "k66": (*SMALL, 0, (0, 120, 0, 24)),
    "k3": (*SMALL, 0, (20, 36, 44, 60)),
    "k1": (*SMALL, 0, (8, 24, 68, 84)),
    # current frames: n_cf = 80, 209, 95 (0, 1, 15 mod 16), 15 and 1 (less than one block's sixteen)
    "c80": (*SMALL, 2, (0, 120, 0, 26)),
    "c209": (*SMALL, 2, (0, 120, 0, 54)),
    "c95": (*SMALL, 2, (0, 120, 0, 36)),
    "c15": (*SMALL, 2, (32, 48, 128, 144)),
    "c1": (*SMALL, 2, (8, 24, 140, 156)),
}

# name: (keyframe, current frame, cell size, stages)
UNIT_CASES = {
    "kf80-cf209": ("k80", "c209", 15, 1),
    "kf209-cf95": ("k209", "c95", 15, 1),
    "kf239-cf80": ("k239", "c80", 15, 1),
    "kf66": ("k66", "small2", 15, 1),
    "kf3": ("k3", "small2", 15, 1),
    "kf1": ("k1", "small2", 15, 1),
    "cf15": ("small0", "c15", 15, 1),
    "cf1": ("small0", "c1", 15, 1),
    "cells-104-crowded": ("kf", "cf2", 30, 1),      # fewer cells than cell_scan's 256 threads; cells of 64, 65 and more mates
    "cells-256": ("sq0", "sq2", 10, 1),             # one cell per thread of cell_scan
    "cells-375": ("small0", "small2", 8, 1),        # two cells per thread, the last threads idle
}


def add_boxed(frames):
    FRAMES.update(frames)


@functools.lru_cache(maxsize=None)
def images(name):
    h, w, k, box = FRAMES[name]
    l, r = synth.stereo_pair("s2", h, w, scene=7, noise_base=2 * k, disparity=9)
    l, r = np.roll(l, k, axis=1), np.roll(r, k, axis=1)
    if box is not None:
        y0, y1, x0, x1 = box
        for img in (l, r):
            keep = img[y0:y1, x0:x1].copy()
            img[:] = 128
            img[y0:y1, x0:x1] = keep
    return np.ascontiguousarray(l), np.ascontiguousarray(r)


@functools.lru_cache(maxsize=None)
def oracle_mates(name):
    """(left TOED edge, final right edge) of every final pair of the oracle's stereo chain (no SIFT stages)"""
    l, r = images(name)
    F, calib = rig()
    ch = oracle_chain.stereo_edge_pairs(l, r, F, calib)
    return ch["left"][ch["left_index"]], ch["right"]


def triple(name):
    """(raw left, undistorted left, undistorted right): no distortion here"""
    l, r = images(name)
    return l, l, r


def cells_of(v, cell):
    """(int)v / cell, truncating towards zero as C does"""
    return np.trunc(np.trunc(v) / cell).astype(np.int64)


def cell_populations(name, cell):
    """population of every LEFT grid cell of the frame's mates (mates outside the grid are in no cell)"""
    h, w = FRAMES[name][:2]
    L, _ = oracle_mates(name)
    gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
    cx, cy = cells_of(L["x"], cell), cells_of(L["y"], cell)
    ok = (cx >= 0) & (cx < gw) & (cy >= 0) & (cy < gh)
    return np.bincount((cy * gw + cx)[ok], minlength=gw * gh), gw * gh


def conditions(kf, cf, cell=15):
    """the counts the tests put on a (keyframe, current frame, cell size) case, from the oracle alone"""
    pop, n_cells = cell_populations(cf, cell)
    return dict(n_kf=len(oracle_mates(kf)[0]), n_cf=len(oracle_mates(cf)[0]), n_cells=n_cells, max_cell=int(pop.max()),
                cells_64_65=int(((pop == 64) | (pop == 65)).sum()),
                n_candidates=reference(kf, cf, None, False, cell=cell)["counts"]["n_candidates"])


def rows_outside_grid(kf, cf, cell=15, sr=2):
    """(keyframe mates whose left query cell lies outside the current frame's grid, those among them whose walk is clipped to
    nothing: dx1 < dx0 or dy1 < dy0 in temporal_candidates_kernel)"""
    h, w = FRAMES[cf][:2]
    L, _ = oracle_mates(kf)
    gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
    qx, qy = cells_of(L["x"], cell), cells_of(L["y"], cell)
    outside = (qx >= gw) | (qy >= gh)
    empty = (qx > gw - 1 + sr) | (qy > gh - 1 + sr)
    return np.flatnonzero(outside), np.flatnonzero(empty)


@functools.lru_cache(maxsize=None)
def reference(kf, cf, size=None, chain=True, **kw):
    """oracle_chain.temporal_reference of two named frames; size = (w, h) of the CURRENT frame (its own by default)"""
    h, w = FRAMES[cf][:2]
    w, h = size or (w, h)
    return oracle_chain.temporal_reference(*oracle_mates(kf), *oracle_mates(cf), triple(kf), triple(cf), w, h, chain=chain, **kw)


@functools.lru_cache(maxsize=None)
def sift_levels(kf, cf):
    """Ascending distinct values of max(left, right SIFT distance) over the quads that pass the default NCC filter: a quad
    passes apply_SIFT_filtering_quads iff its value is BELOW sift_thr, so sift_thr = levels[k] keeps exactly the quads of the
    k smallest levels (none for k = 0)."""
    ref = reference(kf, cf, chain=False)
    (kfL, kfR), (cfL, cfR) = oracle_mates(kf), oracle_mates(cf)
    (_, kl, kr), (_, cl, cr) = triple(kf), triple(cf)
    keep = ref["keep"].astype(bool)
    rows, cols = oracle_chain.rows_of(ref["row_ptr"])[keep], ref["col_idx"][keep]
    rp = oracle_chain.filter_rows(ref["row_ptr"], keep)
    dL = orc.sift_min_distances(orc.sift_descriptors(kl, kfL), orc.sift_descriptors(cl, cfL)[cols], rp)
    dR = orc.sift_min_distances(orc.sift_descriptors(kr, kfR), orc.sift_descriptors(cr, cfR)[cols], rp)
    worst = np.maximum(dL, dR)
    levels = np.unique(worst)
    return levels, np.array([int((worst < v).sum()) for v in levels[:4]]), rows


# what tools/search_temporal_cases.py found, as tests/test_temporal_cases.py recomputes it (oracle only)
EXPECTED = {
    "kf80-cf209": dict(n_kf=80, n_cf=209, n_cells=112, max_cell=26, cells_64_65=0, n_candidates=1286),
    "kf209-cf95": dict(n_kf=209, n_cf=95, n_cells=112, max_cell=13, cells_64_65=0, n_candidates=1083),
    "kf239-cf80": dict(n_kf=239, n_cf=80, n_cells=112, max_cell=23, cells_64_65=0, n_candidates=898),
    "kf66": dict(n_kf=66, n_cf=1120, n_cells=112, max_cell=37, cells_64_65=0, n_candidates=810),
    "kf3": dict(n_kf=3, n_cf=1120, n_cells=112, max_cell=37, cells_64_65=0, n_candidates=111),
    "kf1": dict(n_kf=1, n_cf=1120, n_cells=112, max_cell=37, cells_64_65=0, n_candidates=15),
    "cf15": dict(n_kf=1175, n_cf=15, n_cells=112, max_cell=8, cells_64_65=0, n_candidates=202),
    "cf1": dict(n_kf=1175, n_cf=1, n_cells=112, max_cell=1, cells_64_65=0, n_candidates=11),
    "cells-104-crowded": dict(n_kf=4884, n_cf=4904, n_cells=104, max_cell=98, cells_64_65=4, n_candidates=136451),
    "cells-256": dict(n_kf=1241, n_cf=1179, n_cells=256, max_cell=29, cells_64_65=0, n_candidates=23696),
    "cells-375": dict(n_kf=1175, n_cf=1120, n_cells=375, max_cell=18, cells_64_65=0, n_candidates=23291),
}
