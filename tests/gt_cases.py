"""The stereo pairs of the ground-truth tests (tests/test_gt_oracle.py, tests/test_gpu_gt.py) and their oracle side, computed
once per process: images, calibration, disparity map, TOED + candidates + first NCC pass, GT locations, veridical pool and
the evaluated stage lists -- all from tests/oracle.py and tests/oracle_gt.py (no device)."""
import functools

import numpy as np

from edge_based_visual_odometry_amd import synth
from tests import oracle as orc
from tests import oracle_gt as og

# name: (config, generator kind, (h, w), arguments of synth.stereo_pair)
PAIRS = {
    "s1-200x320": ("kitti", "s1", (200, 320), dict(disparity=12)),
    "s2-200x320": ("kitti", "s2", (200, 320), dict(disparity=12)),
    "eth3d-942x489": ("eth3d", "s2", synth.SHAPES["eth3d"], dict(scene=11, noise_base=4, disparity=9)),
    "kitti": ("kitti", "s2", synth.SHAPES["kitti"], dict(scene=7, noise_base=0, disparity=12)),   # bench.py's pair
}
SIFT_PAIRS = tuple(PAIRS)   # every pair's chain is also run with use_sift = 1


def calib_of(cfg):
    c = synth.CALIB[cfg]
    kl = [c["K"][0], 0, c["K"][2], 0, c["K"][1], c["K"][3], 0, 0, 1]
    kr = [c["K_right"][0], 0, c["K_right"][2], 0, c["K_right"][1], c["K_right"][3], 0, 0, 1]
    return kl, kr, c["R21"], c["T21"]


@functools.lru_cache(maxsize=None)
def base(name):
    cfg, kind, (h, w), args = PAIRS[name]
    F = synth.fundamental_for(cfg)
    l, r = synth.stereo_pair(kind, h, w, **args)
    L, R = orc.toed(l)["edges"], orc.toed(r)["edges"]
    lines = orc.epipolar_lines(F, L)
    rp, ci = orc.epi_candidates(L, R, lines)
    sims, best, keep, _ = orc.ncc_pairs(l, r, L, R[ci], rp)
    calib = calib_of(cfg)
    disp = og.disparity_map(h, w, args["disparity"])
    loc = og.find_gt_locations(L, disp, calib[0], calib[2], calib[3])
    pool = og.gt_pool(L, R, lines, loc["valid"], loc["gt_xy"])
    return dict(l=l, r=r, F=F, calib=calib, disp=disp, left=L, right=R, lines=lines, row_ptr=rp, col_idx=ci, sims=sims,
                best=best, keep=keep, loc=loc, pool=pool)


@functools.lru_cache(maxsize=None)
def stages(name, sift=False):
    """{stage id: (n_tp [nL, 2], metrics dict)} and the chain's final pairs"""
    b = base(name)
    lists, final = og.stage_lists(b["l"], b["r"], b["F"], b, sift=sift)
    return og.evaluate_stages(lists, b["pool"]["focused"], b["loc"]["gt_xy"]), final


def input_conditions(name):
    """The conditions the tests put on their inputs (counts from the oracle alone)."""
    b = base(name)
    ev, _ = stages(name, False)
    best = ev[og.BEST][0]
    foc = b["pool"]["focused"].astype(bool)
    return dict(n_left=len(b["left"]), n_valid=int(b["loc"]["valid"].sum()), n_focused=int(foc.sum()),
                n_pool=len(b["pool"]["pool_idx"]),
                valid_with_empty_pool=int(((b["loc"]["valid"] != 0) & (b["pool"]["pool_count"] == 0)).sum()),
                best_rows_with_tp=int((best[foc, 1] > 0).sum()), best_rows_without_tp=int((best[foc, 1] == 0).sum()))
