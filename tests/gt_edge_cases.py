"""The edge cases of the stereo ground-truth tests (tests/test_gt_edge_cases.py, tests/test_gpu_gt_edges.py) and their oracle
side, computed once per process from tests/oracle.py and tests/oracle_gt.py (no device): slanted epipolar lines, long pool
rows, ground-truth and run parameters off their defaults, every stage mask, odd sizes, a zero-disparity patch.

Every image pair is synth.stereo_pair("s2", h, w) with the generator's 12-px disparity.  A case is
  dict(shape, geom, run, gt, zero_patch, finalize)
run: the run's epi_thr, max_disp, orient_thr_deg and stage_mask; gt: the five ebvo_gt_params; finalize: the GPU test also
runs the finalisation chain, armed and unarmed, and the oracle side holds all ten lists of a chain without SIFT."""
import functools
import math

import numpy as np

from edge_based_visual_odometry_amd import synth
from tests import gt_cases as gc
from tests import oracle as orc
from tests import oracle_chain as oc
from tests import oracle_gt as og

RUN_DEFAULT = dict(epi_thr=0.5, max_disp=25.0, orient_thr_deg=10.0, stage_mask=7)
GT_DEFAULT = dict(orient_gate_deg=4.0, pool_epi_thr=0.5, pool_dist=1.0, pool_orient_deg=5.0, tp_dist=1.0)
DISPARITY = 12
RUN_STAGES = (og.EPIPOLAR, og.DISPARITY, og.ORIENTATION, og.NCC)   # present after arming, before any finalisation

# the slanted geometry of tests/test_gpu_match.py (F_SLANT): a rotation about the optical axis, a baseline with all three
# components, two different cameras; its K, R21 and T21 are the GT calibration
_c, _s = math.cos(0.03), math.sin(0.03)
SLANT = dict(K=(450.0, 450.0, 100.0, 60.0), K_right=(460.0, 455.0, 98.0, 63.0),
             R21=((_c, -_s, 0.0), (_s, _c, 0.0), (0.0, 0.0, 1.0)), T21=(0.11, 0.02, 0.003))

# a rectified pair whose K inverts exactly in binary floating point (powers of two): the third component of K^-1 (x, y, 1) is
# exactly 1, so a zero disparity makes the back-projection's denominator exactly 0.  (Kitti's K gives 1 - 2^-53 there.)
POW2 = dict(K=(512.0, 512.0, 64.0, 32.0), K_right=(512.0, 512.0, 64.0, 32.0),
            R21=((1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)), T21=(0.5, 0.0, 0.0))

INF = float("inf")
PARAM_VALUES = dict(orient_gate_deg=(0.0, 45.0, INF), pool_epi_thr=(0.0, 3.0, INF), pool_dist=(0.0, 8.0, INF),
                    pool_orient_deg=(0.0, 30.0, 400.0), tp_dist=(0.0, 2.5, INF))
SIZES = ((33, 65), (37, 101))


def _case(shape=(120, 200), geom="kitti", run=None, gt=None, zero_patch=False, finalize=False):
    return dict(shape=shape, geom=geom, run=dict(RUN_DEFAULT, **(run or {})), gt=dict(GT_DEFAULT, **(gt or {})),
                zero_patch=zero_patch, finalize=finalize)


def _build_cases():
    c = {
        "default": _case(finalize=True),                         # the yardstick of the one-at-a-time parameters and of re-arming
        "wide_pool": _case(gt=dict(pool_epi_thr=8.0, pool_dist=12.0, pool_orient_deg=400.0), finalize=True),
        "mid_pool": _case(run=dict(epi_thr=2.0, max_disp=40.0, orient_thr_deg=30.0),
                          gt=dict(pool_epi_thr=3.0, pool_dist=8.0, pool_orient_deg=30.0, tp_dist=2.5), finalize=True),
        "short_reach": _case(run=dict(max_disp=11.5), finalize=True),
        "slant": _case(geom="slant", finalize=True),
        "slant_wide": _case(geom="slant", run=dict(epi_thr=2.0), gt=dict(pool_epi_thr=2.0, pool_dist=2.0, pool_orient_deg=5.0),
                            finalize=True),
        "zero_disp": _case(zero_patch=True),
        "zero_disp_exact": _case(geom="pow2", zero_patch=True),
    }
    for field, values in PARAM_VALUES.items():
        for v in values:
            c[f"{field}={v:g}"] = _case(gt={field: v})
    for mask in range(1, 8):
        c[f"mask{mask}"] = _case(shape=(37, 101), run=dict(stage_mask=mask), finalize=(mask == 7))
    for h, w in SIZES:
        c[f"size-{h}x{w}"] = _case(shape=(h, w), finalize=True)
    return c


CASES = _build_cases()
PARAM_CASES = tuple(f"{f}={v:g}" for f, vs in PARAM_VALUES.items() for v in vs)
MASK_CASES = tuple(f"mask{m}" for m in range(1, 8))
SIZE_CASES = tuple(f"size-{h}x{w}" for h, w in SIZES)
# the cases whose setting is meant to leave no focused row at all; every other case has focused rows
DELIBERATELY_UNFOCUSED = ("orient_gate_deg=inf", "pool_epi_thr=0", "pool_dist=0", "pool_orient_deg=0")


def geometry(geom):
    """(F21, (K_left, K_right, R21, T21))"""
    if geom == "kitti":
        return synth.fundamental_for("kitti"), gc.calib_of("kitti")
    g = dict(slant=SLANT, pow2=POW2)[geom]
    kl = [g["K"][0], 0, g["K"][2], 0, g["K"][1], g["K"][3], 0, 0, 1]
    kr = [g["K_right"][0], 0, g["K_right"][2], 0, g["K_right"][1], g["K_right"][3], 0, 0, 1]
    return synth.fundamental_21(g["K"], g["K_right"], g["R21"], g["T21"]), (kl, kr, g["R21"], g["T21"])


@functools.lru_cache(maxsize=None)
def pair(shape):
    """(left image, right image, oracle TOED edges of both)"""
    l, r = synth.stereo_pair("s2", *shape, disparity=DISPARITY)
    return l, r, orc.toed(l)["edges"], orc.toed(r)["edges"]


@functools.lru_cache(maxsize=None)
def _lines(shape, geom):
    return orc.epipolar_lines(geometry(geom)[0], pair(shape)[2])


@functools.lru_cache(maxsize=None)
def _stage1(shape, geom, epi_thr, max_disp, orient_thr_deg, stage_mask):
    """the run: candidate CSR and the first NCC pass"""
    l, r, L, R = pair(shape)
    rp, ci = orc.epi_candidates(L, R, _lines(shape, geom), epi_thr, max_disp, orient_thr_deg, stage_mask=stage_mask)
    sims, best, keep, _ = orc.ncc_pairs(l, r, L, R[ci], rp)
    return dict(row_ptr=rp, col_idx=ci, sims=sims, best=best, keep=keep)


@functools.lru_cache(maxsize=None)
def disparity(shape, zero_patch=False):
    return og.disparity_map(*shape, DISPARITY, zero_patch=zero_patch)


@functools.lru_cache(maxsize=None)
def _locations(shape, geom, zero_patch, gate):
    calib = geometry(geom)[1]
    return og.find_gt_locations(pair(shape)[2], disparity(shape, zero_patch), calib[0], calib[2], calib[3], gate)


@functools.lru_cache(maxsize=None)
def _pool(shape, geom, zero_patch, gate, epi_thr, dist, orient):
    _, _, L, R = pair(shape)
    loc = _locations(shape, geom, zero_patch, gate)
    return og.gt_pool(L, R, _lines(shape, geom), loc["valid"], loc["gt_xy"], epi_thr, dist, orient)


@functools.lru_cache(maxsize=None)
def _geometric(shape, geom, epi_thr, max_disp, orient_thr_deg, stage_mask):
    _, _, L, R = pair(shape)
    return og.geometric_lists(L, R, _lines(shape, geom), epi_thr, max_disp, orient_thr_deg, stage_mask)


@functools.lru_cache(maxsize=None)
def _chain_lists(shape, geom, epi_thr, max_disp, orient_thr_deg, stage_mask):
    """all ten lists of a chain without SIFT, and its final pairs"""
    l, r, L, R = pair(shape)
    s1 = dict(_stage1(shape, geom, epi_thr, max_disp, orient_thr_deg, stage_mask), left=L, right=R)
    return og.stage_lists(l, r, geometry(geom)[0], s1, epi_thr=epi_thr, max_disp=max_disp, orient_thr_deg=orient_thr_deg,
                          stage_mask=stage_mask)


@functools.lru_cache(maxsize=None)
def case(name):
    """The oracle side of one case, in the layout of gt_cases.base() (so test_gpu_gt.py's helpers take it) plus
    ev = {stage id: (n_tp [nL, 2], metrics dict)} and `final` (None unless the case finalises)."""
    c = CASES[name]
    shape, geom, run, gt = c["shape"], c["geom"], c["run"], c["gt"]
    l, r, L, R = pair(shape)
    F, calib = geometry(geom)
    rk = (run["epi_thr"], run["max_disp"], run["orient_thr_deg"], run["stage_mask"])
    s1 = _stage1(shape, geom, *rk)
    loc = _locations(shape, geom, c["zero_patch"], gt["orient_gate_deg"])
    pool = _pool(shape, geom, c["zero_patch"], gt["orient_gate_deg"], gt["pool_epi_thr"], gt["pool_dist"], gt["pool_orient_deg"])
    final = None
    if c["finalize"]:
        lists, final = _chain_lists(shape, geom, *rk)
    else:
        lists = dict(_geometric(shape, geom, *rk))
        k = s1["keep"].astype(bool)
        cand = R[s1["col_idx"][k]]
        lists[og.NCC] = (oc.filter_rows(s1["row_ptr"], k), cand["x"].copy(), cand["y"].copy())            # :1427
    ev = og.evaluate_stages(lists, pool["focused"], loc["gt_xy"], gt["tp_dist"])
    return dict(s1, l=l, r=r, F=F, calib=calib, disp=disparity(shape, c["zero_patch"]), left=L, right=R,
                lines=_lines(shape, geom), loc=loc, pool=pool, ev=ev, final=final, run=run, gt=gt, finalize=c["finalize"])


def conditions(name):
    """Counts of one case, from the oracle alone: what tests/test_gt_edge_cases.py asserts its conditions on."""
    b = case(name)
    pool, loc = b["pool"], b["loc"]
    foc = pool["focused"].astype(bool)
    rp, idx = pool["pool_row_ptr"], pool["pool_idx"]
    rows = [idx[rp[q]:rp[q + 1]] for q in range(len(rp) - 1)]
    out = dict(n_left=len(b["left"]), n_right=len(b["right"]), n_valid=int(loc["valid"].sum()), n_focused=int(foc.sum()),
               n_pool=len(idx), longest_pool_row=max((len(k) for k in rows), default=0),
               most_chunks=max((len(np.unique(k // 8)) for k in rows), default=0),
               most_groups=max((len(np.unique(k // 512)) for k in rows), default=0),
               empty_pool_on_focused_row=int((np.diff(rp) == 0).sum()))
    for sid, (n_tp, m) in b["ev"].items():
        n, tp = n_tp[foc, 0], n_tp[foc, 1]
        out[sid] = dict(empty=int((n == 0).sum()), without_tp=int(((n > 0) & (tp == 0)).sum()), with_tp=int((tp > 0).sum()),
                        longest=int(n.max()) if foc.any() else 0, sum_tp=m["sum_tp"], sum_n=m["sum_n"], recall=m["recall"])
    return out


def gt_to_line_distance(name):
    """distance of every valid edge's GT location from its epipolar line (px)"""
    b = case(name)
    v = b["loc"]["valid"].astype(bool)
    a, bb, c = b["lines"][v].T
    x, y = b["loc"]["gt_xy"][v].T
    return np.abs(a * x + bb * y + c) / np.sqrt(a * a + bb * bb)
