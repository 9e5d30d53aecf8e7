"""The conditions tests/test_gpu_gt_edges.py puts on its inputs (tests/gt_edge_cases.py), re-derived from the oracle alone, and
the rules tests/oracle_gt.py gained for them.  No device.  A case that stops meeting its condition fails here, whatever the
device would have made of it.  The counts found are recorded in tests/test_gpu_gt_edges.py's docstring."""
import math

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib
from tests import gt_edge_cases as ge
from tests import oracle_gt as og

GEOMETRIC = (og.EPIPOLAR, og.DISPARITY, og.ORIENTATION)


def _rows(name, sid):
    """(n, tp) of the focused rows of one stage"""
    b = ge.case(name)
    return b["ev"][sid][0][b["pool"]["focused"].astype(bool)]


@pytest.mark.parametrize("name", list(ge.CASES))
def test_general_health(name):
    """Every case but the deliberate ones focuses rows, and every focused row has a non-empty pool; a finalising case
    carries all ten lists of a chain without SIFT, the others the four lists of the run."""
    c, b = ge.conditions(name), ge.case(name)
    if name in ge.DELIBERATELY_UNFOCUSED:
        assert c["n_focused"] == 0 and c["n_pool"] == 0
    else:
        assert c["n_focused"] > 0 and c["empty_pool_on_focused_row"] == 0
        assert (np.diff(b["pool"]["pool_row_ptr"]) > 0).all()
    assert c["n_left"] > 100 and c["n_right"] > 100
    want = set(range(12)) - {og.SIFT, og.BNB_SIFT} if b["finalize"] else set(ge.RUN_STAGES)
    assert set(b["ev"]) == want
    assert (b["final"] is not None) == b["finalize"]


def test_wide_pool_has_long_rows_over_many_chunks_and_two_groups():
    c = ge.conditions("wide_pool")
    assert c["longest_pool_row"] > 64          # more than one round of the wave in gt_pool_kernel<true>
    assert c["most_chunks"] > 8                # more than one batch of eight marked chunks in walk_right_edges
    assert c["most_groups"] >= 2               # a row whose pool crosses a boundary between groups of 512 right edges
    assert c["n_focused"] > ge.conditions("default")["n_focused"]


def test_mid_pool_has_rows_with_and_without_a_tp_and_long_epipolar_rows():
    c = ge.conditions("mid_pool")
    assert c[og.BEST]["with_tp"] > 0 and c[og.BEST]["without_tp"] > 0 and c[og.BEST]["empty"] > 0
    assert c[og.EPIPOLAR]["longest"] > 64


def test_short_reach_has_all_three_kinds_of_row_from_the_disparity_stage_on():
    c = ge.conditions("short_reach")
    assert ge.CASES["short_reach"]["run"]["max_disp"] < ge.DISPARITY
    for sid in sorted(k for k in c if isinstance(k, int) and k >= og.DISPARITY):
        for kind in ("empty", "without_tp", "with_tp"):
            assert c[sid][kind] >= 100, (sid, kind, c[sid])
    assert c[og.EPIPOLAR]["empty"] == 0        # the epipolar stage does not know max_disp


def test_slant_focuses_part_of_the_valid_edges():
    c, w = ge.conditions("slant"), ge.conditions("slant_wide")
    assert 0 < 2 * c["n_focused"] < c["n_valid"]
    assert 2 * w["n_focused"] > w["n_valid"]
    assert 0.3 < w[og.BEST]["recall"] < 0.95
    assert ge.gt_to_line_distance("slant").max() > 3.0          # the GT location (x - d, y) leaves the epipolar line
    lines = ge.case("slant")["lines"]
    assert (np.abs(lines[:, 0] / lines[:, 1]) > 1e-2).all()     # no line with a = 0: the band test sees a slope


def test_one_parameter_at_a_time():
    d = ge.conditions("default")
    dflt = ge.case("default")
    # gate 0 leaves no edge gated: the valid edges are exactly those with a valid disparity, near-horizontal ones included
    g0 = ge.case("orient_gate_deg=0")["loc"]["valid"].astype(bool)
    deg = dflt["left"]["theta"] * og.RAD_TO_DEG
    gated = (np.abs(deg) < 4.0) | (np.abs(deg - 180.0) < 4.0) | (np.abs(deg + 180.0) < 4.0)
    assert (g0[~gated] == dflt["loc"]["valid"][~gated].astype(bool)).all() and (g0 & gated).sum() > 0
    assert ge.conditions("orient_gate_deg=45")["n_valid"] < d["n_valid"]
    assert ge.conditions("orient_gate_deg=inf")["n_valid"] == 0
    for name in ("pool_epi_thr=0", "pool_dist=0", "pool_orient_deg=0"):
        c = ge.conditions(name)
        assert c["n_valid"] == d["n_valid"] > 0 and c["n_focused"] == 0, name
    for name in ("pool_epi_thr=3", "pool_epi_thr=inf", "pool_dist=8", "pool_dist=inf", "pool_orient_deg=30", "pool_orient_deg=400"):
        assert ge.conditions(name)["n_pool"] > d["n_pool"], name
    for sid in ge.RUN_STAGES:
        n_tp = _rows("tp_dist=inf", sid)
        assert (n_tp[:, 1] == n_tp[:, 0]).all() and n_tp[:, 0].sum() > 0
        assert ge.conditions("tp_dist=0")[sid]["sum_tp"] < d[sid]["sum_tp"] < ge.conditions("tp_dist=2.5")[sid]["sum_tp"]


@pytest.mark.parametrize("mask", range(1, 8))
def test_masks(mask):
    name = f"mask{mask}"
    b, c = ge.case(name), ge.conditions(name)
    if not mask & 1:
        assert (_rows(name, og.EPIPOLAR)[:, 0] == c["n_right"]).all()      # no predicate yet: every right edge
        assert c["n_right"] > 64
    foc = b["pool"]["focused"].astype(bool)
    assert (_rows(name, og.ORIENTATION)[:, 0] == np.diff(b["row_ptr"])[foc]).all()
    # a stage that is switched off passes its list on unchanged
    for sid, bit in ((og.DISPARITY, 2), (og.ORIENTATION, 4)):
        if not mask & bit:
            assert (b["ev"][sid][0] == b["ev"][sid - 1][0]).all()
    assert c["n_focused"] >= 30


@pytest.mark.parametrize("name", ge.SIZE_CASES)
def test_sizes(name):
    assert ge.conditions(name)["n_focused"] >= 30


def test_zero_disparity():
    """d = 0 is valid and puts the GT location on the edge.  With Kitti's K the third component of K^-1 (x, y, 1) is
    1 - 2^-53, not 1: the back-projection's denominator is an ulp of the ray's x, not 0, and the 3-D points are finite
    and enormous.  The exactly invertible K of zero_disp_exact makes the denominator 0 and the points infinite."""
    for name in ("zero_disp", "zero_disp_exact"):
        b = ge.case(name)
        v = b["loc"]["valid"].astype(bool)
        on_edge = v & (b["loc"]["gt_xy"][:, 0] == b["left"]["x"])
        assert on_edge.sum() >= 1 and (b["disp"] == 0.0).any()
        gl, gr = b["loc"]["gamma_left"][on_edge], b["loc"]["gamma_right"][on_edge]
        if name == "zero_disp":
            assert np.isfinite(gl).all() and (np.abs(gl[:, 2]) > 1e12).all()
        else:
            assert np.isinf(gl).any() and not np.isfinite(gr).all()
        assert np.isfinite(b["loc"]["gamma_left"][v & ~on_edge]).all()
    assert og.inverse3(np.reshape(ge.case("zero_disp")["calib"][0], (3, 3)))[2][2] == 1.0 - 2.0 ** -53
    assert og.inverse3(np.reshape(ge.case("zero_disp_exact")["calib"][0], (3, 3)))[2][2] == 1.0


def test_zero_patch_leaves_the_rest_of_the_map_alone():
    for h, w in ((120, 200), (37, 101), (200, 320)):
        a, z = og.disparity_map(h, w, 12), og.disparity_map(h, w, 12, zero_patch=True)
        differ = a.view(np.uint32) != z.view(np.uint32)
        assert differ.any() and (z[differ] == 0.0).all() and not (a == 0.0).any()


def test_non_finite_coordinates_are_skipped():
    """The stated rule of find_gt_locations: valid 0 and the fill values, whatever the orientation gate."""
    e = np.zeros(6, dtype=_lib.EDGE_DTYPE)
    e["x"] = [math.nan, 20.5, math.inf, -math.inf, 20.5, 20.5]
    e["y"] = [10.5, math.nan, 10.5, 10.5, math.inf, 10.5]
    e["theta"] = 1.0
    d = np.full((48, 64), 4.0, dtype=np.float32)
    K = [100.0, 0, 32.0, 0, 100.0, 24.0, 0, 0, 1]
    for gate in (0.0, 4.0):
        r = og.find_gt_locations(e, d, K, np.eye(3), [-0.5, 0.0, 0.0], gate)
        assert r["valid"].tolist() == [0, 0, 0, 0, 0, 1]
        assert (r["gt_xy"][:5] == -1.0).all() and (r["gamma_left"][:5] == -1.0).all() and (r["gamma_right"][:5] == -1.0).all()


def test_geometric_lists_follow_the_mask():
    """stage_mask & 1, & 3, & 7: with every stage on, the lists of tests/oracle.py at masks 1, 3 and 7 (what stage_lists
    formed before it took a mask); with none on yet, every right edge."""
    from tests import oracle as orc
    b = ge.case("mask7")
    L, R, lines = b["left"], b["right"], b["lines"]
    full = og.geometric_lists(L, R, lines)
    for sid, mask in ((og.EPIPOLAR, 1), (og.DISPARITY, 3), (og.ORIENTATION, 7)):
        rp, ci = orc.epi_candidates(L, R, lines, stage_mask=mask)
        assert (full[sid][0] == rp).all() and full[sid][1].tobytes() == R["x"][ci].tobytes()
    dense = og.geometric_lists(L, R, lines, stage_mask=4)[og.EPIPOLAR]
    assert (np.diff(dense[0]) == len(R)).all() and dense[1].tobytes() == np.tile(R["x"], len(L)).tobytes()
