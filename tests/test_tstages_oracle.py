"""The stage trail without a device: the oracle's restated chain (tests/oracle_tstages.py) against oracle_chain's, the
library's new entry points, and the conditions the GPU tests (tests/test_gpu_tstages.py) rely on, from the oracle alone."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib
from tests import oracle_tgt as ot
from tests import oracle_tstages as ots
from tests import temporal_cases as tc
from tests import tgt_cases
from tests import tstages_cases as cases

NEW_SYMBOLS = ("ebvo_temporal_keep_stages", "ebvo_temporal_stage_size", "ebvo_temporal_fetch_stage", "ebvo_temporal_gt_stage_rows",
               "ebvo_tgt_grid_rows")
# the issue's table for `small` (defaults, no kf_gamma / kf_is_tp): stage -> (sum_n, sum_tp)
SMALL = {ot.GRID: (122399, 1728), ot.ORIENTATION: (12727, 1314), ot.NCC: (2051, 1276), ot.SIFT: (1122, 936),
         ot.BNB_NCC: (1122, 936), ot.BNB_SIFT: (586, 515), ot.CLUSTER: (509, 462)}


def test_library_exports_the_new_entry_points():
    root = Path(_lib.__file__).parent
    lib = ctypes.CDLL(str(root / "libebvo_hip.so"))
    header = (root.parent / "include" / "ebvo_hip.h").read_text()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.ABI_SYMBOLS and re.search(rf"\bint {name}\(", header), name
    assert re.search(r"#define EBVO_ABI_VERSION 6\b", header)       # additive: the version stays


@pytest.mark.parametrize("pset", list(cases.PARAMS))
def test_restated_chain_is_oracle_chains(pset):
    kf, cf, _ = tgt_cases.RESIDENT["small"]
    final, trail = cases.chain("small", pset)
    ref = tc.reference(kf, cf, None, True, **cases.PARAMS[pset])["final"]
    assert ots.same_final(final, ref)
    # the trail is consistent with the counts and with itself
    for k in cases.INTERIOR:
        t = trail[k]
        assert len(t["cf_index"]) == int(t["row_ptr"][-1]) == final["counts"][cases.TRAIL_COUNT[k]]
    assert (trail[ot.REFINE]["row_ptr"] == trail[ot.BNB_SIFT]["row_ptr"]).all()
    assert (trail[ot.REFINE]["cf_index"] == trail[ot.BNB_SIFT]["cf_index"]).all()
    moved = trail[ot.REFINE]["left"]["x"] != trail[ot.BNB_SIFT]["left"]["x"]
    assert moved.any()                                            # the refinement moves centres where it is valid


def test_small_has_every_stage_populated_and_every_filter_removes():
    r = {p: cases.resident_reference("small", p, 1, False) for p in cases.PARAMS}
    m = {k: v[2] for k, v in r["default"]["stages"].items()}
    assert sorted(m) == list(range(8))
    for k, (sum_n, sum_tp) in SMALL.items():
        assert (m[k]["sum_n"], m[k]["sum_tp"]) == (sum_n, sum_tp), k
    assert m[ot.REFINE]["sum_n"] == m[ot.BNB_SIFT]["sum_n"] and m[ot.REFINE]["sum_tp"] > 0
    assert all(v["sum_n"] > 0 and v["sum_tp"] > 0 for v in m.values())
    # every filter removes at least one quad from the evaluated rows under at least one parameter set (the refinement
    # removes none by construction); BNB-NCC only under the second one
    order = (ot.GRID, ot.ORIENTATION, ot.NCC, ot.SIFT, ot.BNB_NCC, ot.BNB_SIFT, ot.REFINE, ot.CLUSTER)
    for a, b in zip(order, order[1:]):
        if b == ot.REFINE:
            continue
        drops = [r[p]["stages"][a][2]["sum_n"] - r[p]["stages"][b][2]["sum_n"] for p in cases.PARAMS]
        assert max(drops) > 0 and min(drops) >= 0, (a, b, drops)
    d = r["default"]["stages"]
    assert d[ot.BNB_NCC][2]["sum_n"] == d[ot.SIFT][2]["sum_n"]
    t = r["tight-bnb-ncc"]["stages"]
    assert t[ot.BNB_NCC][2]["sum_n"] < t[ot.SIFT][2]["sum_n"]
    # each BNB test reorders rows
    for p in cases.PARAMS:
        assert r[p]["trail"][ot.BNB_NCC]["moved"] > 0 and r[p]["trail"][ot.BNB_SIFT]["moved"] > 0, p


def test_no_parameter_reaches_an_empty_list_after_a_populated_sift_stage():
    """Either best-nearly-best test keeps the best quad of every non-empty row (src/Temporal_Matches.cpp:517-570), so the
    chain's n3 == 0 exit follows only from an empty SIFT stage.  The harshest ratios leave one quad per non-empty row."""
    kf, cf, _ = tgt_cases.RESIDENT["small"]
    c = tc.reference(kf, cf, None, True, bnb_ncc=2.0, bnb_sift=2.0)["counts"]
    rows = int((np.diff(cases.chain("small", "default")[1][ot.SIFT]["row_ptr"]) > 0).sum())
    assert c["n_sift"] > rows and c["n_bnb_ncc"] == c["n_bnb_sift"] == rows > 0


def test_empty_exits_are_the_intended_ones():
    kf, cf, _ = tgt_cases.RESIDENT["small"]
    levels, _, _ = tc.sift_levels(kf, cf)
    c = tc.reference(kf, cf, None, True, sift_thr=float(levels[0]))["counts"]
    assert c["n_kept"] > 0 and c["n_sift"] == 0 and c["n_final"] == 0
    c = tc.reference(kf, cf, None, True, ncc_thr=2.0)["counts"]
    assert c["n_candidates"] > 0 and c["n_kept"] == 0 and c["n_final"] == 0


def test_grid_scenes_hold_their_conditions():
    s = cases.grid_scene("kf65")
    pop = cases.left_cell_populations(s["cfL"])
    assert {0, 1, 15, 16, 17, 33} <= set(pop.tolist())
    for name in cases.GRID_SCENES:
        if name.startswith("kf"):
            n_tp, m = cases.grid_reference(name)
            sc = cases.grid_scene(name)
            assert len(n_tp) == int(name[2:]) and m["sum_tp"] >= 1 and m["rows"] == int(sc["on"].sum())
            if len(n_tp) > 2:
                assert n_tp[2].tolist() == [0, 0] and not sc["on"][2]
    assert max(cases.grid_reference("kf65")[0][:, 0]) > 33        # a row walks the crowded cell and its neighbours
    n0, _ = cases.grid_reference("radius0")
    n17, _ = cases.grid_reference("kf17")
    nw, _ = cases.grid_reference("radius-wide")
    assert 0 < n0[:, 0].sum() < n17[:, 0].sum() < nw[:, 0].sum()
    on = cases.grid_scene("radius-wide")["on"]
    n_cf = len(cases.grid_scene("radius-wide")["cfL"])
    assert all(nw[i, 0] == n_cf for i in np.flatnonzero(on))       # wider than the grid: every mate of both grids
    e, me = cases.grid_reference("edges")
    sc = cases.grid_scene("edges")
    assert e[0, 0] > 0 and e[1, 0] > 0                            # the corner cells
    assert e[2].tolist() == [0, 0] and e[3].tolist() == [0, 0]     # query cells outside the grid, clipped to nothing
    assert e[4, 0] > 0                                            # outside, but within reach
    assert e[5].tolist() == [e[6, 0], 0] and e[6, 1] == 1          # exactly tp_dist is not a true positive
    dx = sc["cfL"]["x"] - sc["pl"][5, 0]
    dy = sc["cfL"]["y"] - sc["pl"][5, 1]
    assert (np.sqrt(dx * dx + dy * dy) == sc["tp_dist"]).any()
    assert e[7, 0] == e[6, 0] and e[7, 1] == 0                     # NaN projection
    assert e[8].tolist() == [0, 0] and not sc["on"][8]
    # the mate whose right (left) edge is outside its grid is in no row, although it lies at the projections of rows 9 (10)
    assert e[9, 1] == 0 and e[10, 1] == 0
    with_all = ots.grid_rows(sc["kfL"], sc["kfR"], sc["cfL"], sc["cfL"], cases.G_W, cases.G_H, cases.CELL, 5000.0, sc["on"], sc["pl"], sc["pl"])
    assert with_all[9, 0] == len(sc["cfL"]) - 1                   # (only the mate whose left edge is outside is missing)
    assert cases.grid_reference("no-cf")[1]["sum_n"] == 0 and cases.grid_reference("no-cf")[1]["rows"] == 4
    assert cases.grid_reference("no-kf")[1]["rows"] == 0
