"""The stage trail of the temporal chain and the ground-truth evaluation of all eight stages on the device
(ebvo_temporal_keep_stages, ebvo_temporal_stage_size / _fetch_stage, ebvo_temporal_gt_stage_rows, ebvo_tgt_grid_rows, and
ebvo_temporal_set_gt / _gt_metrics / _gt_flags on a slot that kept its trail) against tests/oracle_tstages.py and
tests/oracle_tgt.py, bit for bit: integers with ==, doubles by their bit patterns.

Inputs (tests/tstages_cases.py; tests/test_tstages_oracle.py checks their conditions without a device):
  resident      small0 / small2 under the default parameters and under a bnb_ncc at which BNB-NCC removes quads, stages 0
                and 1, with and without kf_gamma / kf_is_tp; kf / cf2 (240 x 376) once at the defaults
  empty exits   an NCC threshold above every score, the lowest SIFT level, and the harshest best-nearly-best ratios.  No
                parameter reaches the chain's n3 == 0 exit with a populated SIFT stage: each best-nearly-best test keeps the
                best quad of every non-empty row (test_tstages_oracle asserts it), so that exit is reached through an empty
                SIFT stage only, and the harshest ratios are checked for the one quad per row they leave
  host arrays   hand-made mates: 1 ... 65 keyframe mates, cells of 0, 1, 15, 16, 17 and 33 mates, radius 0 and wider than
                the grid, corner cells, query cells outside the grid, mates outside either grid, an off row, a NaN
                projection, a distance of exactly tp_dist, no mates on either side
"""
import numpy as np
import pytest

from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EBVO_ERR_CAPACITY, EBVO_ERR_STATE, EbvoError, ptr
from tests import oracle_chain
from tests import oracle_tgt as ot
from tests import temporal_cases as tc
from tests import tgt_cases
from tests import tstages_cases as cases
from tests.test_gpu_pose import assert_same
from tests.test_gpu_temporal_edges import CALIB, keys, load, match, new_context, same_results
from tests.test_gpu_tgt import DBL_KEYS, INT_KEYS, check_stage, device_keyframe_gt
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu

LEGACY = {ot.ORIENTATION, ot.NCC, ot.CLUSTER}


@pytest.fixture(scope="module")
def gctx():
    """a context of these tests' own (the switch and the developer keys never reach the session context)"""
    c = new_context("hybrid")
    yield c
    c.close()


@pytest.fixture()
def kept(gctx):
    """slot 0 with the switch on for the test, off afterwards"""
    gctx.temporal_keep_stages(True)
    yield gctx
    gctx.temporal_keep_stages(False)


def raises(status, call):
    with pytest.raises(EbvoError) as ei:
        call()
    assert ei.value.status == status, ei.value
    return str(ei.value)


def frames(c, name):
    """keyframe and current frame of a resident case in slot 0; (kf, cf, gamma, is_tp)"""
    kf, cf, _ = tgt_cases.RESIDENT[name]
    load(c, kf)
    gamma, is_tp = device_keyframe_gt(c, kf, 0)
    c.temporal_set_keyframe()
    load(c, cf)
    return kf, cf, gamma, is_tp


def expected_present(stages):
    return {ot.GRID, ot.ORIENTATION, ot.NCC} | (set(cases.INTERIOR) | {ot.CLUSTER} if stages else set())


def check_trail(c, trail, what):
    for k in cases.INTERIOR:
        got, ref = c.temporal_fetch_stage(k), trail[k]
        for f in ("row_ptr", "cf_index"):
            assert_bit_equal(got[f], ref[f], f"{what}: stage {k} {f}")
        for f in ("left", "right"):
            assert oracle_chain._same_edges(got[f], ref[f]), f"{what}: stage {k} {f} centres"


def check_all(c, r, counts, stages, what):
    """every stage record, its per-row counts and its flags against the oracle's"""
    m = c.temporal_gt_metrics()
    present = expected_present(stages)
    assert [s["present"] for s in m] == [k in present for k in range(8)], what
    sizes = {ot.ORIENTATION: counts["n_candidates"], ot.NCC: counts["n_kept"], ot.CLUSTER: counts.get("n_final", 0)}
    sizes.update({k: counts.get(cases.TRAIL_COUNT[k], 0) for k in cases.INTERIOR})
    for k in range(8):
        if k not in present:
            assert all(m[k][key] == 0 for key in INT_KEYS + DBL_KEYS)
            raises(EBVO_ERR_STATE, lambda: c.temporal_gt_stage_rows(k))
            continue
        n_tp, flags, ref = r["stages"][k]
        check_stage(m[k], ref, f"{what} stage {k}")
        assert_bit_equal(c.temporal_gt_stage_rows(k), n_tp, f"{what}: rows of stage {k}")
        if k == ot.GRID:
            assert "no list" in raises(EBVO_ERR_STATE, lambda: c.temporal_gt_flags(k, 1))
        else:
            assert_bit_equal(c.temporal_gt_flags(k, sizes[k]), flags, f"{what}: flags of stage {k}")
    if stages:
        check_trail(c, r["trail"], what)


def arm(c, r, gamma, is_tp, with_gt):
    return c.temporal_set_gt(r["R"], r["t"], r["calib"], kf_gamma=gamma if with_gt else None, kf_is_tp=is_tp if with_gt else None)


# --- resident slot -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages", [0, 1])
@pytest.mark.parametrize("pset", list(cases.PARAMS))
def test_resident_small_equals_oracle(kept, pset, stages):
    c = kept
    kf, cf, gamma, is_tp = frames(c, "small")
    counts, q, _ = match(c, kf, cf, stages=stages, **cases.PARAMS[pset])
    for with_gt in (False, True):
        r = cases.resident_reference("small", pset, stages, with_gt)
        arm(c, r, gamma, is_tp, with_gt)
        check_all(c, r, counts, stages, f"small {pset} stages {stages} gt {with_gt}")
    if not stages:
        raises(EBVO_ERR_STATE, lambda: c.temporal_fetch_stage(ot.SIFT))   # stages = 0 holds no interior stage


def test_resident_euroc_half_equals_oracle(kept):
    c = kept
    kf, cf, gamma, is_tp = frames(c, "euroc-half")
    counts, q, _ = match(c, kf, cf, stages=1)
    r = cases.resident_reference("euroc-half", "default", 1, False)
    arm(c, r, gamma, is_tp, False)
    check_all(c, r, counts, 1, "euroc-half")


def test_launch_grids_change_no_bit(kept):
    c = kept
    kf, cf, gamma, is_tp = frames(c, "small")
    r = cases.resident_reference("small", "default", 1, False)
    for grid in (1, 3, 0):                                        # developer key 22: the chain's launches
        with keys(c, {22: grid}):
            counts, q, _ = match(c, kf, cf, stages=1)
        for gt_grid in (1, 3, 0):                                 # developer key 21: the evaluation's launches
            with keys(c, {21: gt_grid}):
                arm(c, r, gamma, is_tp, False)
                check_all(c, r, counts, 1, f"key 22 = {grid}, key 21 = {gt_grid}")


# --- no change when off, and when on ------------------------------------------------------------------------------------
def run_profiled(c, kf, cf, r):
    c.profile_enable(True)
    c.profile_reset()
    counts, q, _ = match(c, kf, cf, stages=1)
    launches = {k: v[1] for k, v in c.profile_get().items()}
    c.profile_enable(False)
    c.temporal_set_gt(r["R"], r["t"], r["calib"])
    return counts, q, launches, c.temporal_estimate_pose_gt(CALIB), c.temporal_gt_metrics()


def test_switch_off_is_the_legacy_slot_and_on_changes_no_result(gctx):
    c = gctx
    kf, cf, gamma, is_tp = frames(c, "small")
    r = cases.resident_reference("small", "default", 1, False)
    c.temporal_keep_stages(False)
    counts0, q0, launches0, pose0, m0 = run_profiled(c, kf, cf, r)
    assert {k for k in range(8) if m0[k]["present"]} == LEGACY
    for k in cases.INTERIOR:
        raises(EBVO_ERR_STATE, lambda: c.temporal_fetch_stage(k))
        raises(EBVO_ERR_STATE, lambda: c.temporal_gt_flags(k, 1))
    raises(EBVO_ERR_STATE, lambda: c.temporal_gt_stage_rows(ot.GRID))
    assert "ebvo_temporal_fetch returns" in raises(EBVO_ERR_ARG, lambda: c.temporal_fetch_stage(ot.NCC))
    assert "ebvo_temporal_fetch_final" in raises(EBVO_ERR_ARG, lambda: c.temporal_fetch_stage(ot.CLUSTER))
    assert "no list" in raises(EBVO_ERR_ARG, lambda: c.temporal_fetch_stage(ot.GRID))
    c.temporal_keep_stages(True)
    try:
        # the switch alone touches neither the match nor the armed state
        assert c.temporal_gt_metrics() == m0
        counts1, q1, launches1, pose1, m1 = run_profiled(c, kf, cf, r)
    finally:
        c.temporal_keep_stages(False)
    assert counts1 == counts0
    same_results(q1, q0, "switch on")
    assert_same(pose1, dict(pose0, quad_geom=None), geom=False)
    assert launches1 == launches0                                  # the trail adds copies, no launch
    assert {k for k in range(8) if m1[k]["present"]} == set(range(8))
    for k in LEGACY:
        assert m1[k] == m0[k]


# --- empty exits ---------------------------------------------------------------------------------------------------------
def _exit_cases():
    kf, cf, _ = tgt_cases.RESIDENT["small"]
    levels, _, _ = tc.sift_levels(kf, cf)
    return {"nothing-kept": (dict(ncc_thr=2.0), ot.NCC), "nothing-passes-sift": (dict(sift_thr=float(levels[0])), ot.SIFT),
            "no-candidates": (dict(orient_thr_deg=0.0), ot.ORIENTATION)}


@pytest.mark.parametrize("case", ["nothing-kept", "nothing-passes-sift", "no-candidates"])
def test_empty_exits_report_empty_stages(kept, case):
    c = kept
    kw, first_empty = _exit_cases()[case]
    kf, cf, gamma, is_tp = frames(c, "small")
    match(c, kf, cf, stages=1)                                    # full lists sit in the slot's buffers
    counts, q, ref = match(c, kf, cf, stages=1, **kw)
    assert ref["counts"]["n_final"] == 0
    r = cases.resident_reference("small", "default", 0, False)
    arm(c, r, gamma, is_tp, False)
    on, zero = cases.empty_reference("small", counts["n_kf"])
    assert zero["rows"] == int(on.sum()) > 0 and zero["sum_n"] == 0
    m = c.temporal_gt_metrics()
    assert all(s["present"] for s in m)
    for k in (ot.GRID, ot.ORIENTATION, ot.NCC):
        if k < first_empty:
            check_stage(m[k], r["stages"][k][2], f"{case} stage {k}")
            assert m[k]["sum_n"] > 0
    for k in range(first_empty, 8):
        check_stage(m[k], zero, f"{case} stage {k}")
        assert [m[k][key] for key in DBL_KEYS] == [0.0] * 4
        assert not c.temporal_gt_stage_rows(k).any()
    for k in cases.INTERIOR:
        got = c.temporal_fetch_stage(k)
        assert not got["row_ptr"].any() and len(got["row_ptr"]) == counts["n_kf"] + 1 and len(got["cf_index"]) == 0
        assert len(c.temporal_gt_flags(k, 0)) == 0


def test_harshest_ratios_leave_one_quad_per_row(kept):
    c = kept
    kf, cf, gamma, is_tp = frames(c, "small")
    counts, q, ref = match(c, kf, cf, stages=1, bnb_ncc=2.0, bnb_sift=2.0)
    sift, bnb = c.temporal_fetch_stage(ot.SIFT), c.temporal_fetch_stage(ot.BNB_SIFT)
    assert_bit_equal(np.diff(bnb["row_ptr"]), (np.diff(sift["row_ptr"]) > 0).astype(np.int32), "one quad per non-empty row")
    assert counts["n_bnb_sift"] == len(bnb["cf_index"]) > 0


# --- state ---------------------------------------------------------------------------------------------------------------
def test_state(gctx):
    c = gctx
    kf, cf, gamma, is_tp = frames(c, "small")
    r = cases.resident_reference("small", "default", 1, False)
    c.temporal_keep_stages(True)
    try:
        c.temporal_match_submit(stages=1)
        raises(EBVO_ERR_STATE, lambda: c.temporal_keep_stages(False))   # a match is in flight
        counts, q = c.temporal_match_wait()
        raises(EBVO_ERR_ARG, lambda: c.temporal_keep_stages(True, slot=9))
        check_trail(c, r["trail"], "before arming")                 # the trail needs no ground truth
        arm(c, r, gamma, is_tp, False)
        check_all(c, r, counts, 1, "first pose")
        # a second pose: the same trail, evaluated again
        R2, t2 = tgt_cases.resident_pose(2.0)
        c.temporal_set_gt(R2, t2, r["calib"])
        m2 = c.temporal_gt_metrics()
        assert all(s["present"] for s in m2) and m2[ot.GRID]["sum_tp"] != r["stages"][ot.GRID][2]["sum_tp"]
        check_trail(c, r["trail"], "after a second pose")
        arm(c, r, gamma, is_tp, False)
        check_all(c, r, counts, 1, "first pose again")
        # a refused call leaves the stages as they were
        before = (c.temporal_gt_metrics(), [c.temporal_gt_stage_rows(k) for k in range(8)])
        raises(EBVO_ERR_ARG, lambda: c.temporal_set_gt(np.full((3, 3), np.nan), r["t"], r["calib"]))
        raises(EBVO_ERR_ARG, lambda: c.temporal_set_gt(r["R"], r["t"], r["calib"], tp_dist=-1.0))
        assert c.temporal_gt_metrics() == before[0]
        for k in range(8):
            assert_bit_equal(c.temporal_gt_stage_rows(k), before[1][k], f"after refusals: stage {k}")
        raises(EBVO_ERR_ARG, lambda: c.temporal_gt_stage_rows(8))
        out = np.zeros((counts["n_kf"] - 1, 2), dtype=np.int32)
        assert c.lib.ebvo_temporal_gt_stage_rows(c._ctx, 0, ot.SIFT, ptr(out), counts["n_kf"] - 1) == EBVO_ERR_CAPACITY
        assert not out.any()
        # the host-array twin on slot 0 leaves the armed slot and its trail alone
        s = cases.grid_scene("kf5")
        c.tgt_grid_rows(s["kfL"], s["kfR"], s["cfL"], s["cfR"], cases.G_W, cases.G_H, s["on"], s["pl"], s["pr"])
        check_all(c, r, counts, 1, "after the host twin")
        # a new match without the switch drops the trail ...
        c.temporal_keep_stages(False)
        match(c, kf, cf, stages=1)
        raises(EBVO_ERR_STATE, lambda: c.temporal_fetch_stage(ot.SIFT))
        c.temporal_keep_stages(True)
        match(c, kf, cf, stages=1)
        check_trail(c, r["trail"], "matched again")
        # ... and so do an upload and a run of the slot
        l, rr = tc.images(cf)
        c.stereo_upload(l, rr)
        raises(EBVO_ERR_STATE, lambda: c.temporal_fetch_stage(ot.SIFT))
        load(c, cf)
        raises(EBVO_ERR_STATE, lambda: c.temporal_fetch_stage(ot.SIFT))
        match(c, kf, cf, stages=1)
        check_trail(c, r["trail"], "after a new run")
    finally:
        c.temporal_keep_stages(False)


# --- host arrays ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.GRID_SCENES)
def test_grid_rows_on_host_arrays(gctx, name):
    s = cases.grid_scene(name)
    n_tp, ref = cases.grid_reference(name)
    for grid in (0, 1, 3):                                        # developer key 21: same bits for any grid
        with keys(gctx, {21: grid}):
            got, g = gctx.tgt_grid_rows(s["kfL"], s["kfR"], s["cfL"], s["cfR"], cases.G_W, cases.G_H, s["on"], s["pl"], s["pr"],
                                        grid_radius=s["radius"], tp_dist=s["tp_dist"])
        assert_bit_equal(got, n_tp, f"{name} grid {grid}: n_tp")
        check_stage(g, ref, f"{name} grid {grid}")
        assert g["present"]
    if len(s["on"]):
        got, g = gctx.tgt_grid_rows(s["kfL"], s["kfR"], s["cfL"], s["cfR"], cases.G_W, cases.G_H, None, s["pl"], s["pr"],
                                    grid_radius=s["radius"], tp_dist=s["tp_dist"])
        assert g["rows"] == len(s["on"]) and (got[s["on"] != 0] == n_tp[s["on"] != 0]).all()   # row_on = NULL: every row


def test_grid_rows_refusals_and_profiler(gctx):
    s = cases.grid_scene("kf17")
    args = (s["kfL"], s["kfR"], s["cfL"], s["cfR"], cases.G_W, cases.G_H, s["on"], s["pl"], s["pr"])
    for kw in (dict(cell_size=0), dict(grid_radius=-1.0), dict(grid_radius=float("inf")), dict(grid_radius=float("nan")),
               dict(tp_dist=-0.5), dict(tp_dist=float("nan"))):
        raises(EBVO_ERR_ARG, lambda: gctx.tgt_grid_rows(*args, **kw))
    gctx.profile_enable(True)
    gctx.profile_reset()
    gctx.tgt_grid_rows(*args)
    prof = gctx.profile_get()
    gctx.profile_enable(False)
    assert prof["tgt_grid_rows"][1] == 1 and prof["tgt_rows"][1] == 0
