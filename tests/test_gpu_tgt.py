"""Temporal ground truth on the device (ebvo_temporal_set_gt, ebvo_temporal_gt_size / _fetch / _metrics / _flags,
ebvo_tgt_veridical, ebvo_tgt_evaluate_rows) against tests/oracle_tgt.py, bit for bit: in-image flags, both projections, both
projected orientations, the veridical CSR, the per-row (n, tp), the per-quad flags, the integer totals and the four doubles.

Inputs (tests/tgt_cases.py; tests/test_tgt_oracle.py checks their conditions without a device):
  host arrays   synthetic quads of a known motion, n_kf = 1, 3, 63, 64, 65, 257; grids of 40 / 52 cells (fewer than a
                block's 256 threads) and 1650 / 2025 cells (more)
  borders       projections on both sides of the margin and of a cell border, a mate in the left cell set only,
                orientation offsets around 0, 180 and 360 degrees
  resident      small0 / small2 (120 x 200) and kf / cf2 (240 x 376) of tests/temporal_cases.py, the pose of
                tgt_cases.RESIDENT; counts in tgt_cases.EXPECTED
The kf_gamma / kf_is_tp variant takes both from the stereo ground truth of the keyframe on the device: the keyframe slot is
armed with the disparity map, and since this rig leaves no focused row in these frames (tgt_cases.keyframe_gt) the per-mate
values come from ebvo_gt_locate, the kernel arming runs, and are asserted equal to the oracle's before they are used.
The oracle side is computed from the ORACLE's mates and lists; the device's are asserted equal to those first
(tests/test_gpu_temporal_edges.py: load, match).  The temporal stages do not depend on the detector mode."""
import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib
from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EBVO_ERR_STATE, EbvoError
from tests import oracle_tgt as ot
from tests import temporal_cases as tc
from tests import tgt_cases as cases
from tests.test_gpu_temporal_edges import CALIB, keys, load, match, new_context, same_results
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu

INT_KEYS = ("rows", "nonempty", "rows_with_tp", "sum_tp", "sum_n")
DBL_KEYS = ("recall", "precision", "precision_pair", "ambiguity")
VER_KEYS = ("in_image", "proj_left", "proj_right", "orient_left", "orient_right", "ver_row_ptr", "ver_idx")


@pytest.fixture(scope="module")
def gctx():
    """a context of these tests' own (developer key 21 never reaches the session context)"""
    c = new_context("hybrid")
    yield c
    c.close()


def check_veridical(got, ref, what):
    for k in VER_KEYS:
        assert_bit_equal(got[k], ref[k], f"{what}: {k}")


def check_stage(got, ref, what):
    for k in INT_KEYS:
        assert got[k] == ref[k], f"{what}: {k} {got[k]} != oracle {ref[k]}"
    for k in DBL_KEYS:
        assert_bit_equal(np.array([got[k]]), np.array([ref[k]]), f"{what}: {k}")


# --- host arrays ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cases.HOST_CASES))
def test_host_arrays_equal_oracle(gctx, name):
    s, ref = cases.host_scene(name), cases.host_reference(name)
    args = (s["kfL"], s["kfR"], s["cfL"], s["cfR"], s["w"], s["h"], s["R"], s["t"], s["calib"])
    for grid in (0, 1, 3):                                        # developer key 21: same bits for any grid
        with keys(gctx, {21: grid}):
            got = gctx.tgt_veridical(*args, cell_size=s["cell"])
            check_veridical(got, ref, f"{name} grid {grid}")
            # the scene's own quads as a stage list
            on = ot.row_on(ref["ver_row_ptr"])
            n_tp, flags, m = ot.evaluate_stage(s["row_ptr"], s["cfL"], s["cfR"], on, ref)
            g_tp, g_flags, g = gctx.tgt_evaluate_rows(s["row_ptr"], s["cfL"], s["cfR"], on, ref["proj_left"], ref["proj_right"])
            assert_bit_equal(g_tp, n_tp, f"{name}: n_tp")
            assert_bit_equal(g_flags, flags, f"{name}: flags")
            check_stage(g, m, name)
    assert len(ref["ver_idx"]) > 0
    # a given kf_gamma replaces the triangulated point
    gamma = np.random.default_rng(5).uniform([-2, -1, 4], [2, 1, 20], (len(s["kfL"]), 3))
    ref_g = ot.build_veridical_quads(s["kfL"], s["kfR"], s["cfL"], s["cfR"], s["R"], s["t"], s["calib"], s["w"], s["h"],
                                     kf_gamma=gamma, cell=s["cell"])
    check_veridical(gctx.tgt_veridical(*args, kf_gamma=gamma, cell_size=s["cell"]), ref_g, f"{name} with kf_gamma")


@pytest.mark.parametrize("which", ["margin", "cells", "orient"])
def test_border_scenes_equal_oracle(gctx, which):
    s, ref = cases.border_scene(which), cases.border_reference(which)
    got = gctx.tgt_veridical(*s["kf"], *s["cf"], cases.B_W, cases.B_H, cases.B_R, cases.B_T, cases.B_CALIB, cell_size=cases.B_CELL,
                             **s["params"])
    check_veridical(got, ref, which)


def test_host_rows_zero_return_and_empty(gctx):
    rp = np.zeros(4, dtype=np.int32)
    e = np.zeros(0, dtype=_lib.EDGE_DTYPE)
    p = np.zeros((3, 2))
    for on in (np.zeros(3, dtype=np.uint8), np.ones(3, dtype=np.uint8), None):
        n_tp, flags, g = gctx.tgt_evaluate_rows(rp, e, e, on, p, p)
        check_stage(g, ot.metrics(np.zeros((3, 2), dtype=np.int32), np.ones(3) if on is None else on), "empty rows")
        assert [g[k] for k in DBL_KEYS] == [0.0] * 4 and not n_tp.any()
    n_tp, flags, g = gctx.tgt_evaluate_rows(np.zeros(1, dtype=np.int32), e, e, None, np.zeros((0, 2)), np.zeros((0, 2)))
    assert g["rows"] == 0 and [g[k] for k in DBL_KEYS] == [0.0] * 4
    got = gctx.tgt_veridical(e, e, e, e, 200, 120, cases.B_R, cases.B_T, cases.B_CALIB)
    assert got["n_veridical"] == 0 and got["ver_row_ptr"].tolist() == [0]


# --- resident slot -------------------------------------------------------------------------------------------------------
def device_keyframe_gt(c, kf, slot):
    """kf_gamma / kf_is_tp of the keyframe in `slot` from the device's stereo ground truth, equal to tgt_cases.keyframe_gt"""
    g = cases.keyframe_gt(kf)
    sz = c.stereo_set_gt(g["disp"], CALIB, slot=slot)            # the armed keyframe slot
    assert sz["n_valid"] > 0
    L, Rm = tc.oracle_mates(kf)
    loc = c.gt_locate(L, g["disp"], CALIB)
    for k in ("valid", "gt_xy", "gamma_left"):
        assert_bit_equal(loc[k], g["loc"][k], f"keyframe {kf}: {k}")
    dx, dy = Rm["x"] - loc["gt_xy"][:, 0], Rm["y"] - loc["gt_xy"][:, 1]
    is_tp = ((loc["valid"] != 0) & (np.sqrt(dx * dx + dy * dy) <= cases.KF_TP_DIST)).astype(np.uint8)
    assert (is_tp == g["is_tp"]).all()
    return loc["gamma_left"], is_tp


def check_resident(c, r, counts, q, stages, what):
    ver, on = r["ver"], r["on"]
    f = c.temporal_gt_fetch()
    check_veridical(f, ver, what)
    assert (f["n_kf"], f["n_rows"], f["n_veridical"]) == (len(on), int((np.diff(ver["ver_row_ptr"]) > 0).sum()), len(ver["ver_idx"]))
    m = c.temporal_gt_metrics()
    assert [s["name"] for s in m] == list(ot.STAGE_NAMES)
    present = {ot.ORIENTATION, ot.NCC} | ({ot.CLUSTER} if stages else set())
    assert [s["present"] for s in m] == [k in present for k in range(8)]
    sizes = {ot.ORIENTATION: counts["n_candidates"], ot.NCC: counts["n_kept"], ot.CLUSTER: counts.get("n_final", 0)}
    for k in range(8):
        if k in present:
            n_tp, flags, ref = r["stages"][k]
            check_stage(m[k], ref, f"{what} stage {k}")
            assert_bit_equal(c.temporal_gt_flags(k, sizes[k]), flags, f"{what}: flags of stage {k}")
        else:
            assert all(m[k][key] == 0 for key in INT_KEYS + DBL_KEYS)
            with pytest.raises(EbvoError) as ei:
                c.temporal_gt_flags(k, 1)                         # absent, not zero
            assert ei.value.status == EBVO_ERR_STATE


@pytest.mark.parametrize("stages", [0, 1])
@pytest.mark.parametrize("name", list(cases.RESIDENT))
def test_resident_slot_equals_oracle(gctx, name, stages):
    c = gctx
    kf, cf, _ = cases.RESIDENT[name]
    load(c, kf)
    gamma, is_tp = device_keyframe_gt(c, kf, 0)
    c.temporal_set_keyframe()
    load(c, cf)
    with pytest.raises(EbvoError) as ei:
        c.temporal_set_gt(np.eye(3), np.zeros(3), CALIB)          # no match yet
    assert ei.value.status == EBVO_ERR_STATE
    counts, q, _ = match(c, kf, cf, stages=stages)
    for with_gt in (False, True):
        r = cases.resident_reference(name, stages, with_gt)
        sz = c.temporal_set_gt(r["R"], r["t"], r["calib"], kf_gamma=gamma if with_gt else None, kf_is_tp=is_tp if with_gt else None)
        if stages:
            e = cases.EXPECTED[(name, with_gt)]
            assert (sz["n_kf"], sz["n_rows"], sz["n_veridical"]) == (e["n_kf"], e["n_rows"], e["n_veridical"])
            fl = c.temporal_gt_flags(ot.CLUSTER, counts["n_final"])
            assert (int(fl.sum()), int(len(fl) - fl.sum())) == (e["final_tp"], e["final_not_tp"])
        for grid in (0, 1, 5):
            with keys(c, {21: grid}):
                if grid:
                    c.temporal_set_gt(r["R"], r["t"], r["calib"], kf_gamma=gamma if with_gt else None,
                                      kf_is_tp=is_tp if with_gt else None)
                check_resident(c, r, counts, q, stages, f"{name} stages {stages} gt {with_gt} grid {grid}")
    # arming changed nothing the slot holds
    counts2, q2 = c._temporal_results(0, _counts_struct(counts), stages, True)
    same_results(q, q2, f"{name}: after arming")


def _counts_struct(counts):
    s = _lib.TemporalCounts()
    for k, v in counts.items():
        setattr(s, k, v)
    return s


# --- state ---------------------------------------------------------------------------------------------------------------
def test_state_and_refusals(gctx):
    c = gctx
    load(c, "small0")
    c.temporal_set_keyframe()
    load(c, "small2")
    counts, q, _ = match(c, "small0", "small2", stages=1)
    r = cases.resident_reference("small", 1, False)
    R, t, cal = r["R"], r["t"], r["calib"]
    for call in (c.temporal_gt_size, c.temporal_gt_metrics, lambda: c.temporal_gt_flags(ot.NCC, counts["n_kept"])):
        with pytest.raises(EbvoError) as ei:
            call()                                                # not armed
        assert ei.value.status == EBVO_ERR_STATE
    c.temporal_set_gt(R, t, cal)
    before = (c.temporal_gt_fetch(), c.temporal_gt_metrics())
    # every refused call leaves the armed slot as it was
    bad_R = np.full((3, 3), np.nan)
    for kw, args in ((dict(tp_dist=-1.0), (R, t)), (dict(orient_thr_deg=float("nan")), (R, t)), (dict(search_radius=-0.5), (R, t)),
                     (dict(img_margin=-1.0), (R, t)), ({}, (bad_R, t))):
        with pytest.raises(EbvoError) as ei:
            c.temporal_set_gt(*args, cal, **kw)
        assert ei.value.status == EBVO_ERR_ARG, kw
    with pytest.raises(EbvoError) as ei:
        c.temporal_set_gt(R, t, cal, slot=7)
    assert ei.value.status == EBVO_ERR_ARG
    with pytest.raises(EbvoError) as ei:
        c.temporal_gt_flags(99, 1)
    assert ei.value.status == EBVO_ERR_ARG
    after = (c.temporal_gt_fetch(), c.temporal_gt_metrics())
    for k in VER_KEYS:
        assert_bit_equal(after[0][k], before[0][k], f"after refusals: {k}")
    assert after[1] == before[1]
    # the slot's own results are what they were
    _, q2 = c._temporal_results(0, _counts_struct(counts), 1, True)
    same_results(q, q2, "after arming")
    # the host-array twins on slot 0 leave the armed slot alone
    s = cases.host_scene("kf3")
    c.tgt_veridical(s["kfL"], s["kfR"], s["cfL"], s["cfR"], s["w"], s["h"], s["R"], s["t"], s["calib"], cell_size=s["cell"])
    check_veridical(c.temporal_gt_fetch(), r["ver"], "after the host twin")
    # a new match disarms; so does a replaced keyframe
    match(c, "small0", "small2", stages=0)
    with pytest.raises(EbvoError) as ei:
        c.temporal_gt_metrics()
    assert ei.value.status == EBVO_ERR_STATE
    c.temporal_set_gt(R, t, cal)
    m = c.temporal_gt_metrics()
    assert not m[ot.CLUSTER]["present"] and m[ot.NCC]["present"]
    load(c, "small0", slot=1)
    c.temporal_set_keyframe(slot=1)
    for call in (c.temporal_gt_metrics, lambda: c.temporal_set_gt(R, t, cal)):
        with pytest.raises(EbvoError) as ei:
            call()                                                # the keyframe was replaced since the match
        assert ei.value.status == EBVO_ERR_STATE
    # a new upload of the slot: no match to arm
    l, rr = tc.images("small2")
    c.stereo_upload(l, rr)
    with pytest.raises(EbvoError) as ei:
        c.temporal_set_gt(R, t, cal)
    assert ei.value.status == EBVO_ERR_STATE


def test_profiler_lists_the_kernels(gctx):
    s = cases.host_scene("kf64")
    gctx.profile_enable(True)
    gctx.profile_reset()
    gctx.tgt_veridical(s["kfL"], s["kfR"], s["cfL"], s["cfR"], s["w"], s["h"], s["R"], s["t"], s["calib"], cell_size=s["cell"])
    ref = cases.host_reference("kf64")
    gctx.tgt_evaluate_rows(s["row_ptr"], s["cfL"], s["cfR"], None, ref["proj_left"], ref["proj_right"])
    prof = gctx.profile_get()
    gctx.profile_enable(False)
    # (ms, launches).  The wrapper calls ebvo_tgt_veridical twice: once to size ver_idx (project, count) and once to
    # fill it (project, count, fill); the scene has veridical quads, so the second call is made
    assert prof["tgt_project"][1] == 2 and prof["tgt_veridical"][1] == 3
    assert prof["tgt_rows"][1] == 1                                # one launch per evaluated list
