"""The keyframe coverage on the device (ebvo_keyframe_cover_edges, ebvo_temporal_keyframe_cover) against its CPU restatement
tests/oracle_cover.py: every integer of ebvo_keyframe_cover with ==, flags, assoc, explained, both cell planes, hist and disp
by their bit patterns.  The cases are tests/cover_cases.py, each with the branch it exercises; tests/test_cover_oracle.py
checks without a device that each case meets its condition.  The resident tests run on the frames tests/test_gpu_depth.py
builds."""
import ctypes

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib
from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EBVO_ERR_STATE
from tests import cover_cases as cc
from tests import oracle_cover as ocv
from tests.test_gpu_carry import finalized, same_quads
from tests.test_gpu_depth import H, W, assert_state, current, keyframe, pose, raises
from tests.test_gpu_temporal_edges import CALIB, new_context
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu

CASES = cc.cases()


@pytest.fixture(scope="module")
def vctx():
    """a context of these tests' own (developer key 22 never reaches the session context)"""
    c = new_context("hybrid", slots=2)
    yield c
    c.close()


def assert_cover(got, ref, what=""):
    for k in ocv.INT_FIELDS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in ocv.ARRAYS:
        assert got[k].dtype == ref[k].dtype, (what, k, got[k].dtype, ref[k].dtype)
        assert_bit_equal(got[k], ref[k], f"{what} {k}")


def device(c, case, **kw):
    return c.keyframe_cover_edges(case["kf_left"], case["kf_right"], case["edges_left"], case["img_w"], case["img_h"], case["calib"],
                                  case["R"], case["t"], lambda_=case["lambda_"], **dict(case["params"], **kw))


@pytest.mark.parametrize("name", list(CASES))
def test_bit_parity_with_the_oracle(vctx, name):
    case = CASES[name]()
    ref = cc.run_oracle(case)
    assert case["check"](ref), f"{name}: the case does not meet its condition ({case['note']})"
    assert_cover(device(vctx, case), ref, f"{name}: {case['note']}")


@pytest.mark.parametrize("name", cc.PICKED)
def test_launch_geometry_changes_no_bit(vctx, name):
    """developer key 22 at 1, 2 and 7 blocks, and a second call"""
    c, case = vctx, CASES[name]()
    ref = cc.run_oracle(case)
    try:
        for blocks in (1, 2, 7):
            c.debug_set(22, blocks)
            assert_cover(device(c, case), ref, f"{name} key 22 = {blocks}")
    finally:
        c.debug_set(22, 0)
    assert_cover(device(c, case), ref, f"{name} again")
    assert_cover(device(c, case), ref, f"{name} a second call")


def test_null_outputs_are_accepted(vctx):
    c, case = vctx, CASES["kitti_all"]()
    ref = cc.run_oracle(case)
    got = device(c, case, arrays=False)
    assert set(got) == set(ocv.INT_FIELDS) | {"hist"}
    for k in ocv.INT_FIELDS:
        assert got[k] == ref[k], k
    assert_bit_equal(got["hist"], ref["hist"], "hist")
    # one output at a time
    p, cal, r = c.cover_params(**case["params"]), c._calib(case["calib"]), _lib.KeyframeCover()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    kfL, kfR, E0 = (np.ascontiguousarray(case[k]) for k in ("kf_left", "kf_right", "edges_left"))
    Rc, tc_ = np.ascontiguousarray(case["R"], dtype=np.float64).reshape(9), np.ascontiguousarray(case["t"], dtype=np.float64)
    lam = np.ascontiguousarray(case["lambda_"])
    for pos, key in enumerate(("flags", "assoc", "disp", "explained", "cell_edges", "cell_explained")):
        out = np.zeros_like(ref[key])
        outs = [None] * 6
        outs[pos] = ptr(out)
        c._check(c.lib.ebvo_keyframe_cover_edges(c._ctx, ptr(kfL), ptr(kfR), ptr(lam), len(kfL), ptr(E0), len(E0), case["img_w"], case["img_h"],
                                                 ctypes.byref(cal), ctypes.byref(p), ptr(Rc), ptr(tc_), ctypes.byref(r), *outs),
                 "ebvo_keyframe_cover_edges")
        assert_bit_equal(out, ref[key], key)
        assert r.n_assoc == ref["n_assoc"]


BAD = [dict(radius=0.0), dict(radius=-1.0), dict(radius=np.nan), dict(radius=np.inf), dict(radius=40.0), dict(cell_size=0), dict(orient_thr_deg=-1.0),
       dict(orient_thr_deg=np.nan), dict(img_margin=-1.0), dict(img_margin=np.nan), dict(inlier_px=-1.0), dict(inlier_px=np.nan), dict(bin_px=0.0),
       dict(bin_px=-1.0), dict(bin_px=np.inf), dict(bin_px=np.nan), dict(cover_cell=0), dict(cover_cell=-3), dict(min_cell_edges=0),
       dict(min_cell_explained=0), dict(reserved=1), dict(pad=1)]


# ---- resident ------------------------------------------------------------------------------------------------------------
COVER_KW = dict(radius=3.0, cell_size=5, orient_thr_deg=12.0, cover_cell=24, bin_px=0.25)


def test_refused_calls_leave_the_state_alone(vctx):
    c = vctx
    keyframe(c)
    current(c, 1)
    R, t = pose(1)
    c.temporal_refine_depth(CALIB, R, t)
    before = c.temporal_depth_fetch()
    case = CASES["n_kf_65"]()
    Rn, ti = np.array(R, dtype=np.float64).copy(), np.array(t, dtype=np.float64).copy()
    Rn[1, 2] = np.nan
    ti[0] = np.inf
    for kw in BAD:
        raises(EBVO_ERR_ARG, lambda: c.temporal_keyframe_cover(CALIB, R, t, **kw))
        raises(EBVO_ERR_ARG, lambda: c.temporal_keyframe_cover(CALIB, R, t, arrays=False, **kw))
        raises(EBVO_ERR_ARG, lambda: device(c, case, **kw))
    for R0, t0 in ((Rn, t), (R, ti)):
        raises(EBVO_ERR_ARG, lambda: c.temporal_keyframe_cover(CALIB, R0, t0))
        raises(EBVO_ERR_ARG, lambda: device(c, dict(case, R=R0, t=t0)))
    raises(EBVO_ERR_ARG, lambda: c.temporal_keyframe_cover(CALIB, R, t, slot=99))
    raises(EBVO_ERR_ARG, lambda: device(c, dict(case, img_w=0)))
    raises(EBVO_ERR_STATE, lambda: c.temporal_keyframe_cover(CALIB, R, t, slot=1))      # no waited pair on slot 1
    p, cal = c.cover_params(), c._calib(CALIB)
    Rc, tc_ = np.ascontiguousarray(R, dtype=np.float64).reshape(9), np.ascontiguousarray(t, dtype=np.float64)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert c.lib.ebvo_temporal_keyframe_cover(c._ctx, 0, ctypes.byref(cal), ctypes.byref(p), ptr(Rc), ptr(tc_), None, None, None, None, None,
                                              None, None) == EBVO_ERR_ARG           # no record
    assert_state(c.temporal_depth_fetch(), before, "after the refused calls")
    fresh = new_context("hybrid", slots=1)
    try:
        raises(EBVO_ERR_STATE, lambda: fresh.temporal_keyframe_cover(CALIB, R, t))       # no keyframe, no pair
        raises(EBVO_ERR_STATE, lambda: fresh.temporal_keyframe_pose())
    finally:
        fresh.close()


def test_resident_form_equals_the_host_form_and_the_oracle(vctx):
    c = vctx
    kfL, kfR = keyframe(c)
    assert len(kfL) > 100
    for k in (1, 3):
        pair, E0, E1 = current(c, k)
        R, t = pose(k)
        before = c.temporal_depth_fetch()
        got = c.temporal_keyframe_cover(CALIB, R, t, **COVER_KW)
        host = c.keyframe_cover_edges(kfL, kfR, E0, W, H, CALIB, R, t, **COVER_KW)
        ref = ocv.cover(kfL, kfR, None, E0, W, H, CALIB, R, t, **COVER_KW)
        print(f"frame {k}:", {f: ref[f] for f in ocv.INT_FIELDS})
        assert_cover(host, ref, f"frame {k}: host form against the oracle")
        assert_cover(got, ref, f"frame {k}: resident form against the oracle")
        assert ref["n_in_frame"] > 100 and ref["n_assoc"] > 50 and ref["n_explained"] > 50 and ref["n_cells_cur"] > 0
        after = c.stereo_fetch(pair)                            # the slot's pair reads the same
        assert_bit_equal(after["left"], E0, "left edges")
        assert_bit_equal(after["right"], E1, "right edges")
        assert_state(c.temporal_depth_fetch(), before, "the depth state")


def test_resident_form_on_the_fused_lambda(vctx):
    """two fused frames, ebvo_temporal_use_depth on: the resident call works on Gamma / lambda, off: on Gamma"""
    c = vctx
    kfL, kfR = keyframe(c)
    for k in (1, 2):
        current(c, k)
        c.temporal_refine_depth(CALIB, *pose(k))
    _, E0, _ = current(c, 3)
    R, t = pose(3)
    state = c.temporal_depth_fetch()
    lam = state["lambda_"]
    assert (lam != 1.0).sum() > 50
    try:
        c.temporal_use_depth(True)
        on = c.temporal_keyframe_cover(CALIB, R, t, **COVER_KW)
    finally:
        c.temporal_use_depth(False)
    off = c.temporal_keyframe_cover(CALIB, R, t, **COVER_KW)
    assert_cover(on, c.keyframe_cover_edges(kfL, kfR, E0, W, H, CALIB, R, t, lambda_=lam, **COVER_KW), "on: the host form given the fetched lambda")
    assert_cover(on, ocv.cover(kfL, kfR, lam, E0, W, H, CALIB, R, t, **COVER_KW), "on: the oracle on Gamma / lambda")
    assert_cover(off, ocv.cover(kfL, kfR, None, E0, W, H, CALIB, R, t, **COVER_KW), "off: the oracle on Gamma")
    assert on["disp"].tobytes() != off["disp"].tobytes(), "lambda changed nothing"
    assert_state(c.temporal_depth_fetch(), state, "the depth state")


def test_a_temporal_match_is_not_disturbed(vctx):
    c = vctx
    keyframe(c)
    finalized(c, 2)
    first = c.temporal_match(stages=1)
    c.temporal_keyframe_cover(CALIB, *pose(2), **COVER_KW)
    c.temporal_keyframe_cover(CALIB, *pose(2), arrays=False)
    same_quads(c.temporal_match(stages=1), first, "a match after the cover call")
    assert first[0]["n_candidates"] > 0
