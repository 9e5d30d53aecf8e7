"""The inverse-depth filter of the keyframe mates on the device (ebvo_depth_refine_edges, ebvo_temporal_refine_depth, the state
calls, ebvo_temporal_use_depth, ebvo_pose_align_edges_depth) against its CPU restatement tests/oracle_depth.py: the state
arrays, the flags and every field of ebvo_depth_refined bit for bit (integers with ==, doubles by their bit patterns).  The
cases are tests/depth_cases.py, each with the branch it exercises; tests/test_depth_oracle.py checks without a device that each
case meets its condition."""
import ctypes

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib, synth
from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EBVO_ERR_STATE, EbvoError
from tests import depth_cases as dc
from tests import oracle_align as oa
from tests import oracle_depth as od
from tests import temporal_cases as tc
from tests import tgt_cases
from tests.test_gpu_temporal_edges import CALIB, load, new_context
from tests.test_gpu_temporal_edges import F as F_RIG
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu

INT_FIELDS = ("n_kf", "n_dead", "n_updated", "n_restored", "n_terms", "n_gated")
STATE = ("lambda_", "info", "n_obs", "flags")
CASES = dc.cases()
KF = "small0"
H, W = tc.FRAMES[KF][:2]


@pytest.fixture(scope="module")
def dctx():
    """a context of these tests' own (developer key 22 never reaches the session context)"""
    c = new_context("hybrid")
    yield c
    c.close()


def assert_refined(got, ref, what=""):
    for k in INT_FIELDS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in ("rms_before", "rms_after"):
        assert_bit_equal(np.float64(got[k]), np.float64(ref[k]), f"{what} {k}")
    for k in STATE:
        assert_bit_equal(got[k], ref[k], f"{what} {k}")


def assert_state(got, ref, what=""):
    for k in STATE:
        assert_bit_equal(got[k], ref[k], f"{what} {k}")


def device(c, case, **kw):
    return c.depth_refine_edges(case["kf_left"], case["kf_right"], case["edges_left"], case["edges_right"], case["assoc_left"],
                                case["assoc_right"], case["img_w"], case["img_h"], case["calib"], case["R"], case["t"], state=case["state"],
                                **dict(case["params"], **kw))


@pytest.mark.parametrize("name", list(CASES))
def test_bit_parity_with_the_oracle(dctx, name):
    case = CASES[name]()
    ref = dc.run_oracle(case)
    assert case["check"](ref), f"{name}: the case does not meet its condition ({case['note']})"
    assert_refined(device(dctx, case), ref, f"{name}: {case['note']}")


def test_right_list_may_be_null_with_one_camera(dctx):
    case = CASES["n_kf_65_cameras_1"]()
    assert_refined(device(dctx, dict(case, edges_right=None, assoc_right=None)), dc.run_oracle(case), "NULL right list")


@pytest.mark.parametrize("name", ["kitti_all", "n_kf_1025_cameras_2", "gate_small", "second_update"])
def test_launch_geometry_changes_no_bit(dctx, name):
    """block_threads 256 / 512 / 1024, developer key 22 at 1, 2 and 7 blocks, and a second call"""
    c, case = dctx, CASES[name]()
    ref = dc.run_oracle(case)
    for bt in (0, 256, 512, 1024):
        assert_refined(device(c, case, block_threads=bt), ref, f"{name} block {bt}")
    try:
        for blocks in (1, 2, 7):
            c.debug_set(22, blocks)
            assert_refined(device(c, case), ref, f"{name} key 22 = {blocks}")
            assert_refined(device(c, case, block_threads=256), ref, f"{name} key 22 = {blocks}, block 256")
    finally:
        c.debug_set(22, 0)
    assert_refined(device(c, case), ref, f"{name} again")


# ---- resident ------------------------------------------------------------------------------------------------------------
def frame(k):
    """the scene of tests/temporal_cases.py::images moved by k px, at the small size"""
    l, r = synth.stereo_pair("s2", H, W, scene=7, noise_base=2 * k, disparity=9)
    return np.ascontiguousarray(np.roll(l, k, axis=1)), np.ascontiguousarray(np.roll(r, k, axis=1))


def pose(k):
    return tgt_cases.resident_pose(0.625 * k)


def keyframe(c):
    load(c, KF)
    c.temporal_set_keyframe()
    return tc.oracle_mates(KF)


def current(c, k, slot=0):
    """frame k through the stereo chain of the slot: its kept TOED edge lists"""
    l, r = frame(k)
    c.stereo_upload(l, r, slot=slot)
    c.stereo_submit(c.default_params(F_RIG), slot=slot)
    pair = c.stereo_wait(slot=slot)
    f = c.stereo_fetch(pair, slot=slot)
    return pair, f["left"].copy(), f["right"].copy()


ALIGN_KW = dict(radius=3.0, cell_size=5, orient_thr_deg=12.0)


def host_step(c, kfL, kfR, E0, E1, R, t, state, cameras, **dp):
    """the host-array form of one resident update: the association of the host alignment under the start pose (no step), which
    is the oracle's, then the update"""
    lam = None if state is None else state[0]
    a = c.pose_align_edges(kfL, kfR, E0, E1, W, H, CALIB, R, t, lambda_=lam, rounds=1, iterations=0, cameras=cameras, **ALIGN_KW)
    ref = od.associate(kfL, kfR, lam, E0, E1 if cameras > 1 else None, W, H, CALIB, R, t, cameras=cameras, **ALIGN_KW)
    assert_bit_equal(a["assoc_left"], ref[0], "assoc_left")
    assert_bit_equal(a["assoc_right"], ref[1], "assoc_right")
    got = c.depth_refine_edges(kfL, kfR, E0, E1, a["assoc_left"], a["assoc_right"], W, H, CALIB, R, t, state=state, cameras=cameras, **dp)
    want = od.update(kfL, kfR, E0, E1, ref[0], ref[1], W, H, CALIB, R, t, state=state, cameras=cameras, **dp)
    assert_refined(got, want, "host form against the oracle")
    return got


@pytest.mark.parametrize("cameras", [2, 1])
def test_resident_form_equals_the_host_form_chained(dctx, cameras):
    c = dctx
    kfL, kfR = keyframe(c)
    n = len(kfL)
    assert n > 100
    fresh = c.temporal_depth_fetch()
    assert all(fresh["lambda_"] == 1.0) and not fresh["info"].any() and not fresh["n_obs"].any() and not fresh["flags"].any()
    dp = dict(gate_px=2.0, sigma_normal_px=0.4)
    state = None
    for k in (1, 2, 3):
        pair, E0, E1 = current(c, k)
        R, t = pose(k)
        got = c.temporal_refine_depth(CALIB, R, t, align=ALIGN_KW, cameras=cameras, **dp)
        host = host_step(c, kfL, kfR, E0, E1, R, t, state, cameras, **dp)
        for f in INT_FIELDS + ("rms_before", "rms_after"):
            assert_bit_equal(np.asarray(got[f], dtype=np.float64), np.asarray(host[f], dtype=np.float64), f"frame {k}: {f}")
        now = c.temporal_depth_fetch()
        assert_state(now, host, f"frame {k}")
        assert got["n_kf"] == n and got["n_updated"] > 50
        after = c.stereo_fetch(pair)                            # the slot's pair reads the same
        assert_bit_equal(after["left"], E0, "left edges")
        assert_bit_equal(after["right"], E1, "right edges")
        state = (host["lambda_"], host["info"], host["n_obs"])
    assert state[2].max() == 3
    # back to the prior through either door; the next update starts from it again
    pair, E0, E1 = current(c, 1)
    first = host_step(c, kfL, kfR, E0, E1, *pose(1), None, cameras, **dp)
    c.temporal_depth_reset()
    assert_state(c.temporal_depth_fetch(), fresh, "after the reset")
    c.temporal_refine_depth(CALIB, *pose(1), align=ALIGN_KW, cameras=cameras, **dp)
    assert_state(c.temporal_depth_fetch(), first, "first update after the reset")
    keyframe(c)
    assert_state(c.temporal_depth_fetch(), fresh, "after a new keyframe")
    current(c, 1)
    c.temporal_refine_depth(CALIB, *pose(1), align=ALIGN_KW, cameras=cameras, **dp)
    assert_state(c.temporal_depth_fetch(), first, "first update after a new keyframe")


def raises(status, call):
    with pytest.raises(EbvoError) as ei:
        call()
    assert ei.value.status == status


def test_state_errors():
    c = new_context("hybrid", slots=2)
    try:
        R, t = pose(1)
        raises(EBVO_ERR_STATE, lambda: c.temporal_refine_depth(CALIB, R, t))          # no keyframe, no pair
        raises(EBVO_ERR_STATE, lambda: c.temporal_depth_reset())
        assert c.lib.ebvo_temporal_depth_fetch(c._ctx, None, None, None, None) == EBVO_ERR_STATE
        load(c, KF)
        raises(EBVO_ERR_STATE, lambda: c.temporal_refine_depth(CALIB, R, t))          # a pair, no keyframe
        c.temporal_set_keyframe()
        raises(EBVO_ERR_STATE, lambda: c.temporal_refine_depth(CALIB, R, t, slot=1))  # a keyframe, no waited pair on slot 1
        ok = c.temporal_refine_depth(CALIB, R, t)                                     # the keyframe's own pair will do
        state = c.temporal_depth_fetch()
        l, r = frame(1)
        c.stereo_upload(l, r, slot=0)
        c.stereo_submit(c.default_params(F_RIG), slot=0)
        try:
            raises(EBVO_ERR_STATE, lambda: c.temporal_refine_depth(CALIB, R, t))      # the slot in flight
            raises(EBVO_ERR_STATE, lambda: device(c, CASES["n_kf_65_cameras_2"]()))   # the host form runs on slot 0
        finally:
            c.stereo_wait(slot=0)
        assert ok["n_kf"] > 100
        assert_state(c.temporal_depth_fetch(), state, "after the refused calls")
    finally:
        c.close()


BAD = [dict(sigma_disp_px=0.0), dict(sigma_disp_px=-1.0), dict(sigma_disp_px=np.inf), dict(sigma_disp_px=np.nan), dict(sigma_normal_px=0.0),
       dict(sigma_normal_px=np.inf), dict(sigma_normal_px=np.nan), dict(huber_px=0.0), dict(huber_px=-1.0), dict(huber_px=np.nan),
       dict(gate_px=0.0), dict(gate_px=-2.0), dict(gate_px=np.nan), dict(iterations=-1), dict(iterations=17), dict(lambda_min=0.0),
       dict(lambda_min=-0.5), dict(lambda_min=np.nan), dict(lambda_min=2.0, lambda_max=1.5), dict(lambda_max=np.inf), dict(lambda_max=np.nan),
       dict(info_max=0.0), dict(info_max=-1.0), dict(info_max=np.nan), dict(img_margin=-1.0), dict(img_margin=np.nan), dict(cameras=0),
       dict(cameras=3), dict(block_threads=128), dict(block_threads=2048), dict(reserved=1)]


def test_refused_calls_leave_the_state_alone(dctx):
    c = dctx
    keyframe(c)
    current(c, 1)
    R, t = pose(1)
    c.temporal_refine_depth(CALIB, R, t)
    before = c.temporal_depth_fetch()
    case = CASES["n_kf_65_cameras_2"]()
    Rn, ti = np.array(R, dtype=np.float64).copy(), np.array(t, dtype=np.float64).copy()
    Rn[1, 2] = np.nan
    ti[0] = np.inf
    for kw in BAD:
        raises(EBVO_ERR_ARG, lambda: c.temporal_refine_depth(CALIB, R, t, **kw))
        raises(EBVO_ERR_ARG, lambda: device(c, case, **kw))
    for R0, t0 in ((Rn, t), (R, ti)):
        raises(EBVO_ERR_ARG, lambda: c.temporal_refine_depth(CALIB, R0, t0))
        raises(EBVO_ERR_ARG, lambda: device(c, dict(case, R=R0, t=t0)))
    for akw in (dict(radius=0.0), dict(cell_size=0), dict(orient_thr_deg=np.nan), dict(radius=33.0, cell_size=4)):
        raises(EBVO_ERR_ARG, lambda: c.temporal_refine_depth(CALIB, R, t, align=akw))
    raises(EBVO_ERR_ARG, lambda: c.temporal_refine_depth(CALIB, R, t, slot=99))
    raises(EBVO_ERR_ARG, lambda: device(c, dict(case, img_w=0)))
    lam, info, nobs = np.ones(65), np.ones(65), np.zeros(65, dtype=np.int32)
    assert c.lib.ebvo_temporal_use_depth(None, 1) == EBVO_ERR_ARG
    assert_state(c.temporal_depth_fetch(), before, "after the refused calls")
    # an incoming state is three arrays or none
    p, cal, r = c.depth_params(), c._calib(case["calib"]), _lib.DepthRefined()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    kfL, kfR, E0, E1 = (np.ascontiguousarray(case[k]) for k in ("kf_left", "kf_right", "edges_left", "edges_right"))
    Rc, tc_ = np.ascontiguousarray(case["R"], dtype=np.float64), np.ascontiguousarray(case["t"], dtype=np.float64)
    fl = np.zeros(65, dtype=np.uint8)
    rc = c.lib.ebvo_depth_refine_edges(c._ctx, ptr(kfL), ptr(kfR), 65, ptr(E0), len(E0), ptr(E1), len(E1), ptr(case["assoc_left"]),
                                       ptr(case["assoc_right"]), case["img_w"], case["img_h"], ctypes.byref(cal), ctypes.byref(p), ptr(Rc),
                                       ptr(tc_), ptr(lam), None, ptr(nobs), ptr(lam), ptr(info), ptr(nobs), ptr(fl), ctypes.byref(r))
    assert rc == EBVO_ERR_ARG


# ---- the consumer ----------------------------------------------------------------------------------------------------------
def assert_aligned(got, ref, what=""):
    for k in ("status", "stop_reason", "rounds_run", "steps_kept", "n_kf", "fit_terms", "inliers", "n_assoc"):
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in ("cost_first", "cost_last", "rms_normal"):
        assert_bit_equal(np.float64(got[k]), np.float64(ref[k]), f"{what} {k}")
    for k in ("R", "t", "assoc_left", "assoc_right"):
        assert_bit_equal(got[k], ref[k], f"{what} {k}")


def test_the_alignment_consumes_the_refined_depths(dctx):
    c = dctx
    kfL, kfR = keyframe(c)
    akw = dict(rounds=2, iterations=4)
    try:
        _, E0, E1 = current(c, 2)
        R, t = pose(2)
        R0, t0 = oa.op.rot((0.3, -1.0, 0.2), 0.004) @ R, t + np.array([0.004, -0.003, 0.005])
        plain = oa.align(kfL, kfR, E0, E1, W, H, CALIB, R0, t0, **akw)
        off = c.temporal_align_pose(CALIB, R0, t0, **akw)
        assert_aligned(off, plain, "switch off, at the prior")
        # on, at the prior, and on with every lambda = 1 (an update of no step): the bits of the switch off
        c.temporal_use_depth(True)
        assert_aligned(c.temporal_align_pose(CALIB, R0, t0, **akw), plain, "switch on, at the prior")
        c.temporal_refine_depth(CALIB, R, t, iterations=0)
        ones = c.temporal_depth_fetch()
        assert all(ones["lambda_"] == 1.0) and ones["n_obs"].max() == 1
        assert_aligned(c.temporal_align_pose(CALIB, R0, t0, **akw), plain, "switch on, every lambda = 1")
        # fused lambda: the resident form, the host form and the oracle on Gamma / lambda agree
        c.temporal_depth_reset()
        fused = c.temporal_refine_depth(CALIB, R, t)
        lam = c.temporal_depth_fetch()["lambda_"]
        assert fused["n_updated"] > 50 and (lam != 1.0).sum() > 50
        ref = od.align(kfL, kfR, lam, E0, E1, W, H, CALIB, R0, t0, **akw)
        assert_aligned(c.temporal_align_pose(CALIB, R0, t0, **akw), ref, "resident on Gamma / lambda")
        assert_aligned(c.pose_align_edges(kfL, kfR, E0, E1, W, H, CALIB, R0, t0, lambda_=lam, **akw), ref, "host on Gamma / lambda")
        assert any(np.asarray(ref[k]).tobytes() != np.asarray(plain[k]).tobytes() for k in ("R", "t")), "lambda changed nothing"
        # the switch off after a fusion: the parent's results on the same inputs
        c.temporal_use_depth(False)
        assert_aligned(c.temporal_align_pose(CALIB, R0, t0, **akw), plain, "switch off after a fusion")
        assert_aligned(c.pose_align_edges(kfL, kfR, E0, E1, W, H, CALIB, R0, t0, **akw), plain, "host, no lambda")
        # lambda = NULL through the new symbol
        p, cal, r = c.align_params(**akw), c._calib(CALIB), _lib.AlignedPose()
        ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        aL, aR = np.full(len(kfL), -1, dtype=np.int32), np.full(len(kfL), -1, dtype=np.int32)
        Rc, tc_ = np.ascontiguousarray(R0, dtype=np.float64).reshape(9), np.ascontiguousarray(t0, dtype=np.float64)
        kl, kr, e0, e1 = (np.ascontiguousarray(v) for v in (kfL, kfR, E0, E1))
        c._check(c.lib.ebvo_pose_align_edges_depth(c._ctx, ptr(kl), ptr(kr), None, len(kl), ptr(e0), len(e0), ptr(e1), len(e1), W, H,
                                                   ctypes.byref(cal), ctypes.byref(p), ptr(Rc), ptr(tc_), ctypes.byref(r), ptr(aL), ptr(aR)),
                 "ebvo_pose_align_edges_depth")
        assert_aligned(c._aligned_dict(r, aL, aR), plain, "lambda = NULL")
    finally:
        c.temporal_use_depth(False)
