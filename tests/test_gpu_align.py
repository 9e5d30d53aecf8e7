"""The alignment of the pose to the current frame's TOED edges on the device (ebvo_pose_align_edges, ebvo_temporal_align_pose)
against its CPU restatement tests/oracle_align.py: every field of ebvo_aligned_pose, the pose and both association arrays, bit
for bit (integers with ==, doubles by their bit patterns).  The cases are tests/align_cases.py, each with the branch it
exercises; tests/test_align_oracle.py checks without a device that the list reaches every status and stop reason."""
import ctypes

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib, synth
from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EBVO_ERR_STATE, EbvoError
from tests import align_cases as ac
from tests import oracle_align as oa
from tests import tgt_cases
from tests.test_gpu_temporal_edges import CALIB, load, new_context
from tests.test_gpu_temporal_edges import F as F_RIG
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu

INT_FIELDS = ("status", "stop_reason", "rounds_run", "steps_kept", "n_kf", "fit_terms", "inliers", "n_assoc")
CASES = ac.cases()


@pytest.fixture(scope="module")
def actx():
    """a context of these tests' own (developer key 22 never reaches the session context)"""
    c = new_context("hybrid")
    yield c
    c.close()


def assert_aligned(got, ref, what=""):
    for k in INT_FIELDS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in ("cost_first", "cost_last", "rms_normal"):
        assert_bit_equal(np.float64(got[k]), np.float64(ref[k]), f"{what} {k}")
    assert_bit_equal(got["R"], ref["R"], f"{what} R")
    assert_bit_equal(got["t"], ref["t"], f"{what} t")
    assert_bit_equal(got["assoc_left"], ref["assoc_left"], f"{what} assoc_left")
    assert_bit_equal(got["assoc_right"], ref["assoc_right"], f"{what} assoc_right")


def device(c, case, **kw):
    return c.pose_align_edges(case["kf_left"], case["kf_right"], case["edges_left"], case["edges_right"], case["img_w"], case["img_h"],
                              case["calib"], case["R0"], case["t0"], **dict(case["params"], **kw))


@pytest.mark.parametrize("name", list(CASES))
def test_bit_parity_with_the_oracle(actx, name):
    case = CASES[name]()
    ref = ac.run_oracle(case)
    got = device(actx, case)
    assert_aligned(got, ref, f"{name}: {case['note']}")
    if got["status"]:                                       # 1 and 2 return the start pose
        assert_bit_equal(got["R"], case["R0"], "start R")
        assert_bit_equal(got["t"], case["t0"], "start t")


def test_right_list_may_be_null_with_one_camera(actx):
    case = CASES["cameras_1"]()
    assert_aligned(device(actx, dict(case, edges_right=None)), ac.run_oracle(case), "NULL right list")


@pytest.mark.parametrize("name", ["kitti_all", "n_kf_1025", "few_later", "segment_33"])
def test_launch_geometry_changes_no_bit(actx, name):
    """block_threads 256 / 512 / 1024, developer key 22 at 1, 2 and 7 blocks, and a second call (the tile counter re-armed)"""
    c, case = actx, CASES[name]()
    ref = ac.run_oracle(case)
    for bt in (0, 256, 512, 1024):
        assert_aligned(device(c, case, block_threads=bt), ref, f"{name} block {bt}")
    try:
        for blocks in (1, 2, 7):
            c.debug_set(22, blocks)
            assert_aligned(device(c, case), ref, f"{name} key 22 = {blocks}")
            assert_aligned(device(c, case, block_threads=256), ref, f"{name} key 22 = {blocks}, block 256")
    finally:
        c.debug_set(22, 0)
    assert_aligned(device(c, case), ref, f"{name} again")


def _resident(c, prior):
    """the small resident pair of tests/tgt_cases.py: keyframe, current frame, temporal match (under a prior or not), armed GT;
    returns the temporal counts, the reference pose and the current pair's stereo counts"""
    from tests import temporal_cases as tc
    kf, cf, _ = tgt_cases.RESIDENT["small"]
    load(c, kf)
    c.temporal_set_keyframe()
    l, rr = tc.images(cf)
    c.stereo_upload(l, rr)
    c.stereo_submit(c.default_params(F_RIG))
    pair = c.stereo_wait()
    c.stereo_finalize(CALIB)
    r = tgt_cases.resident_reference("small", 1, False)
    if prior:
        c.temporal_set_prior(r["R"], r["t"], r["calib"])
    counts, q = c.temporal_match(stages=1)
    c.temporal_set_gt(r["R"], r["t"], r["calib"])
    return counts, r, pair


def _slot_edges(c, pair):
    n_kf, n0, n1 = (ctypes.c_int32() for _ in range(3))
    c._check(c.lib.ebvo_temporal_align_size(c._ctx, 0, ctypes.byref(n_kf), ctypes.byref(n0), ctypes.byref(n1)), "align_size")
    assert (n0.value, n1.value) == (pair.n_left, pair.n_right)
    f = c.stereo_fetch(pair)
    return n_kf.value, f["left"], f["right"]


@pytest.mark.parametrize("prior", [False, True])
def test_resident_form_equals_the_host_form(actx, prior):
    from tests import temporal_cases as tc
    from tests.test_gpu_pose_gt import assert_snapshot_unchanged, snapshot
    c = actx
    counts, r, pair = _resident(c, prior)
    kf, cf, _ = tgt_cases.RESIDENT["small"]
    h, w = tc.FRAMES[cf][:2]
    kfL, kfR = tc.oracle_mates(kf)
    before = snapshot(c, counts, CALIB)
    prior_before = c.temporal_prior_fetch() if prior else None
    n_kf, E0, E1 = _slot_edges(c, pair)
    assert n_kf == len(kfL) > 100 and len(E0) > 1000 and len(E1) > 1000
    for kw in (dict(rounds=2, iterations=4), dict(rounds=2, iterations=4, cameras=1), dict(rounds=1, iterations=2, radius=8.0, cell_size=15)):
        got = c.temporal_align_pose(CALIB, r["R"], r["t"], **kw)
        host = c.pose_align_edges(kfL, kfR, E0, E1, w, h, CALIB, r["R"], r["t"], **kw)
        ref = oa.align(kfL, kfR, E0, E1, w, h, CALIB, r["R"], r["t"], **kw)
        assert_aligned(host, ref, f"host {kw}")
        assert_aligned(got, ref, f"resident {kw}")
        assert got["n_kf"] == n_kf and got["fit_terms"] > 100
    # the slot reads the same: its pair, the final quads, the armed ground truth, the search's random stream, the prior
    after = c.stereo_fetch(pair)
    assert_bit_equal(after["left"], E0, "left edges")
    assert_bit_equal(after["right"], E1, "right edges")
    assert_snapshot_unchanged(c, counts, CALIB, before, "after the alignments")
    if prior:
        now = c.temporal_prior_fetch()
        for k in prior_before:
            assert_bit_equal(np.asarray(now[k]), np.asarray(prior_before[k]), f"prior {k}")


def raises(status, call):
    with pytest.raises(EbvoError) as ei:
        call()
    assert ei.value.status == status


def test_state_errors():
    c = new_context("hybrid", slots=2)
    try:
        R, t = np.eye(3), np.zeros(3)
        raises(EBVO_ERR_STATE, lambda: c.temporal_align_pose(CALIB, R, t))        # no keyframe, no pair
        kf, cf, _ = tgt_cases.RESIDENT["small"]
        load(c, kf)
        raises(EBVO_ERR_STATE, lambda: c.temporal_align_pose(CALIB, R, t))        # a pair, no keyframe
        c.temporal_set_keyframe()
        raises(EBVO_ERR_STATE, lambda: c.temporal_align_pose(CALIB, R, t, slot=1))  # a keyframe, no pair on slot 1
        ok = c.temporal_align_pose(CALIB, R, t, rounds=1, iterations=1)           # the keyframe's own pair will do
        l, r = synth.stereo_pair("s2", 96, 160)
        c.stereo_upload(l, r, slot=0)
        c.stereo_submit(c.default_params(F_RIG), slot=0)
        try:
            raises(EBVO_ERR_STATE, lambda: c.temporal_align_pose(CALIB, R, t))    # the slot in flight
            case = CASES["n_kf_16"]()
            raises(EBVO_ERR_STATE, lambda: device(c, case))                       # the host form runs on slot 0
        finally:
            c.stereo_wait(slot=0)
        assert ok["n_kf"] > 100
    finally:
        c.close()


BAD = [dict(rounds=0), dict(rounds=17), dict(iterations=-1), dict(iterations=101), dict(radius=0.0), dict(radius=-1.0),
       dict(radius=np.inf), dict(radius=np.nan), dict(cell_size=0), dict(cell_size=-4), dict(radius=8.5, cell_size=1),
       dict(radius=33.0, cell_size=4), dict(orient_thr_deg=-1.0), dict(orient_thr_deg=np.nan), dict(huber_px=0.0), dict(huber_px=-1.0),
       dict(huber_px=np.nan), dict(inlier_px=-0.5), dict(inlier_px=np.nan), dict(step_eps=-1e-12), dict(step_eps=np.nan),
       dict(min_terms=5), dict(img_margin=-1.0), dict(img_margin=np.nan), dict(cameras=0), dict(cameras=3), dict(block_threads=128),
       dict(block_threads=2048)]


def test_refused_calls_leave_the_slot_alone(actx):
    from tests.test_gpu_pose_gt import assert_snapshot_unchanged, snapshot
    c = actx
    counts, r, _ = _resident(c, False)
    before = snapshot(c, counts, CALIB)
    ok = c.temporal_align_pose(CALIB, r["R"], r["t"], rounds=1, iterations=2)
    case = CASES["n_kf_65"]()
    Rn, ti = np.array(r["R"], dtype=np.float64).copy(), np.array(r["t"], dtype=np.float64).copy()
    Rn[1, 2] = np.nan
    ti[0] = np.inf
    for kw in BAD:
        raises(EBVO_ERR_ARG, lambda: c.temporal_align_pose(CALIB, r["R"], r["t"], **kw))
        raises(EBVO_ERR_ARG, lambda: device(c, case, **kw))
    for R0, t0 in ((Rn, r["t"]), (r["R"], ti)):
        raises(EBVO_ERR_ARG, lambda: c.temporal_align_pose(CALIB, R0, t0))
        raises(EBVO_ERR_ARG, lambda: device(c, dict(case, R0=R0, t0=t0)))
    raises(EBVO_ERR_ARG, lambda: c.temporal_align_pose(CALIB, r["R"], r["t"], slot=99))
    raises(EBVO_ERR_ARG, lambda: device(c, dict(case, img_w=0)))
    raises(EBVO_ERR_ARG, lambda: device(c, dict(case, img_w=1 << 20, img_h=1 << 20), cell_size=1))   # more than 2^26 cells
    assert_snapshot_unchanged(c, counts, CALIB, before, "after the refused calls")
    again = c.temporal_align_pose(CALIB, r["R"], r["t"], rounds=1, iterations=2)
    assert_aligned(again, ok, "after the refused calls")
