"""The handover of the refined depths to the next keyframe on the device (ebvo_depth_carry, ebvo_temporal_promote_keyframe,
ebvo_temporal_depth_source) against its CPU restatement tests/oracle_carry.py: the state arrays, the flags, src_index and
every field of ebvo_depth_carried bit for bit (integers with ==, doubles by their bit patterns).  The cases are
tests/carry_cases.py, each with the branch it exercises; tests/test_carry_oracle.py checks without a device that each case
meets its condition.  The resident tests run on the frames tests/test_gpu_depth.py builds."""
import numpy as np
import pytest

from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EBVO_ERR_STATE
from tests import carry_cases as cc
from tests import oracle_carry as oc
from tests import oracle_depth as od
from tests.test_gpu_depth import ALIGN_KW, H, W, assert_aligned, assert_state, current, host_step, keyframe, pose, raises
from tests.test_gpu_temporal_edges import CALIB, new_context
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu

STATE = ("lambda_", "info", "n_obs", "flags", "src_index")
CASES = cc.cases()


@pytest.fixture(scope="module")
def cctx():
    """a context of these tests' own (developer key 22 never reaches the session context)"""
    c = new_context("hybrid", slots=2)
    yield c
    c.close()


def assert_carried(got, ref, what=""):
    for k in oc.INT_FIELDS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in STATE:
        assert_bit_equal(got[k], ref[k], f"{what} {k}")


def device(c, case, **kw):
    return c.depth_carry(case["kf_left"], case["kf_right"], case["new_left"], case["new_right"], case["img_w"], case["img_h"], case["calib"],
                         case["R"], case["t"], state=case["state"], **dict(case["params"], **kw))


@pytest.mark.parametrize("name", list(CASES))
def test_bit_parity_with_the_oracle(cctx, name):
    case = CASES[name]()
    ref = cc.run_oracle(case)
    assert case["check"](ref), f"{name}: the case does not meet its condition ({case['note']})"
    assert_carried(device(cctx, case), ref, f"{name}: {case['note']}")


@pytest.mark.parametrize("name", cc.PICKED)
def test_launch_geometry_changes_no_bit(cctx, name):
    """developer key 22 at 1, 2 and 7 blocks, and a second call"""
    c, case = cctx, CASES[name]()
    ref = cc.run_oracle(case)
    try:
        for blocks in (1, 2, 7):
            c.debug_set(22, blocks)
            assert_carried(device(c, case), ref, f"{name} key 22 = {blocks}")
    finally:
        c.debug_set(22, 0)
    assert_carried(device(c, case), ref, f"{name} again")
    assert_carried(device(c, case), ref, f"{name} a second call")


# ---- resident ------------------------------------------------------------------------------------------------------------
def finalized(c, k, slot=0):
    """frame k through the stereo chain and the finalisation of the slot: its kept TOED edge lists and its final mates"""
    _, E0, E1 = current(c, k, slot=slot)
    _, fin = c.stereo_finalize(CALIB, slot=slot)
    return E0, E1, E0[fin["left_index"]].copy(), fin["right"].copy()


def fused_keyframe(c):
    """keyframe = frame 0, frames 1 and 2 fused, frame 2 finalised on slot 0: (old mates, old state, frame 2's final mates)"""
    kfL, kfR = keyframe(c)
    current(c, 1)
    c.temporal_refine_depth(CALIB, *pose(1))
    _, _, nL, nR = finalized(c, 2)
    c.temporal_refine_depth(CALIB, *pose(2))
    return kfL, kfR, c.temporal_depth_fetch(), nL, nR


def same_quads(a, b, what):
    (ca, qa), (cb, qb) = a, b
    assert ca == cb, (what, ca, cb)
    lists = [(k, qa[k], qb[k]) for k in ("row_ptr", "col_idx", "sim_left", "sim_right", "keep")]
    lists += [(f"final {k}", v, qb["final"][k]) for k, v in qa["final"].items()]
    for k, x, y in lists:
        for f in x.dtype.names or (None,):
            assert_bit_equal(x if f is None else x[f].copy(), y if f is None else y[f].copy(), f"{what} {k} {f or ''}")


@pytest.fixture(scope="module")
def promoted(cctx):
    """the promotion of frame 2 under its pose, the host form on the fetched arrays and the oracle: computed once"""
    c = cctx
    kfL, kfR, old, nL, nR = fused_keyframe(c)
    R, t = pose(2)
    rec = c.temporal_promote_keyframe(CALIB, R, t)
    now = dict(c.temporal_depth_fetch(), src_index=c.temporal_depth_source())
    st = (old["lambda_"], old["info"], old["n_obs"])
    host = c.depth_carry(kfL, kfR, nL, nR, W, H, CALIB, R, t, state=st)
    ref = oc.carry(kfL, kfR, nL, nR, W, H, CALIB, R, t, state=st)
    return dict(rec=rec, now=now, host=host, ref=ref, old=old, nL=nL, nR=nR)


def test_promotion_equals_the_host_form_and_the_oracle(cctx, promoted):
    p = promoted
    print("promotion record:", p["rec"])
    assert (p["old"]["n_obs"] > 0).sum() > 50
    assert_carried(p["host"], p["ref"], "host form against the oracle")
    assert_carried(dict(p["rec"], **p["now"]), p["ref"], "resident form against the oracle")
    assert p["rec"]["n_new"] == len(p["nL"]) > 100 and p["rec"]["n_live"] > 50 and p["rec"]["n_carried"] > 20
    assert (p["now"]["lambda_"] != 1.0).sum() > 20 and p["now"]["n_obs"].max() == 2


def test_the_store_is_the_one_set_keyframe_installs(cctx, promoted):
    """a temporal match of frame 3 against the promoted keyframe and, in a second context, against the same frame installed
    by ebvo_temporal_set_keyframe: the same quads and counts"""
    finalized(cctx, 3)
    got = cctx.temporal_match(stages=1)
    c2 = new_context("hybrid", slots=1)
    try:
        finalized(c2, 2)
        c2.temporal_set_keyframe()
        finalized(c2, 3)
        want = c2.temporal_match(stages=1)
        raises(EBVO_ERR_STATE, lambda: c2.temporal_depth_source())
    finally:
        c2.close()
    assert got[0]["n_kf"] == promoted["rec"]["n_new"] and got[0]["n_candidates"] > 0
    same_quads(got, want, "promoted against set")
    assert_state(cctx.temporal_depth_fetch(), promoted["now"], "the carried state after a match")


def test_refine_depth_continues_from_the_carried_state(cctx, promoted):
    c, p = cctx, promoted
    _, E0, E1 = current(c, 3)
    R, t = pose(1)
    got = c.temporal_refine_depth(CALIB, R, t, align=ALIGN_KW)
    try:
        state = (p["now"]["lambda_"], p["now"]["info"], p["now"]["n_obs"])
        host = host_step(c, p["nL"], p["nR"], E0, E1, R, t, state, 2)
        for f in ("n_kf", "n_dead", "n_updated", "n_restored", "n_terms", "n_gated", "rms_before", "rms_after"):
            assert_bit_equal(np.asarray(got[f], dtype=np.float64), np.asarray(host[f], dtype=np.float64), f)
        assert_state(c.temporal_depth_fetch(), host, "after the fusion on the carried state")
        assert got["n_updated"] > 50 and host["n_obs"].max() == 3
        assert_bit_equal(c.temporal_depth_source(), p["now"]["src_index"], "src_index after a fusion")
    finally:
        # back to the carried state for the tests that follow: the same promotion again
        fused_keyframe(c)
        c.temporal_promote_keyframe(CALIB, *pose(2))
    assert_state(dict(c.temporal_depth_fetch()), p["now"], "the promotion repeated")


def test_the_alignment_consumes_the_carried_lambda(cctx, promoted):
    c, p = cctx, promoted
    _, E0, E1 = current(c, 3)
    R, t = pose(1)
    R0, t0 = od.oa.op.rot((0.3, -1.0, 0.2), 0.004) @ R, t + np.array([0.004, -0.003, 0.005])
    akw = dict(rounds=2, iterations=4)
    lam = c.temporal_depth_fetch()["lambda_"]
    assert_bit_equal(lam, p["now"]["lambda_"], "the carried lambda")
    try:
        c.temporal_use_depth(True)
        on = c.temporal_align_pose(CALIB, R0, t0, **akw)
    finally:
        c.temporal_use_depth(False)
    off = c.temporal_align_pose(CALIB, R0, t0, **akw)
    assert_aligned(on, c.pose_align_edges(p["nL"], p["nR"], E0, E1, W, H, CALIB, R0, t0, lambda_=lam, **akw), "on the carried lambda")
    assert_aligned(off, c.pose_align_edges(p["nL"], p["nR"], E0, E1, W, H, CALIB, R0, t0, **akw), "switch off")
    assert any(np.asarray(on[k]).tobytes() != np.asarray(off[k]).tobytes() for k in ("R", "t")), "the carried lambda changed nothing"


def test_a_keyframe_that_fused_nothing_promotes_to_the_prior():
    c = new_context("hybrid", slots=1)
    try:
        kfL, _ = keyframe(c)
        fresh = c.temporal_depth_fetch()
        _, _, nL, _ = finalized(c, 2)
        rec = c.temporal_promote_keyframe(CALIB, *pose(2))
        assert rec == dict(n_old=len(kfL), n_sources=0, n_live=0, n_new=len(nL), n_dead=0, n_assoc=0, n_carried=0, n_gated=0)
        now = c.temporal_depth_fetch()
        assert len(now["lambda_"]) == len(nL)
        assert all(now["lambda_"] == 1.0) and not now["info"].any() and not now["n_obs"].any() and not now["flags"].any()
        assert all(c.temporal_depth_source() == -1)
        # exactly as after ebvo_temporal_set_keyframe: the first fusion starts from the prior
        current(c, 3)
        c.temporal_refine_depth(CALIB, *pose(1))
        first = c.temporal_depth_fetch()
        finalized(c, 2)
        c.temporal_set_keyframe()
        assert_state(c.temporal_depth_fetch(), dict(now), "set_keyframe reads the same prior")
        current(c, 3)
        c.temporal_refine_depth(CALIB, *pose(1))
        assert_state(c.temporal_depth_fetch(), first, "first fusion after either door")
        assert len(fresh["lambda_"]) == len(kfL)
    finally:
        c.close()


def test_refused_calls_leave_the_keyframe_and_its_state_alone():
    c = new_context("hybrid", slots=2)
    try:
        R, t = pose(2)
        finalized(c, 2)
        raises(EBVO_ERR_STATE, lambda: c.temporal_promote_keyframe(CALIB, R, t))              # no keyframe
        assert c.lib.ebvo_temporal_depth_source(c._ctx, None) == EBVO_ERR_STATE
        fused_keyframe(c)
        before, size = c.temporal_depth_fetch(), len(c.temporal_depth_fetch()["lambda_"])
        for kw in (dict(carry=np.nan), dict(carry=0.0), dict(carry=1.5), dict(radius=np.nan), dict(radius=0.0), dict(radius=40.0), dict(cell_size=0),
                   dict(sigma_disp_px=np.nan), dict(sigma_disp_px=0.0), dict(gate_sigmas=0.0), dict(gate_sigmas=np.nan), dict(min_obs=-1),
                   dict(lambda_min=0.0), dict(lambda_min=2.0, lambda_max=1.0), dict(lambda_max=np.inf), dict(info_max=0.0), dict(info_max=np.nan),
                   dict(img_margin=-1.0), dict(orient_thr_deg=np.nan), dict(reserved=1)):
            raises(EBVO_ERR_ARG, lambda: c.temporal_promote_keyframe(CALIB, R, t, **kw))      # a NaN or out-of-range parameter
            raises(EBVO_ERR_ARG, lambda: c.depth_carry(*_host_args(), **kw))
        Rn, ti = np.array(R, dtype=np.float64).copy(), np.array(t, dtype=np.float64).copy()
        Rn[1, 2] = np.nan
        ti[0] = np.inf
        for R0, t0 in ((Rn, t), (R, ti)):
            raises(EBVO_ERR_ARG, lambda: c.temporal_promote_keyframe(CALIB, R0, t0))          # a non-finite pose
        raises(EBVO_ERR_ARG, lambda: c.temporal_promote_keyframe(CALIB, R, t, slot=99))
        finalized(c, 3, slot=1)
        c.temporal_match_submit(slot=1, stages=1)
        try:
            raises(EBVO_ERR_STATE, lambda: c.temporal_promote_keyframe(CALIB, R, t))          # a match in flight in another slot
        finally:
            c.temporal_match_wait(slot=1)
        assert_state(c.temporal_depth_fetch(), before, "after the refused calls")
        current(c, 1)                                                                         # a pair that is not finalised
        raises(EBVO_ERR_STATE, lambda: c.temporal_promote_keyframe(CALIB, R, t))              # no final mates
        assert_state(c.temporal_depth_fetch(), before, "after the refusal without final mates")
        assert len(c.temporal_depth_fetch()["lambda_"]) == size
        raises(EBVO_ERR_STATE, lambda: c.temporal_depth_source())                             # still the keyframe set_keyframe installed
        # the slot and the keyframe still work: the promotion goes through
        finalized(c, 2)
        rec = c.temporal_promote_keyframe(CALIB, R, t)
        assert rec["n_old"] == size and rec["n_carried"] > 20
    finally:
        c.close()


def _host_args():
    case = CASES["n_new_65"]()
    return (case["kf_left"], case["kf_right"], case["new_left"], case["new_right"], case["img_w"], case["img_h"], case["calib"], case["R"],
            case["t"], case["state"])
