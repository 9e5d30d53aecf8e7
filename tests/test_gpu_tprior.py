"""Temporal matching under a pose prior on the device (ebvo_temporal_set_prior / _clear_prior / _prior_fetch,
ebvo_tprior_candidates, and the temporal chain, its ground truth and the pose stages on a match made under a prior) against
tests/oracle_tprior.py, bit for bit: integers with ==, doubles by their bit patterns.  No device output is ever passed to
the oracle: the references come from the ORACLE's stereo mates (tests/tprior_cases.py), and the device's mates are asserted
equal to those before every match.

Inputs (tests/tprior_cases.py; tests/test_tprior_oracle.py checks their conditions without a device):
  resident      120 x 200 frames 0 and 60 of tests/temporal_cases.images under a rectified rig: priors of 60 px at radius 30
                and of 57 px at radius 8 (one cell, off-centre), the latter also with the mate's own orientations
  host arrays   tgt_cases.host_scene's 1, 3, 63, 64, 65 and 257 keyframe mates under their own pose; the three border scenes
                under the identity pose with a mate behind the cameras and a NaN mate
"""
import numpy as np
import pytest

from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EBVO_ERR_CAPACITY, EBVO_ERR_STATE, EbvoError
from tests import oracle_chain
from tests import oracle_pose as op
from tests import oracle_pose_refit as orf
from tests import oracle_tgt as ot
from tests import oracle_tprior as otp
from tests import oracle_tstages as ots
from tests import tprior_cases as cases
from tests.test_gpu_pose import _fetch_counts, assert_same
from tests.test_gpu_pose_refit import assert_refined
from tests.test_gpu_temporal_edges import keys, new_context, same_results
from tests.test_gpu_tgt import check_stage
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu

PRIOR_KEYS = ("live", "proj_left", "proj_right", "orient_left", "orient_right")
INTERIOR = (ot.SIFT, ot.BNB_NCC, ot.BNB_SIFT, ot.REFINE)


@pytest.fixture(scope="module")
def pctx():
    """a context of these tests' own (the priors, the switch and the developer keys never reach the session context)"""
    c = new_context("hybrid")
    yield c
    c.close()


def raises(status, call):
    with pytest.raises(EbvoError) as ei:
        call()
    assert ei.value.status == status, ei.value
    return str(ei.value)


def load(c, k, slot=0):
    """frame k through the stereo chain of `slot` under the rectified rig; its mates are the oracle's"""
    l, r = cases.images(k)
    c.stereo_upload(l, r, slot=slot)
    c.stereo_submit(c.default_params(cases.F), slot=slot)
    cnt = c.stereo_wait(slot=slot)
    left = c.stereo_fetch(cnt, slot=slot)["left"]
    _, fin = c.stereo_finalize(cases.CALIB, slot=slot)
    oL, oR = cases.mates(k)
    for got, ref, what in ((left[fin["left_index"]], oL, "left"), (fin["right"], oR, "right")):
        assert len(got) == len(ref), (k, what, len(got), len(ref))
        for f in ("x", "y", "theta"):
            assert_bit_equal(got[f].copy(), ref[f].copy(), f"frame {k}: {what} mate {f}")


def frames(c, slots=(0,)):
    """the keyframe stored from slot 0, the current frame in every slot of `slots`"""
    load(c, cases.KF, 0)
    c.temporal_set_keyframe(0)
    for s in slots:
        load(c, cases.CF, s)


def arm(c, name, slot=0):
    px, radius, use_orientation = cases.RESIDENT[name]
    c.temporal_set_prior(*cases.prior_pose(px), cases.CALIB, slot=slot, use_orientation=use_orientation)
    return dict(grid_radius=radius)


def check_match(c, counts, q, ref, what, slot=0):
    bad = oracle_chain.temporal_problems(counts, q, ref)
    assert bad == [], (what, bad)
    got = c.temporal_prior_fetch(slot)
    for k in PRIOR_KEYS:
        assert_bit_equal(got[k], ref["prior"][k], f"{what}: prior {k}")


def prior_match(c, name, stages, slot=0, what=""):
    kw = arm(c, name, slot)
    counts, q = c.temporal_match(slot=slot, stages=stages, **kw)
    check_match(c, counts, q, cases.case_reference(name, stages), f"{name} stages {stages} {what}", slot)
    return counts, q


def unprimed_match(c, stages, slot=0, what=""):
    counts, q = c.temporal_match(slot=slot, stages=stages)
    bad = oracle_chain.temporal_problems(counts, q, cases.unprimed_reference(stages))
    assert bad == [], (what, bad)
    raises(EBVO_ERR_STATE, lambda: c.temporal_prior_fetch(slot))
    return counts, q


# --- 1. resident parity -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stages", [0, 1])
@pytest.mark.parametrize("name", list(cases.RESIDENT))
def test_resident_match_equals_oracle(pctx, name, stages):
    frames(pctx)
    counts, q = prior_match(pctx, name, stages)
    ref = cases.case_reference(name, stages)
    assert counts["n_candidates"] == ref["counts"]["n_candidates"] > 100000
    if stages:
        assert counts["n_final"] > 1000 and cases.true_final(dict(final=q["final"])) > 1000   # the prior recovers the match


# --- 2. host arrays -----------------------------------------------------------------------------------------------------
def host_call(c, name, **kw):
    s = cases.host_case(name)
    return c.tprior_candidates(s["kfL"], s["kfR"], s["cfL"], s["cfR"], s["w"], s["h"], s["R"], s["t"], s["calib"], cell_size=s["cell"],
                               grid_radius=s["radius"], **kw)


def check_host(got, ref, what):
    for k in PRIOR_KEYS + ("row_ptr", "col_idx"):
        assert_bit_equal(got[k], ref[k], f"{what}: {k}")
    assert got["n_candidates"] == len(ref["col_idx"])


@pytest.mark.parametrize("name", cases.HOST_SCENES + ["border-" + b for b in cases.BORDER_SCENES])
def test_host_arrays_equal_oracle(pctx, name):
    ref = cases.host_reference(name)
    for grid in (0, 1, 3):                                        # developer key 21 moves the projection's grid
        with keys(pctx, {21: grid}):
            check_host(host_call(pctx, name), ref, f"{name} grid {grid}")
    n = len(ref["col_idx"])
    assert n > 0
    with pytest.raises(EbvoError) as ei:                          # one short: the count comes back
        host_call(pctx, name, cap=n - 1)
    assert ei.value.status == EBVO_ERR_CAPACITY and ei.value.n_candidates == n
    check_host(host_call(pctx, name, cap=n), ref, f"{name} exact room")
    if name.startswith("border-"):
        for margin, uo in ((10.0, 1), (0.0, 0)):
            check_host(host_call(pctx, name, img_margin=margin, use_orientation=uo), cases.host_reference(name, margin, uo),
                       f"{name} margin {margin} use_orientation {uo}")


def test_host_arrays_refusals(pctx):
    s = cases.host_case("kf3")
    args = (s["kfL"], s["kfR"], s["cfL"], s["cfR"], s["w"], s["h"])
    bad_R = np.eye(3)
    bad_R[1, 1] = np.inf
    for R, t, kw in ((bad_R, s["t"], {}), (s["R"], [0.0, np.nan, 0.0], {}), (s["R"], s["t"], dict(img_margin=-1.0)),
                     (s["R"], s["t"], dict(img_margin=np.inf)), (s["R"], s["t"], dict(cell_size=0)),
                     (s["R"], s["t"], dict(grid_radius=-1.0)), (s["R"], s["t"], dict(grid_radius=np.nan)),
                     (s["R"], s["t"], dict(orient_thr_deg=-1.0))):
        raises(EBVO_ERR_ARG, lambda: pctx.tprior_candidates(*args, R, t, s["calib"], **kw))


# --- 3. launch grids ----------------------------------------------------------------------------------------------------
def test_launch_grids_change_no_bit(pctx):
    frames(pctx)
    for grid in (1, 3, 64, 0):                                    # developer key 22: every launch of the stage, the projection included
        with keys(pctx, {22: grid}):
            prior_match(pctx, "short-r8", 1, what=f"key 22 = {grid}")
    with keys(pctx, {22: 1}):
        prior_match(pctx, "true-r30", 0, what="key 22 = 1")


# --- 4. nothing changes without a prior ---------------------------------------------------------------------------------
def test_cleared_and_consumed_priors_leave_the_unprimed_match(pctx):
    c = pctx
    frames(c)
    arm(c, "true-r30")
    c.temporal_clear_prior()
    c.temporal_clear_prior()                                      # none pending: no error
    first = unprimed_match(c, 1, what="after set + clear")
    assert cases.true_final(dict(final=first[1]["final"])) == 0    # the unprimed search does not reach 60 px
    prior_match(c, "true-r30", 1)
    again = unprimed_match(c, 1, what="after a prior match, not re-armed")
    assert again[0] == first[0]
    same_results(again[1], first[1], "one-shot")


# --- 5. capacity --------------------------------------------------------------------------------------------------------
def test_a_wider_prior_match_goes_through_the_redo():
    c = new_context("hybrid", slots=1)                            # a fresh slot: its capacity is the first match's
    try:
        frames(c)
        small, _ = prior_match(c, "short-r8", 1)
        big, _ = prior_match(c, "true-r30", 1, what="redo")
        assert big["n_candidates"] > small["n_candidates"] + small["n_candidates"] // 4 + 1024   # above the remembered capacity
        prior_match(c, "short-r8", 0, what="after the redo")
    finally:
        c.close()


# --- 6. two slots in flight ---------------------------------------------------------------------------------------------
def test_two_slots_in_flight(pctx):
    c = pctx
    frames(c, slots=(0, 1))
    names = {0: "true-r30", 1: "short-r8"}
    for slot, name in names.items():
        kw = arm(c, name, slot)
        c.temporal_match_submit(slot=slot, stages=1, **kw)
    for slot in (1, 0):
        counts, q = c.temporal_match_wait(slot=slot)
        check_match(c, counts, q, cases.case_reference(names[slot], 1), f"slot {slot}", slot)


# --- 7. state and argument rules ----------------------------------------------------------------------------------------
def test_state_and_argument_rules(pctx):
    c = pctx
    frames(c)
    R, t = cases.prior_pose(60.0)
    counts, q = prior_match(c, "short-r8", 1)
    arm(c, "true-r30")                                            # pending from here on
    bad_R = np.full((3, 3), np.nan)
    raises(EBVO_ERR_ARG, lambda: c.temporal_set_prior(bad_R, t, cases.CALIB))
    raises(EBVO_ERR_ARG, lambda: c.temporal_set_prior(R, [np.inf, 0.0, 0.0], cases.CALIB))
    raises(EBVO_ERR_ARG, lambda: c.temporal_set_prior(R, t, cases.CALIB, img_margin=-1.0))
    raises(EBVO_ERR_ARG, lambda: c.temporal_set_prior(R, t, cases.CALIB, img_margin=np.nan))
    raises(EBVO_ERR_ARG, lambda: c.temporal_set_prior(R, t, cases.CALIB, slot=9))
    raises(EBVO_ERR_ARG, lambda: c.temporal_clear_prior(slot=9))
    raises(EBVO_ERR_ARG, lambda: c.temporal_prior_fetch(slot=9))
    bad_cal = (cases.CALIB[0], cases.CALIB[1], np.full(9, np.nan), cases.CALIB[3])
    raises(EBVO_ERR_ARG, lambda: c.temporal_set_prior(R, t, bad_cal))
    # ... the slot's match stays as it was
    _, q2 = c._temporal_results(0, _fetch_counts(counts), 1, True)
    same_results(q2, q, "after the refusals")
    for k in PRIOR_KEYS:
        assert_bit_equal(c.temporal_prior_fetch()[k], cases.case_reference("short-r8", 1)["prior"][k], f"after the refusals: {k}")
    # a refused submit leaves the prior pending; the next good one consumes it
    raises(EBVO_ERR_ARG, lambda: c.temporal_match_submit(stages=1, cell_size=0))
    got = c.temporal_match(stages=0, grid_radius=30.0)
    check_match(c, *got, cases.case_reference("true-r30", 0), "the pending prior after the refusals")
    # in flight: no switch
    kw = arm(c, "short-r8")
    c.temporal_match_submit(stages=0, **kw)
    raises(EBVO_ERR_STATE, lambda: c.temporal_set_prior(R, t, cases.CALIB))
    raises(EBVO_ERR_STATE, lambda: c.temporal_clear_prior())
    raises(EBVO_ERR_STATE, lambda: c.temporal_prior_fetch())
    raises(EBVO_ERR_STATE, lambda: host_call(c, "kf3"))           # the host-array form runs on slot 0's stream
    check_match(c, *c.temporal_match_wait(), cases.case_reference("short-r8", 0), "after the in-flight refusals")
    # a new keyframe drops the pending prior: the next match runs unprimed (frame 60 against itself here)
    arm(c, "true-r30")
    c.temporal_set_keyframe()
    counts, q = c.temporal_match(stages=0)
    raises(EBVO_ERR_STATE, lambda: c.temporal_prior_fetch())
    ref = oracle_chain.temporal_reference(*cases.mates(cases.CF), *cases.mates(cases.CF), cases.triple(cases.CF), cases.triple(cases.CF),
                                          cases.W, cases.H, chain=False)
    assert oracle_chain.temporal_problems(counts, q, ref) == []


# --- 8. ground truth on a prior match that kept its trail ---------------------------------------------------------------
def test_ground_truth_of_a_prior_match(pctx):
    c = pctx
    frames(c)
    name = "true-r30"
    px, radius, _ = cases.RESIDENT[name]
    R, t = cases.prior_pose(px)
    ref = cases.case_reference(name, 1)
    (kfL, kfR), (cfL, cfR) = cases.mates(cases.KF), cases.mates(cases.CF)
    c.temporal_keep_stages(True)
    try:
        counts, q = prior_match(c, name, 1)
        c.temporal_set_gt(R, t, cases.CALIB)
        m = c.temporal_gt_metrics()
        ver = ot.build_veridical_quads(kfL, kfR, cfL, cfR, R, t, cases.CALIB, cases.W, cases.H)
        on = ot.row_on(ver["ver_row_ptr"])
        assert on.sum() > 1000 and (ref["prior"]["live"][on != 0] != 0).all() and not ref["prior"]["live"].all()
        rp, col, keep = ref["row_ptr"], ref["col_idx"], ref["keep"].astype(bool)
        final, trail = ots.temporal_edge_pairs_trail(kfL, kfR, cfL, cfR, cases.triple(cases.KF)[1:], cases.triple(cases.CF)[1:], rp, col,
                                                     ref["sim_left"], ref["keep"])
        assert ots.same_final(final, ref["final"])
        g = otp.grid_rows(kfL, kfR, cfL, cfR, ref["prior"], cases.W, cases.H, 15, radius, on, ver["proj_left"], ver["proj_right"])
        want = {ot.GRID: (g, ot.metrics(g, on)),
                ot.ORIENTATION: ot.evaluate_stage(rp, cfL[col], cfR[col], on, ver)[::2],
                ot.NCC: ot.evaluate_stage(oracle_chain.filter_rows(rp, keep), cfL[col[keep]], cfR[col[keep]], on, ver)[::2],
                ot.CLUSTER: ot.evaluate_stage(final["row_ptr"], final["left"], final["right"], on, ver)[::2]}
        for k in INTERIOR:
            want[k] = ot.evaluate_stage(trail[k]["row_ptr"], trail[k]["left"], trail[k]["right"], on, ver)[::2]
        for k in range(8):
            assert m[k]["present"], k
            check_stage(m[k], want[k][1], f"stage {k}")
            assert_bit_equal(c.temporal_gt_stage_rows(k), want[k][0], f"rows of stage {k}")
        # the unprimed walk around the keyframe positions would have counted other cells
        un = ots.grid_rows(kfL, kfR, cfL, cfR, cases.W, cases.H, 15, radius, on, ver["proj_left"], ver["proj_right"])
        assert (un != g).any() and m[ot.GRID]["sum_tp"] > 1000
    finally:
        c.temporal_keep_stages(False)


# --- 9. downstream ------------------------------------------------------------------------------------------------------
def test_pose_stages_take_a_prior_match_as_any_other(pctx):
    c = pctx
    frames(c)
    counts, q = prior_match(c, "short-r8", 1)
    fin = cases.case_reference("short-r8", 1)["final"]
    kfL, kfR = cases.mates(cases.KF)
    args = (kfL, kfR, fin["row_ptr"], fin["left"], fin["right"])
    cal = cases.CALIB
    got = c.temporal_estimate_pose(cal)
    ref = op.estimate_pose(*args, cal[0], cal[2], cal[3])
    assert_same(got, ref, geom=False)
    assert got["found"] and abs(got["t"][0] - cases.prior_pose(60.0)[1][0]) < 0.05      # the scene's motion, not the prior's 57 px
    refined = c.temporal_refine_pose(cal, got["R"], got["t"])
    assert_refined(refined, orf.refit(*args, cal[0], cal[2], cal[3], ref["R"], ref["t"]), "refit on a prior match")
