"""The tracking calls (ebvo_temporal_align_pose, _refine_depth, _keyframe_cover, _promote_keyframe, _track_frame, the resident
pose search and its refit) on other slots than 0 and with work of other slots in flight, on the frames tests/test_gpu_depth.py
builds.  The other GPU files pin these calls against their CPU restatements on slot 0 of a context that runs nothing else;
here the same calls are held to the same bits where a frame loop makes them: on the slot the frame lives in, beside the next
pair's chain, a finalisation or a temporal match of another slot.  The references are a second context that makes the same
calls on slot 0 with nothing in flight, the host-array forms and tests/oracle_cover.py.  Integers with ==, doubles and arrays
by their bit patterns; no tolerance.  Nothing here asserts that kernels overlapped in time: legality and bits only."""
import contextlib

import numpy as np
import pytest

from edge_based_visual_odometry_amd import synth
from edge_based_visual_odometry_amd._lib import EBVO_ERR_STATE, TRACK_STAGE_PROMOTE, EbvoError
from tests import oracle_cover as ocv
from tests import track_loop as tl
from tests.test_gpu_carry import finalized, same_quads
from tests.test_gpu_cover import assert_cover
from tests.test_gpu_depth import H, KF, W, assert_aligned, assert_state, current, keyframe, raises
from tests.test_gpu_fullsize import _calib as full_calib
from tests.test_gpu_pose import assert_same
from tests.test_gpu_pose_refit import assert_refined as assert_refit
from tests.test_gpu_temporal_edges import CALIB, load, new_context
from tests.test_gpu_track import AKW, CKW, DKW, ONLY_PARALLAX, explicit_frame, probe, start  # noqa: F401 (probe is a fixture)
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu

STEP_KW = dict(align=AKW, depth=DKW, cover=CKW)
FULL_H, FULL_W = synth.SHAPES["euroc"]
FULL_F = synth.fundamental_for("euroc")


# ---- 1. every resident tracking call on slot 1 -----------------------------------------------------------------------------
def test_every_resident_call_on_slot_1_equals_slot_0_of_a_twin():
    """context T: the keyframe comes from slot 1 and frames 1 and 2 live there, while slot 0 holds a waited pair of another size;
    context R: the same calls on slot 0 of a context with one slot"""
    T, R = new_context("hybrid", slots=2), new_context("hybrid", slots=1)
    try:
        load(T, KF, slot=1)
        T.temporal_set_keyframe(slot=1)
        kfL, kfR = keyframe(R)
        # the bystander: a pair of another size on slot 0 of T, so that a size, a list or a workspace taken from slot 0 shows
        bl, br = synth.stereo_pair("s2", 96, 160)
        T.stereo_upload(bl, br, slot=0)
        T.stereo_submit(T.default_params(tl.F_RIG), slot=0)
        bystander = tl.collect(T, 0)
        assert bystander[0].n_left > 100
        for c in (T, R):
            c.temporal_use_depth(True)
        for k in (1, 2):
            pT, E0, E1 = current(T, k, slot=1)
            pR, E0r, E1r = current(R, k)
            assert_bit_equal(E0["x"].copy(), E0r["x"].copy(), f"frame {k}: left edges")
            assert len(E0) != bystander[0].n_left, "the bystander has the frame's edge count: it would hide a slot-0 read"
            # the sizes
            assert tl.align_size(T, 1) == tl.align_size(R, 0) == (len(kfL), len(E0), len(E1))
            assert tl.cover_size(T, 1, **CKW) == tl.cover_size(R, 0, **CKW) == (len(kfL), len(E0), -(-W // 24), -(-H // 24))
            assert tl.align_size(T, 0) == (len(kfL), bystander[0].n_left, bystander[0].n_right)
            # the pose
            a, ar = T.temporal_align_pose(CALIB, *start(k, 0), slot=1, **AKW), R.temporal_align_pose(CALIB, *start(k, 0), **AKW)
            assert_aligned(a, ar, f"frame {k}: pose on slot 1")
            assert a["status"] == 0 and a["n_assoc"][0] > 50
            Rp, tp = a["R"], a["t"]
            # the depths
            d, dr = T.temporal_refine_depth(CALIB, Rp, tp, slot=1, align=AKW, **DKW), R.temporal_refine_depth(CALIB, Rp, tp, align=AKW, **DKW)
            tl.same_depth_record(d, dr, f"frame {k}: depth on slot 1")
            assert d["n_updated"] > 50
            state = T.temporal_depth_fetch(slot=1)
            assert_state(state, R.temporal_depth_fetch(), f"frame {k}: the depth state")
            # the coverage, against the twin and against the oracle under the returned pose
            cov, covr = T.temporal_keyframe_cover(CALIB, Rp, tp, slot=1, **CKW), R.temporal_keyframe_cover(CALIB, Rp, tp, **CKW)
            assert_cover(cov, covr, f"frame {k}: cover on slot 1")
            assert_cover(cov, ocv.cover(kfL, kfR, state["lambda_"], E0, W, H, CALIB, Rp, tp, **CKW), f"frame {k}: cover against the oracle")
            tl.same_keyframe_pose(T.temporal_keyframe_pose(), R.temporal_keyframe_pose(), f"frame {k}")
            tl.same_pair((bystander[0], T.stereo_fetch(bystander[0], slot=0)), bystander, f"frame {k}: the bystander on slot 0")
        # frame 2 becomes the keyframe from slot 1
        finT, finR = T.stereo_finalize(CALIB, slot=1), R.stereo_finalize(CALIB)
        tl.same_final(finT, finR, "the finalisation on slot 1")
        rec, recr = T.temporal_promote_keyframe(CALIB, Rp, tp, slot=1), R.temporal_promote_keyframe(CALIB, Rp, tp)
        assert rec == recr and rec["n_carried"] > 20, (rec, recr)
        assert_bit_equal(T.temporal_depth_source(slot=1), R.temporal_depth_source(), "temporal_depth_source")
        assert_state(T.temporal_depth_fetch(slot=1), R.temporal_depth_fetch(), "the carried state")
        tl.same_keyframe_pose(T.temporal_keyframe_pose(), R.temporal_keyframe_pose(), "after the promotion")
        assert T.temporal_keyframe_pose()[1].any()
        tl.same_pair((bystander[0], T.stereo_fetch(bystander[0], slot=0)), bystander, "the bystander after the promotion")
        nL, nR = E0[finT[1]["left_index"]].copy(), finT[1]["right"].copy()
        # a match of frame 3 on slot 0 of T against the keyframe that slot 1 installed, the pose search and the refit on it
        finalized(T, 3, slot=0)
        finalized(R, 3)
        got, want = T.temporal_match(slot=0, stages=1), R.temporal_match(stages=1)
        same_quads(got, want, "the match of frame 3 on slot 0 against the keyframe from slot 1")
        assert got[0]["n_candidates"] > 0 and got[0]["n_final"] > 2 and got[0]["n_kf"] == len(nL)
        fin = got[1]["final"]
        args = (nL, nR, fin["row_ptr"], fin["left"], fin["right"])
        est = T.temporal_estimate_pose(CALIB, slot=0, continue_stream=0)
        assert_same(est, T.pose_from_quads(*args, CALIB), geom=False)
        assert_same(est, R.temporal_estimate_pose(CALIB, continue_stream=0), geom=False)
        assert est["n_quads"] == got[0]["n_final"] == len(est["inlier"])
        fit = T.temporal_refine_pose(CALIB, est["R"], est["t"], slot=0)
        assert_refit(fit, T.pose_refine_from_quads(*args, CALIB, est["R"], est["t"]), "the refit against the host form")
        assert_refit(fit, R.temporal_refine_pose(CALIB, est["R"], est["t"]), "the refit against the twin")
        assert fit["n_quads"] == got[0]["n_final"]
    finally:
        T.close()
        R.close()


# ---- 2. the pipelined frame loop ------------------------------------------------------------------------------------------
LOOP = (1, 2, 3, 4, 5)


@pytest.fixture(scope="module")
def sequential(probe):
    """frames 1 .. 5 one after the other on the one slot of context S: upload, chain, wait, step"""
    S = new_context("hybrid", slots=1)
    try:
        keyframe(S)
        S.temporal_use_depth(True)
        kf, rows = 0, {}
        for k in LOOP:
            tl.submit(S, k, 0)
            pair = tl.collect(S, 0)
            step = S.temporal_track_frame(CALIB, *start(k, kf), **STEP_KW, policy=probe)
            rows[k] = dict(step=step, pair=pair, state=S.temporal_depth_fetch(), kpose=S.temporal_keyframe_pose(),
                           src=S.temporal_depth_source() if step["switched"] else None)
            if step["switched"]:
                kf = k
        tl.submit(S, 6, 0)
        rows[6] = dict(pair=tl.collect(S, 0))
        S.stereo_finalize(CALIB)
        nxt = S.temporal_match(stages=1)
    finally:
        S.close()
    return dict(rows=rows, next=nxt, policy=probe)


def test_the_sequential_loop_switches_at_frame_3_only(sequential):
    rows = sequential["rows"]
    decisions = [rows[k]["step"]["decision"] for k in LOOP]
    print("decisions:", decisions, "median bins:", [rows[k]["step"]["cover"]["disp_median_bin"] for k in LOOP])
    assert decisions == [0, 0, 1, 0, 0]
    assert [rows[k]["step"]["switched"] for k in LOOP] == [0, 0, 1, 0, 0]
    assert all(rows[k]["step"]["tracked"] == 1 and rows[k]["step"]["failed_stage"] == 0 for k in LOOP)


@pytest.mark.parametrize("upload", ["upload", "async"])
def test_the_pipelined_loop_equals_the_sequential_one(sequential, upload):
    """context P: frame k lives on slot k % 2; frame k + 1 is uploaded and submitted on the other slot BEFORE frame k is tracked
    and waited for after it, so every step -- frame 3's finalisation and promotion included -- runs beside a chain in flight"""
    want, policy = sequential["rows"], sequential["policy"]
    P = new_context("hybrid", slots=2)
    try:
        keyframe(P)
        P.temporal_use_depth(True)
        tl.submit(P, 1, 1, upload)
        pairs = {1: tl.collect(P, 1)}
        kf, decisions = 0, []
        for k in LOOP:
            s, o = k % 2, (k + 1) % 2
            tl.submit(P, k + 1, o, upload)
            raises(EBVO_ERR_STATE, lambda: tl.align_size(P, o))                  # the library holds the other slot in flight
            step = P.temporal_track_frame(CALIB, *start(k, kf), slot=s, **STEP_KW, policy=policy)
            pairs[k + 1] = tl.collect(P, o)
            w = want[k]
            decisions.append(step["decision"])
            tl.same_step(step, w["step"], f"frame {k}")
            assert_state(P.temporal_depth_fetch(slot=s), w["state"], f"frame {k}: the depth state")
            tl.same_keyframe_pose(P.temporal_keyframe_pose(), w["kpose"], f"frame {k}")
            if step["switched"]:
                assert_bit_equal(P.temporal_depth_source(slot=s), w["src"], f"frame {k}: temporal_depth_source")
                assert step["carried"]["n_carried"] > 20 and step["finalized"]["n_final"] == step["carried"]["n_new"]
                kf = k
        assert decisions == [0, 0, 1, 0, 0]                                      # frame 3 switched with frame 4's chain in flight
        assert want[3]["step"]["failed_stage"] == 0 and want[3]["step"]["switched"] == 1
        # the chains that ran beside the steps left what they leave alone
        for k in (*LOOP, 6):
            tl.same_pair(pairs[k], want[k]["pair"], f"frame {k}: the pair of the pipelined loop")
        P.stereo_finalize(CALIB, slot=0)
        got = P.temporal_match(slot=0, stages=1)
        same_quads(got, sequential["next"], "the match of frame 6 after the pipelined loop")
        assert got[0]["n_candidates"] > 0
    finally:
        P.close()


# ---- 3. beside a full-size pair, a finalisation and a match in flight --------------------------------------------------------
def calls(c, around, promote_around=True):
    """keyframe 0 and frame 1 on slot 0, then the four calls, each inside around(name); returns everything they leave"""
    kfL, kfR = keyframe(c)
    c.temporal_use_depth(True)
    _, E0, E1 = current(c, 1)
    out = dict(E0=E0)
    with around("align"):
        a = out["align"] = c.temporal_align_pose(CALIB, *start(1, 0), **AKW)
    assert a["status"] == 0
    with around("depth"):
        out["depth"] = c.temporal_refine_depth(CALIB, a["R"], a["t"], align=AKW, **DKW)
    out["state"] = c.temporal_depth_fetch()
    with around("cover"):
        out["cover"] = c.temporal_keyframe_cover(CALIB, a["R"], a["t"], **CKW)
    out["fin"] = c.stereo_finalize(CALIB)
    with around("promote") if promote_around else contextlib.nullcontext():
        out["carried"] = c.temporal_promote_keyframe(CALIB, a["R"], a["t"])
    out.update(carried_state=c.temporal_depth_fetch(), src=c.temporal_depth_source(), kpose=c.temporal_keyframe_pose())
    return out


def same_calls(a, b, what):
    assert_aligned(a["align"], b["align"], f"{what}: align")
    tl.same_depth_record(a["depth"], b["depth"], f"{what}: depth")
    assert_state(a["state"], b["state"], f"{what}: the depth state")
    assert_cover(a["cover"], b["cover"], f"{what}: cover")
    tl.same_final(a["fin"], b["fin"], f"{what}: the finalisation")
    assert a["carried"] == b["carried"], (what, a["carried"], b["carried"])
    assert_state(a["carried_state"], b["carried_state"], f"{what}: the carried state")
    assert_bit_equal(a["src"], b["src"], f"{what}: temporal_depth_source")
    tl.same_keyframe_pose(a["kpose"], b["kpose"], what)


@pytest.fixture(scope="module")
def alone():
    """the call sequence with nothing in flight, and the full-size pair and its finalisation on their own: taken once"""
    c = new_context("hybrid", slots=1)
    try:
        out = calls(c, lambda name: contextlib.nullcontext())
        assert out["depth"]["n_updated"] > 50 and out["carried"]["n_carried"] > 20 and out["cover"]["n_assoc"] > 50
        l, r = synth.stereo_pair("s2", FULL_H, FULL_W)
        c.stereo_upload(l, r)
        c.stereo_submit(c.default_params(FULL_F))
        out["full"] = tl.collect(c, 0)
        out["full_final"] = c.stereo_finalize(full_calib("euroc"))
        assert out["full"][0].n_left > 50000 and out["full_final"][0]["n_final"] > 5000
    finally:
        c.close()
    return dict(out, images=(l, r))


@pytest.mark.parametrize("beside", ["pair", "finalize", "match"])
def test_calls_on_slot_0_beside_work_in_flight_on_slot_2(alone, beside):
    Q = new_context("hybrid", slots=3)
    try:
        if beside == "match":
            # slot 2 holds frame 2, finalised; its match against keyframe 0 is taken solo first (calls() installs that keyframe
            # again: the same bits)
            keyframe(Q)
            finalized(Q, 2, slot=2)
            solo = Q.temporal_match(slot=2, stages=1)
            assert solo[0]["n_candidates"] > 0
        else:
            Q.stereo_upload(*alone["images"], slot=2)
            Q.stereo_submit(Q.default_params(FULL_F), slot=2)
            tl.same_pair(tl.collect(Q, 2), alone["full"], "the full-size pair on slot 2, solo")
        seen = []

        @contextlib.contextmanager
        def around(name):
            if beside == "pair":
                Q.stereo_submit(Q.default_params(FULL_F), slot=2)
            elif beside == "finalize":
                Q.stereo_finalize_submit(full_calib("euroc"), slot=2)
            else:
                Q.temporal_match_submit(slot=2, stages=1)
            try:
                raises(EBVO_ERR_STATE, lambda: tl.align_size(Q, 2))              # the library holds slot 2 in flight
                yield
            finally:
                if beside == "pair":
                    got = tl.collect(Q, 2)
                elif beside == "finalize":
                    got = Q.stereo_finalize_wait(slot=2)
                else:
                    got = Q.temporal_match_wait(slot=2)
            if beside == "pair":
                tl.same_pair(got, alone["full"], f"the pair that ran beside {name}")
            elif beside == "finalize":
                tl.same_final(got, alone["full_final"], f"the finalisation that ran beside {name}")
                tl.same_pair((alone["full"][0], Q.stereo_fetch(alone["full"][0], slot=2)), alone["full"], f"the pair after {name}")
            else:
                same_quads(got, solo, f"the match that ran beside {name}")
            seen.append(name)

        # under a match in flight the promotion is refused (tests/test_gpu_carry.py pins that): it is made after the wait
        got = calls(Q, around, promote_around=beside != "match")
        assert seen == ["align", "depth", "cover"] + ["promote"] * (beside != "match")
        same_calls(got, alone, f"beside a {beside} in flight")
    finally:
        Q.close()


# ---- 4. a promotion refused inside the step ----------------------------------------------------------------------------------
def test_a_promotion_refused_inside_the_step_leaves_the_keyframe():
    """a match in flight on slot 1, a policy that switches on every frame: the step on slot 0 aligns, fuses, measures, finalises
    and is refused at the promotion.  Context D makes the explicit calls with nothing in flight."""
    policy = dict(ONLY_PARALLAX, max_disp_bins=0)
    C, D = new_context("hybrid", slots=2), new_context("hybrid", slots=1)
    try:
        keyframe(C)
        mates = keyframe(D)
        for c in (C, D):
            c.temporal_use_depth(True)
        finalized(C, 2, slot=1)
        solo = C.temporal_match(slot=1, stages=1)
        assert solo[0]["n_candidates"] > 0
        current(C, 1)
        kpose, n_kf = C.temporal_keyframe_pose(), tl.align_size(C, 0)[0]
        raises(EBVO_ERR_STATE, lambda: C.temporal_depth_source())                # the keyframe was set, not promoted
        C.temporal_match_submit(slot=1, stages=1)
        try:
            with pytest.raises(EbvoError) as ei:
                C.temporal_track_frame(CALIB, *start(1, 0), **STEP_KW, policy=policy)
        finally:
            got = C.temporal_match_wait(slot=1)
        assert ei.value.status == EBVO_ERR_STATE and ei.value.stage == TRACK_STAGE_PROMOTE
        same_quads(got, solo, "the match that was in flight")
        # the keyframe is the old one: its pose, its source, its size, and what a match reads of it
        tl.same_keyframe_pose(C.temporal_keyframe_pose(), kpose, "after the refused promotion")
        raises(EBVO_ERR_STATE, lambda: C.temporal_depth_source())
        assert tl.align_size(C, 0)[0] == n_kf == len(mates[0])
        same_quads(C.temporal_match(slot=1, stages=1), solo, "a match against the keyframe after the refused promotion")
        # its depth state: one alignment and one fusion, nothing more
        current(D, 1)
        a = D.temporal_align_pose(CALIB, *start(1, 0), **AKW)
        D.temporal_refine_depth(CALIB, a["R"], a["t"], align=AKW, **DKW)
        assert_state(C.temporal_depth_fetch(), D.temporal_depth_fetch(), "the depth state after the refused promotion")
        # the same step after the wait: the frame is fused a second time and promoted
        step = C.temporal_track_frame(CALIB, *start(1, 0), **STEP_KW, policy=policy)
        want = explicit_frame(D, 1, 0, mates, policy)
        assert (step["tracked"], step["failed_stage"], step["switched"], step["decision"]) == (1, 0, 1, 1) == (1, 0, 1, want["decision"])
        assert step["reasons"] == want["reasons"]
        tl.same_pose_record(step["pose"], want["pose"], "the repeated step: pose")
        tl.same_depth_record(step["depth"], want["depth"], "the repeated step: depth")
        tl.same_cover_record(step["cover"], want["cover"], "the repeated step: cover")
        assert step["carried"] == want["carried"] and step["carried"]["n_carried"] > 20, (step["carried"], want["carried"])
        assert step["finalized"]["n_final"] == want["carried"]["n_new"]
        state = C.temporal_depth_fetch()
        assert_state(state, D.temporal_depth_fetch(), "the carried state")
        assert state["n_obs"].max() == 2
        assert_bit_equal(C.temporal_depth_source(), D.temporal_depth_source(), "temporal_depth_source")
        tl.same_keyframe_pose(C.temporal_keyframe_pose(), D.temporal_keyframe_pose(), "after the promotion")
        assert_bit_equal(C.temporal_keyframe_pose()[0], step["R_seq"], "the promoted keyframe's pose is the frame's")
        for c in (C, D):
            finalized(c, 3)
        same_quads(C.temporal_match(stages=1), D.temporal_match(stages=1), "the match of frame 3 against the promoted keyframe")
    finally:
        C.close()
        D.close()
