"""Relative pose from the temporal quads on the device (ebvo_pose_from_quads / ebvo_temporal_estimate_pose) against the CPU
restatement of MotionTracker::estimate_Relative_Pose_From_Quad_Pairs (tests/oracle_pose.py), bit for bit: every result field,
the inlier mask, the quad geometry and the rank order.  Quads of a known motion recover it; the resident chain's final quads
give the same bits as the host arrays fetched from it; the batch size of the device search changes no bit."""
import functools

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib, synth
from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EBVO_ERR_STATE, EbvoError
from tests import oracle_pose as op
from tests.pose_scenes import R_GT, T_GT, resident_chain, rig
from tests.util import assert_bit_equal, assert_edges_equal

pytestmark = pytest.mark.gpu

FIELDS = ("status", "found", "n_quads", "top_n", "iterations", "draws", "hypotheses", "best_inliers", "dynamic_max_iter",
          "best_q1", "best_q2")
def assert_same(got, ref, geom=True):
    for k in FIELDS:
        assert got[k] == ref[k], (k, got[k], ref[k])
    assert_bit_equal(got["inlier_ratio"], np.float64(ref["inlier_ratio"]), "inlier_ratio")
    assert_bit_equal(got["R"], ref["R"], "R")
    assert_bit_equal(got["t"], ref["t"], "t")
    assert_bit_equal(got["inlier"], ref["inlier"], "inlier")
    if geom and ref["quad_geom"] is not None:
        assert_bit_equal(got["quad_geom"], ref["quad_geom"], "quad_geom")
        assert_bit_equal(got["rank_order"], ref["rank_order"], "rank_order")


@functools.lru_cache(maxsize=None)
def synthetic(name, n, frac, multi=None):
    calib = rig(name)
    q = op.synthetic_quads(n, frac, (calib[0], calib[2], calib[3]), R_GT, T_GT, seed=n + int(100 * frac),
                           multi=(0.0 if n <= 3 else 0.2) if multi is None else multi)
    return calib, q


@functools.lru_cache(maxsize=None)
def oracle_of(name, n, frac, **kw):
    calib, (kfL, kfR, rp, cfL, cfR, _) = synthetic(name, n, frac)
    return op.estimate_pose(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], **kw)


CASES = [(n, f) for n in (2, 3, 64, 1000, 20000) for f in (0.0, 0.3, 0.6) if n - int(f * n) >= 2]


@pytest.mark.parametrize("name", ["kitti", "euroc"])
@pytest.mark.parametrize("n,frac", CASES)
def test_known_pose_and_oracle_parity(ctx, name, n, frac):
    calib, (kfL, kfR, rp, cfL, cfR, inl) = synthetic(name, n, frac)
    kw = dict(top_rank_fraction=1.0) if n == 2 else {}
    got = ctx.pose_from_quads(kfL, kfR, rp, cfL, cfR, calib, **kw)
    assert_same(got, oracle_of(name, n, frac, **kw))
    assert got["status"] == 0 and got["found"]
    if int(frac * n) and n < 64:
        return  # 2 inliers + 1 outlier: a pair with the outlier explains two quads as well as the true motion does
    assert np.abs(got["R"] - R_GT).max() < 1e-9 and np.abs(got["t"] - T_GT).max() < 1e-9
    assert_bit_equal(got["inlier"], inl, "planted inliers")


@pytest.mark.parametrize("frame", [2, 3])
def test_resident_chain_pose(ctx, frame):
    calib, kfL, kfR, fin, counts = resident_chain(ctx, frame)
    assert counts["n_final"] > 300
    kitti = rig("kitti")
    for cal in (calib, kitti):
        got = ctx.temporal_estimate_pose(cal)
        host = ctx.pose_from_quads(kfL, kfR, fin["row_ptr"], fin["left"], fin["right"], cal)
        ref = op.estimate_pose(kfL, kfR, fin["row_ptr"], fin["left"], fin["right"], cal[0], cal[2], cal[3])
        assert_same(host, ref)
        assert_same(got, ref, geom=False)
        assert got["n_quads"] == counts["n_final"] == len(got["inlier"])
    # the pose calls left the slot's results alone
    _, q2 = ctx._temporal_results(0, _fetch_counts(counts), 1, True)
    f2 = q2["final"]
    for k in ("row_ptr", "cf_index", "ncc_left", "sift_left", "score_left", "score_right", "valid"):
        assert_bit_equal(f2[k], fin[k], k)
    assert_edges_equal(f2["left"], fin["left"], "left")
    assert_edges_equal(f2["right"], fin["right"], "right")
    # the mask holds the best hypothesis' inliers among every final quad
    assert got["found"] and int(got["inlier"].sum()) == got["best_inliers"] >= 2


def _fetch_counts(counts):
    c = _lib.TemporalCounts()
    for k, v in counts.items():
        setattr(c, k, v)
    return c


def test_batch_size_changes_no_bit(ctx):
    calib, (kfL, kfR, rp, cfL, cfR, _) = synthetic("euroc", 1000, 0.3)
    ref = oracle_of("euroc", 1000, 0.3)
    try:
        for v in (1, 7, 64, 4096, 0):
            ctx.debug_set(20, v)
            assert_same(ctx.pose_from_quads(kfL, kfR, rp, cfL, cfR, calib), ref)
        with pytest.raises(EbvoError):
            ctx.debug_set(20, (1 << 20) + 1)
        ctx.debug_set(20, 1 << 20)
        assert_same(ctx.pose_from_quads(kfL, kfR, rp, cfL, cfR, calib, max_iterations=50, min_iterations=10),
                    op.estimate_pose(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], max_iterations=50, min_iterations=10))
    finally:
        ctx.debug_set(20, 0)


@pytest.mark.parametrize("kw", [dict(max_iterations=0), dict(max_iterations=1), dict(max_iterations=10),
                                dict(max_iterations=20, min_iterations=50), dict(min_iterations=0, max_iterations=300),
                                dict(top_rank_fraction=2.5 / 64), dict(top_rank_fraction=1.5 / 64),
                                dict(tau_length=0.0, tau_t1=0.0, tau_t2=0.0, tau_tangent=0.0, max_draws=3000),
                                dict(tau_length=np.inf, tau_t1=np.inf, tau_t2=np.inf, tau_tangent=np.inf, max_draws=77),
                                dict(rand_seed=42), dict(rand_seed=2**31 - 1), dict(rand_seed=0),
                                dict(max_reproj_error=0.0), dict(max_reproj_error=np.inf, max_iterations=30),
                                dict(success_prob=0.5, dyn_num_trials_mult=0.25, min_iterations=5)])
def test_parameter_edges(ctx, kw):
    calib, (kfL, kfR, rp, cfL, cfR, _) = synthetic("kitti", 64, 0.3)
    got = ctx.pose_from_quads(kfL, kfR, rp, cfL, cfR, calib, **kw)
    ref = op.estimate_pose(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], **kw)
    assert_same(got, ref)
    if kw.get("tau_length") == 0.0:
        assert got["status"] == 2 and got["draws"] == 3000 and not got["found"] and got["hypotheses"] == 0
    if kw.get("max_draws") == 77:
        assert got["status"] == 2 and got["draws"] == 77
    if kw == dict(top_rank_fraction=1.5 / 64):
        assert got["top_n"] == 1 and got["status"] == 1 and (got["R"] == np.eye(3)).all()
    if kw == dict(top_rank_fraction=2.5 / 64):
        assert got["top_n"] == 2 and got["status"] == 0


@pytest.mark.parametrize("n,frac,branch", [(200, 0.0, "high"), (200, 0.3, "mid"), (1000, 0.97, "low")])
def test_dynamic_max_iter_branches(ctx, n, frac, branch):
    calib, (kfL, kfR, rp, cfL, cfR, _) = synthetic("euroc", n, frac, multi=0.0)
    kw = dict(max_iterations=400, min_iterations=100)
    got = ctx.pose_from_quads(kfL, kfR, rp, cfL, cfR, calib, **kw)
    ref = op.estimate_pose(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], **kw)
    assert_same(got, ref)
    r = got["inlier_ratio"]
    if branch == "high":
        assert r >= 0.95 and got["dynamic_max_iter"] == 100 and got["iterations"] == 101
    elif branch == "low":
        assert 0 < r <= 0.05 and got["dynamic_max_iter"] == 400 and got["iterations"] == 400
    else:
        assert 0.05 < r < 0.95 and got["dynamic_max_iter"] not in (100, 400)


@pytest.mark.parametrize("n", [0, 1])
def test_too_few_quads(ctx, n):
    calib, (kfL, kfR, rp, cfL, cfR, _) = synthetic("kitti", 3, 0.0)
    rp = np.array([0, n], dtype=np.int32)
    got = ctx.pose_from_quads(kfL[:1], kfR[:1], rp, cfL[:n], cfR[:n], calib)
    assert got["status"] == 1 and not got["found"] and got["draws"] == 0 and got["n_quads"] == n
    assert (got["R"] == np.eye(3)).all() and (got["t"] == 0).all() and (got["inlier"] == 0).all()
    got = ctx.pose_from_quads(kfL[:0], kfR[:0], np.zeros(1, dtype=np.int32), cfL[:0], cfR[:0], calib)
    assert got["status"] == 1 and got["n_quads"] == 0


def test_resident_slot_without_quads(ctx):
    """ebvo_temporal_estimate_pose on a slot whose chain kept no quad: a current frame without edges, then a keyframe without
    mates.  Insufficient, identity, an empty mask, nothing launched."""
    h, w = 96, 160
    F = synth.fundamental_for("kitti")
    calib = rig("kitti")
    l, r = synth.stereo_pair("s2", h, w)
    flat = np.full((h, w), 128, dtype=np.uint8)
    for kf_img, cf_img in (((l, r), (flat, flat)), ((flat, flat), (l, r))):
        ctx.stereo_upload(*kf_img)
        ctx.stereo_run(ctx.default_params(F))
        ctx.stereo_finalize(None)
        ctx.temporal_set_keyframe()
        ctx.stereo_upload(*cf_img)
        ctx.stereo_run(ctx.default_params(F))
        ctx.stereo_finalize(None)
        counts, _ = ctx.temporal_match(stages=1)
        assert counts["n_final"] == 0
        got = ctx.temporal_estimate_pose(calib)
        assert got["status"] == 1 and not got["found"] and got["n_quads"] == 0 and got["draws"] == 0
        assert (got["R"] == np.eye(3)).all() and (got["t"] == 0).all() and len(got["inlier"]) == 0


def test_continue_stream(ctx):
    calib, (kfL, kfR, rp, cfL, cfR, _) = synthetic("kitti", 64, 0.3)
    args = (kfL, kfR, rp, cfL, cfR)
    kw = dict(max_iterations=40, min_iterations=5, rand_seed=7)
    a = ctx.pose_from_quads(*args, calib, **kw)
    b = ctx.pose_from_quads(*args, calib, continue_stream=1, **kw)
    ra = op.estimate_pose(*args, calib[0], calib[2], calib[3], **kw)
    rb = op.estimate_pose(*args, calib[0], calib[2], calib[3], rng=ra["rng"], **kw)
    assert_same(a, ra)
    assert_same(b, rb)
    # a fresh stream again
    assert_same(ctx.pose_from_quads(*args, calib, **kw), ra)


BAD = [dict(success_prob=0.0), dict(success_prob=1.0), dict(success_prob=np.nan), dict(top_rank_fraction=0.0),
       dict(top_rank_fraction=1.0000001), dict(top_rank_fraction=np.nan), dict(max_reproj_error=-1e-300),
       dict(max_reproj_error=np.nan), dict(tau_length=-0.1), dict(tau_t1=np.nan), dict(tau_t2=-np.inf), dict(tau_tangent=-1.0),
       dict(max_iterations=-1), dict(min_iterations=-1), dict(max_draws=0), dict(max_draws=-5), dict(dyn_num_trials_mult=0.0),
       dict(dyn_num_trials_mult=-1.0), dict(dyn_num_trials_mult=np.nan)]


def test_refused_calls_leave_the_slot_alone(ctx):
    calib, kfL, kfR, fin, counts = resident_chain(ctx, 2)
    ref = ctx.temporal_estimate_pose(calib)
    for kw in BAD:
        for call in (lambda: ctx.temporal_estimate_pose(calib, **kw),
                     lambda: ctx.pose_from_quads(kfL, kfR, fin["row_ptr"], fin["left"], fin["right"], calib, **kw)):
            with pytest.raises(EbvoError) as ei:
                call()
            assert ei.value.status == EBVO_ERR_ARG, kw
    bad_cal = (calib[0], calib[1], np.full(9, np.nan), calib[3])
    with pytest.raises(EbvoError) as ei:
        ctx.temporal_estimate_pose(bad_cal)
    assert ei.value.status == EBVO_ERR_ARG
    with pytest.raises(EbvoError) as ei:
        ctx.temporal_estimate_pose(calib, slot=99)
    assert ei.value.status == EBVO_ERR_ARG
    _, q2 = ctx._temporal_results(0, _fetch_counts(counts), 1, True)
    for k in ("row_ptr", "cf_index", "score_left", "valid"):
        assert_bit_equal(q2["final"][k], fin[k], k)
    assert_same(ctx.temporal_estimate_pose(calib), ref, geom=False)


def test_state_errors(ctx):
    calib = rig("kitti")
    F = synth.fundamental_for("kitti")
    l, r = synth.stereo_pair("s2", 96, 160)
    ctx.stereo_upload(l, r)
    ctx.stereo_run(ctx.default_params(F))
    ctx.stereo_finalize(None)
    with pytest.raises(EbvoError) as ei:                 # no quads at all on the new pair
        ctx.temporal_estimate_pose(calib)
    assert ei.value.status == EBVO_ERR_STATE
    ctx.temporal_set_keyframe()
    ctx.temporal_match(stages=0)                         # stages = 0: no final quads
    with pytest.raises(EbvoError) as ei:
        ctx.temporal_estimate_pose(calib)
    assert ei.value.status == EBVO_ERR_STATE
    ctx.temporal_match(stages=1)
    got = ctx.temporal_estimate_pose(calib)              # a frame against itself
    assert got["status"] in (0, 2) and got["n_quads"] > 2
    ctx.temporal_set_keyframe()                          # the quads belong to the previous keyframe now
    with pytest.raises(EbvoError) as ei:
        ctx.temporal_estimate_pose(calib)
    assert ei.value.status == EBVO_ERR_STATE
