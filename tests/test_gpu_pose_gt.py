"""The pose stage under ground truth on the device (ebvo_pose_from_quads_gt, ebvo_temporal_estimate_pose_gt,
ebvo_pose_constraint_metrics, ebvo_temporal_pose_constraint_metrics) against the CPU restatement (tests/oracle_pose_gt.py),
bit for bit: every integer, every double (NaN included), draw_idx, draw_stage, the inlier mask, the geometry and the rank
order.

Host arrays: the synthetic scenes of tests/test_gpu_pose.py on both rigs.  The default taus reject almost nothing on them, so
every cascade case also runs a tighter set that loses draws at each of the four stages on the euroc scenes (on kitti the last
stage rejects none: both rigs are kept).  max_iterations covers the wave and block edges of pose_cascade_kernel (63 / 64 / 65,
257) and the empty run.
Resident: tests/tgt_cases.py RESIDENT armed as tests/test_gpu_tgt.py arms it; the resident calls give the bits of the
host-array calls fed with what the slot returns, and both equal the restatement."""
import numpy as np
import pytest

from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EBVO_ERR_STATE, EbvoError
from tests import oracle_pose as op
from tests import oracle_pose_gt as og
from tests import oracle_tgt as ot
from tests import temporal_cases as tc
from tests import tgt_cases as cases
from tests.test_gpu_pose import assert_same, synthetic
from tests.test_gpu_temporal_edges import CALIB, load, match, new_context, same_results
from tests.test_gpu_tgt import _counts_struct, device_keyframe_gt
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu

TIGHT = dict(tau_length=0.02, tau_t1=0.01, tau_t2=0.01, tau_tangent=0.02)
SCENES = [(2, 0.0), (3, 0.0), (64, 0.3), (1000, 0.3), (1000, 0.6)]
MAX_ITS = (0, 1, 63, 64, 65, 257, 5000)


@pytest.fixture(scope="module")
def gctx():
    """a context of these tests' own, sized for the full EuRoC frame, with three slots (the pose stage does not depend on the
    detector mode, so these tests do not run once per mode of the session context)"""
    c = new_context("hybrid")
    yield c
    c.close()


def assert_cascade(got, ref, what=""):
    runs, idx, stage = got
    assert len(runs) == len(ref["runs"]), what
    for k, (g, r) in enumerate(zip(runs, ref["runs"])):
        for key in ("status", "n_quads", "top_n", "draws"):
            assert getattr(g, key) == r[key], (what, k, key, getattr(g, key), r[key])
        assert len(g) == len(r["stages"]) == 5
        for gs, rs in zip(g, r["stages"]):
            for key in ("name", "stage", "surviving", "veridical"):
                assert gs[key] == rs[key], (what, k, rs["name"], key, gs[key], rs[key])
            for key in ("recall", "precision"):
                assert_bit_equal(np.array([gs[key]]), np.array([rs[key]], dtype=np.float64), f"{what} run {k} {rs['name']} {key}")
    if ref["draw_idx"] is None:                                # insufficient quads: both arrays untouched
        assert not idx.any() and not stage.any(), what
    else:
        assert_bit_equal(idx, ref["draw_idx"], f"{what}: draw_idx")
        assert_bit_equal(stage, ref["draw_stage"], f"{what}: draw_stage")


def quad_flags(which, inl):
    if which == "planted":
        return inl
    if which == "third":
        return (np.arange(len(inl)) % 3 == 0).astype(np.uint8)
    return None


# --- the cascade on host arrays -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kitti", "euroc"])
@pytest.mark.parametrize("n,frac", SCENES)
def test_cascade_equals_oracle(gctx, name, n, frac):
    calib, (kfL, kfR, rp, cfL, cfR, inl) = synthetic(name, n, frac)
    args = (kfL, kfR, rp, cfL, cfR)
    top = dict(top_rank_fraction=1.0) if n == 2 else {}
    lost = set()
    for taus in ({}, TIGHT):
        for which in ("planted", None, "third"):
            tp = quad_flags(which, inl)
            for max_it in MAX_ITS:
                for n_runs in (1, 3):
                    kw = dict(max_iterations=max_it, **taus, **top)
                    got = gctx.pose_constraint_metrics(*args, calib, quad_is_tp=tp, n_runs=n_runs, details=True, **kw)
                    ref = og.constraint_metrics(*args, calib[0], calib[2], calib[3], quad_is_tp=tp, n_runs=n_runs, **kw)
                    assert_cascade(got, ref, f"{name} {n} {frac} {taus} {which} {max_it} x {n_runs}")
                    assert got[0][0].status == 0
                    if taus and max_it == 5000:
                        s = [g["surviving"] for g in got[0][0]]
                        lost |= {k for k in range(1, 5) if s[k] < s[k - 1]}
    if n == 1000 and name == "euroc":
        assert lost == {1, 2, 3, 4}                            # the tight set exercises every rejection branch


def test_cascade_at_the_reference_run_count(gctx):
    calib, (kfL, kfR, rp, cfL, cfR, inl) = synthetic("euroc", 1000, 0.3)
    args = (kfL, kfR, rp, cfL, cfR)
    got = gctx.pose_constraint_metrics(*args, calib, quad_is_tp=inl, n_runs=20, details=True, **TIGHT)
    ref = og.constraint_metrics(*args, calib[0], calib[2], calib[3], quad_is_tp=inl, n_runs=20, **TIGHT)
    assert_cascade(got, ref, "20 x 5000")
    assert [g["surviving"] for g in got[0][0]] == [5000, 4398, 3940, 3729, 3722]
    from edge_based_visual_odometry_amd.api import cascade_mean
    assert cascade_mean(got[0]) == og.mean_over_runs(ref["runs"])


def test_cascade_with_row_masks(gctx):
    calib, (kfL, kfR, rp, cfL, cfR, inl) = synthetic("euroc", 1000, 0.3)
    args = (kfL, kfR, rp, cfL, cfR)
    i = np.arange(len(kfL))
    listed, tp = (i % 5 != 2).astype(np.uint8), (i % 7 != 3).astype(np.uint8)
    for masks in (dict(row_listed=(i % 3 != 1).astype(np.uint8)), dict(row_listed=listed, kf_is_tp=tp), dict(kf_is_tp=tp)):
        got = gctx.pose_constraint_metrics(*args, calib, quad_is_tp=inl, n_runs=3, details=True, max_iterations=257, **masks, **TIGHT)
        ref = og.constraint_metrics(*args, calib[0], calib[2], calib[3], quad_is_tp=inl, n_runs=3, max_iterations=257, **masks, **TIGHT)
        assert_cascade(got, ref, str(list(masks)))
        assert 2 < got[0][0].n_quads < int(rp[-1])


def test_duplicated_quad_fails_the_length_constraint(gctx):
    """a row copied: the pair of the two copies has zero length on both sides, 0 / 0 is NaN and the comparison is false"""
    calib, (kfL, kfR, rp, cfL, cfR, inl) = synthetic("kitti", 3, 0.0)
    kfL, kfR = np.concatenate([kfL, kfL[:1]]), np.concatenate([kfR, kfR[:1]])
    cfL, cfR = np.concatenate([cfL, cfL[:1]]), np.concatenate([cfR, cfR[:1]])
    rp = np.arange(5, dtype=np.int32)
    tp = np.ones(4, dtype=np.uint8)
    kw = dict(max_iterations=257, top_rank_fraction=1.0)
    got = gctx.pose_constraint_metrics(kfL, kfR, rp, cfL, cfR, calib, quad_is_tp=tp, n_runs=3, details=True, **kw)
    ref = og.constraint_metrics(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], quad_is_tp=tp, n_runs=3, **kw)
    assert_cascade(got, ref, "duplicated quad")
    idx, stage = got[1].reshape(-1, 2), got[2].reshape(-1)
    twins = np.sort(idx, axis=1).tolist()
    dup = np.array([t == [0, 3] for t in twins])
    assert dup.sum() > 20 and ((stage[dup] & 7) == 0).all() and ((stage[~dup] & 7) == 4).all()
    # the search rejects those draws as well
    assert_same(gctx.pose_from_quads_gt(kfL, kfR, rp, cfL, cfR, calib, top_rank_fraction=1.0, max_iterations=50, min_iterations=10),
                og.estimate_pose_gt(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], top_rank_fraction=1.0, max_iterations=50,
                                    min_iterations=10))


# --- the GT-row search on host arrays -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["kitti", "euroc"])
@pytest.mark.parametrize("n,frac", SCENES)
def test_search_over_gt_rows_equals_oracle(gctx, name, n, frac):
    calib, (kfL, kfR, rp, cfL, cfR, inl) = synthetic(name, n, frac)
    args = (kfL, kfR, rp, cfL, cfR)
    kw = dict(top_rank_fraction=1.0) if n == 2 else {}
    n_kf, i = len(kfL), np.arange(len(kfL))
    # all on: the unfiltered search, bit for bit, rank_order included
    plain = gctx.pose_from_quads(*args, calib, **kw)
    for masks in ({}, dict(row_listed=np.ones(n_kf, dtype=np.uint8), kf_is_tp=np.ones(n_kf, dtype=np.uint8))):
        got = gctx.pose_from_quads_gt(*args, calib, **masks, **kw)
        assert_same(got, plain)
        assert_same(got, og.estimate_pose_gt(*args, calib[0], calib[2], calib[3], **kw))
    one = np.zeros(n_kf, dtype=np.uint8)
    one[int(np.argmax(np.diff(rp)))] = 1
    single = np.flatnonzero(np.diff(rp) == 1)[:2]
    two = np.zeros(n_kf, dtype=np.uint8)
    two[single] = 1
    cases_ = [(dict(row_listed=(i % 3 != 1).astype(np.uint8)), {}),                       # every third row off
              (dict(row_listed=(i % 5 != 2).astype(np.uint8), kf_is_tp=(i % 7 != 3).astype(np.uint8)), {}),
              (dict(kf_is_tp=(i % 3 != 1).astype(np.uint8)), {}),
              (dict(row_listed=one), dict(top_rank_fraction=1.0)),                        # one listed row: status 1
              (dict(row_listed=two), dict(top_rank_fraction=1.0)),                        # two listed rows of one quad each
              (dict(row_listed=np.ones(n_kf, dtype=np.uint8), kf_is_tp=two), dict(top_rank_fraction=1.0)),
              (dict(row_listed=one, kf_is_tp=np.ones(n_kf, dtype=np.uint8)), {}),
              (dict(row_listed=np.zeros(n_kf, dtype=np.uint8)), {}),                      # all off
              (dict(kf_is_tp=np.zeros(n_kf, dtype=np.uint8)), {})]
    for masks, extra in cases_:
        p = dict(kw, **extra)
        got = gctx.pose_from_quads_gt(*args, calib, **masks, **p)
        ref = og.estimate_pose_gt(*args, calib[0], calib[2], calib[3], **masks, **p)
        assert_same(got, ref)
        if "row_listed" in masks and masks["row_listed"] is one:
            assert got["status"] == 1 and got["draws"] == 0 and (got["R"] == np.eye(3)).all() and not got["inlier"].any()
        if ref["status"] == 1:
            assert not got["quad_geom"].any() and not got["rank_order"].any()        # left untouched
        elif got["n_quads"] < int(rp[-1]):
            assert (got["rank_order"][got["n_quads"]:] == -1).all()
            off = np.ones(int(rp[-1]), dtype=bool)
            off[got["rank_order"][:got["n_quads"]]] = False
            assert not got["inlier"][off].any() and not got["quad_geom"][off].any()
    if n >= 64:
        got = gctx.pose_from_quads_gt(*args, calib, row_listed=two, top_rank_fraction=1.0)
        assert got["status"] == 0 and got["n_quads"] == 2 and got["top_n"] == 2


def test_one_generator_across_cascade_and_search(gctx):
    calib, (kfL, kfR, rp, cfL, cfR, inl) = synthetic("kitti", 64, 0.3)
    args = (kfL, kfR, rp, cfL, cfR)
    cal = (calib[0], calib[2], calib[3])
    ckw = dict(max_iterations=40, rand_seed=7)
    pkw = dict(max_iterations=40, min_iterations=5, rand_seed=7)
    a = gctx.pose_constraint_metrics(*args, calib, quad_is_tp=inl, n_runs=2, details=True, **ckw)
    b = gctx.pose_from_quads(*args, calib, continue_stream=1, **pkw)
    c = gctx.pose_constraint_metrics(*args, calib, quad_is_tp=inl, details=True, continue_stream=1, **ckw)
    d = gctx.pose_from_quads_gt(*args, calib, continue_stream=1, **pkw)
    ra = og.constraint_metrics(*args, *cal, quad_is_tp=inl, n_runs=2, **ckw)
    rb = op.estimate_pose(*args, *cal, rng=ra["rng"], **pkw)
    rc = og.constraint_metrics(*args, *cal, quad_is_tp=inl, rng=rb["rng"], **ckw)
    rd = og.estimate_pose_gt(*args, *cal, rng=rc["rng"], **pkw)
    assert_cascade(a, ra, "first")
    assert_same(b, rb)
    assert_cascade(c, rc, "continued")
    assert_same(d, rd)
    # a fresh stream again
    assert_cascade(gctx.pose_constraint_metrics(*args, calib, quad_is_tp=inl, n_runs=2, details=True, **ckw), ra, "fresh")


def test_profiler_lists_the_cascade_kernel(gctx):
    calib, (kfL, kfR, rp, cfL, cfR, inl) = synthetic("euroc", 64, 0.3)
    gctx.profile_enable(True)
    gctx.profile_reset()
    try:
        gctx.pose_constraint_metrics(kfL, kfR, rp, cfL, cfR, calib, quad_is_tp=inl, n_runs=3, max_iterations=257)
        prof = gctx.profile_get()
    finally:
        gctx.profile_enable(False)
    assert prof["pose_cascade"][1] == 1                        # one launch for every run of the call


# --- resident slot ------------------------------------------------------------------------------------------------------
def snapshot(c, counts, cal):
    _, q = c._temporal_results(0, _counts_struct(counts), 1, True)
    return q, c.temporal_gt_fetch(), c.temporal_gt_metrics(), c.temporal_estimate_pose(cal)


def assert_snapshot_unchanged(c, counts, cal, before, what):
    q, f, m, pose = snapshot(c, counts, cal)
    same_results(before[0], q, what)
    for k in f:
        assert_bit_equal(np.asarray(f[k]), np.asarray(before[1][k]), f"{what}: {k}")
    assert m == before[2], what
    assert_same(pose, dict(before[3], quad_geom=None), geom=False)


@pytest.mark.parametrize("name,variants", [("small", (False, True)), ("euroc-half", (True,))])
def test_resident_slot_equals_host_arrays_and_oracle(gctx, name, variants):
    c = gctx
    kf, cf, _ = cases.RESIDENT[name]
    load(c, kf)
    gamma, is_tp = device_keyframe_gt(c, kf, 0)
    c.temporal_set_keyframe()
    load(c, cf)
    counts, q, _ = match(c, kf, cf, stages=1)
    fin = q["final"]
    kfL, kfR = tc.oracle_mates(kf)
    args = (kfL, kfR, fin["row_ptr"], fin["left"], fin["right"])
    cal = (CALIB[0], CALIB[2], CALIB[3])
    for with_gt in variants:
        r = cases.resident_reference(name, 1, with_gt)
        c.temporal_set_gt(r["R"], r["t"], r["calib"], kf_gamma=gamma if with_gt else None, kf_is_tp=is_tp if with_gt else None)
        before = snapshot(c, counts, CALIB)
        e = cases.EXPECTED[(name, with_gt)]
        f = c.temporal_gt_fetch()
        listed = (np.diff(f["ver_row_ptr"]) > 0).astype(np.uint8)
        on = ot.row_on(f["ver_row_ptr"], is_tp if with_gt else None)
        assert (int(listed.sum()), int(on.sum())) == (e["n_rows"], e["n_on"])      # both masks matter with GT
        flags = c.temporal_gt_flags(ot.CLUSTER, counts["n_final"])
        what = f"{name} gt {with_gt}"
        # the search
        got = c.temporal_estimate_pose_gt(CALIB)
        host = c.pose_from_quads_gt(*args, CALIB, row_listed=listed, kf_is_tp=on)
        ref = og.estimate_pose_gt(*args, *cal, row_listed=listed, kf_is_tp=on)
        assert_same(host, ref)
        assert_same(got, ref, geom=False)
        assert got["status"] == 0 and 2 <= got["n_quads"] < counts["n_final"] == len(got["inlier"])
        # the cascade
        for kw in (dict(n_runs=3, max_iterations=257, **TIGHT), dict(n_runs=1)):
            got = c.temporal_pose_constraint_metrics(CALIB, details=True, **kw)
            host = c.pose_constraint_metrics(*args, CALIB, row_listed=listed, kf_is_tp=on, quad_is_tp=flags, details=True, **kw)
            ref = og.constraint_metrics(*args, *cal, row_listed=listed, kf_is_tp=on, quad_is_tp=flags, **kw)
            assert_cascade(host, ref, f"{what} host {kw}")
            assert_cascade(got, ref, f"{what} resident {kw}")
            assert got[0][0].status == 0 and got[0][0][0]["veridical"] > 0
        assert_snapshot_unchanged(c, counts, CALIB, before, what)


def test_state_and_refusals(gctx):
    c = gctx
    load(c, "small0")
    c.temporal_set_keyframe()
    load(c, "small2")
    counts, q, _ = match(c, "small0", "small2", stages=1)
    r = cases.resident_reference("small", 1, False)
    R, t, cal = r["R"], r["t"], r["calib"]
    calls = (lambda **kw: c.temporal_estimate_pose_gt(CALIB, **kw), lambda **kw: c.temporal_pose_constraint_metrics(CALIB, **kw))

    def refused(status, **kw):
        for call in calls:
            with pytest.raises(EbvoError) as ei:
                call(**kw)
            assert ei.value.status == status, kw

    refused(EBVO_ERR_STATE)                                    # not armed
    c.temporal_set_gt(R, t, cal)
    before = snapshot(c, counts, CALIB)
    ok = c.temporal_estimate_pose_gt(CALIB)
    assert ok["status"] == 0
    # arguments: the ranges of the search, n_runs and the draw cap; the armed slot stays as it was
    for kw in (dict(tau_length=np.nan), dict(tau_t1=np.nan), dict(tau_t2=np.nan), dict(tau_tangent=np.nan), dict(tau_t1=-1.0),
               dict(top_rank_fraction=0.0), dict(max_iterations=-1), dict(success_prob=1.0)):
        refused(EBVO_ERR_ARG, **kw)
    kfL, kfR = tc.oracle_mates("small0")
    fin = q["final"]
    host = lambda **kw: c.pose_constraint_metrics(kfL, kfR, fin["row_ptr"], fin["left"], fin["right"], CALIB, **kw)
    for kw in (dict(n_runs=0), dict(n_runs=-1), dict(n_runs=(1 << 24) // 5000 + 1), dict(n_runs=2, max_iterations=(1 << 23) + 1),
               dict(tau_length=np.nan)):
        for call in (calls[1], host):
            with pytest.raises(EbvoError) as ei:
                call(**kw)
            assert ei.value.status == EBVO_ERR_ARG, kw
    with pytest.raises(EbvoError) as ei:
        c.pose_from_quads_gt(kfL, kfR, fin["row_ptr"], fin["left"], fin["right"], CALIB, tau_tangent=np.nan)
    assert ei.value.status == EBVO_ERR_ARG
    assert len(c.temporal_pose_constraint_metrics(CALIB, n_runs=(1 << 24) // 5000)) == (1 << 24) // 5000   # the cap itself
    refused(EBVO_ERR_ARG, slot=99)
    assert_snapshot_unchanged(c, counts, CALIB, before, "after refusals")
    assert_same(c.temporal_estimate_pose_gt(CALIB), ok, geom=False)
    # work in flight on the slot: the resident and the host-array calls are refused, nothing is touched
    c.temporal_match_submit(stages=1)
    refused(EBVO_ERR_STATE)
    for call in (host, lambda: c.pose_from_quads_gt(kfL, kfR, fin["row_ptr"], fin["left"], fin["right"], CALIB)):
        with pytest.raises(EbvoError) as ei:
            call()
        assert ei.value.status == EBVO_ERR_STATE
    c.temporal_match_wait()
    refused(EBVO_ERR_STATE)                                    # a new match disarms
    # armed after stages = 0: no final quads
    match(c, "small0", "small2", stages=0)
    c.temporal_set_gt(R, t, cal)
    refused(EBVO_ERR_STATE)
    # the keyframe replaced since the match
    match(c, "small0", "small2", stages=1)
    c.temporal_set_gt(R, t, cal)
    assert c.temporal_estimate_pose_gt(CALIB)["status"] == 0
    load(c, "small0", slot=1)
    c.temporal_set_keyframe(slot=1)
    refused(EBVO_ERR_STATE)
