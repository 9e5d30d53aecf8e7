"""The inlier refit of the relative pose on the device (ebvo_pose_refine_from_quads, ebvo_temporal_refine_pose) against its CPU
restatement tests/oracle_pose_refit.py: every field of ebvo_pose_refined and the mask, bit for bit.  The sizes straddle the
64-lane groups and the 1024 virtual lanes; the start pose is the planted motion turned and moved a little, so that no test
depends on the search."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib, synth
from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EBVO_ERR_STATE, EbvoError
from tests import oracle_pose as op
from tests import oracle_pose_refit as orf
from tests import oracle_tgt as ot
from tests import pose_refit_scenes as sc
from tests import temporal_cases as tc
from tests import tgt_cases as cases
from tests.pose_scenes import R_GT, T_GT, resident_chain
from tests.test_gpu_pose import assert_same
from tests.test_gpu_temporal_edges import CALIB, load, new_context
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT_FIELDS = ("status", "stop_reason", "rounds_run", "steps_kept", "n_quads", "fit_quads", "inliers")
R_NEAR = op.rot((1.0, -2.0, 0.5), 3e-4) @ R_GT          # about a quarter of a pixel off at these focal lengths
T_NEAR = T_GT + np.array([0.002, -0.001, 0.003])
SIZES = (3, 63, 64, 65, 1023, 1024, 1025, 2049, 20000)


@pytest.fixture(scope="module")
def rctx():
    """a context of these tests' own (the refit does not depend on the detector mode)"""
    c = new_context("hybrid")
    yield c
    c.close()


def assert_refined(got, ref, what=""):
    for k in INT_FIELDS:
        assert got[k] == ref[k], (what, k, got[k], ref[k])
    for k in ("cost_first", "cost_last"):
        assert_bit_equal(np.float64(got[k]), np.float64(ref[k]), f"{what} {k}")
    assert_bit_equal(got["R"], ref["R"], f"{what} R")
    assert_bit_equal(got["t"], ref["t"], f"{what} t")
    assert_bit_equal(got["inlier"], ref["inlier"], f"{what} inlier")


@functools.lru_cache(maxsize=None)
def quads(rig_name, n, frac, sigma):
    return sc.noisy_quads(rig_name, n, frac, sigma, 0)[:5]


def both(c, rig_name, q, R0, t0, **kw):
    """(device, oracle) on the same quads"""
    cal = sc.calib(rig_name)
    got = c.pose_refine_from_quads(*q, cal, R0, t0, **kw)
    ref = orf.refit(*q, cal[0], cal[2], cal[3], R0, t0, **kw)
    return got, ref


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("rig_name", sc.RIGS)
def test_bit_parity_with_the_oracle(rctx, rig_name, n):
    reasons = set()
    for frac in (0.0, 0.3, 0.6):
        for sigma in (0.0, 0.3):
            q = quads(rig_name, n, frac, sigma)
            got, ref = both(rctx, rig_name, q, R_NEAR, T_NEAR)
            assert_refined(got, ref, f"{rig_name} {n} {frac} {sigma}")
            assert got["n_quads"] == n
            reasons.add((got["status"], got["stop_reason"]))
            if n >= 63:
                assert got["status"] == 0 and got["fit_quads"] >= 3 and got["steps_kept"] >= 1
    assert reasons   # which branches a size reaches is the oracle's business; that they are reached is pinned below


@pytest.mark.parametrize("rig_name", sc.RIGS)
def test_a_chunk_of_outliers_leaves_lanes_without_a_second_term(rctx, rig_name):
    kfL, kfR, rp, cfL, cfR = (a.copy() for a in quads(rig_name, 2049, 0.0, 0.3))
    for e in (cfL, cfR):                                    # CSR [1024, 2048): every quad 40 px off, none in the fit set
        e["x"][1024:2048] += 40.0
    got, ref = both(rctx, rig_name, (kfL, kfR, rp, cfL, cfR), R_NEAR, T_NEAR)
    assert_refined(got, ref, rig_name)
    assert got["status"] == 0 and not got["inlier"][1024:2048].any() and got["inlier"][:1024].sum() > 600


@pytest.mark.parametrize("rig_name", sc.RIGS)
def test_launch_geometry_changes_no_bit(rctx, rig_name):
    q = quads(rig_name, 2049, 0.3, 0.3)
    cal = sc.calib(rig_name)
    ref = orf.refit(*q, cal[0], cal[2], cal[3], R_NEAR, T_NEAR)
    for bt in (0, 256, 512, 1024):
        assert_refined(rctx.pose_refine_from_quads(*q, cal, R_NEAR, T_NEAR, block_threads=bt), ref, f"{rig_name} block {bt}")
    # the row masks select through the search's compaction: a masked call equals the oracle on the same masks
    n_kf = len(q[0])
    listed = (np.arange(n_kf) % 3 != 0).astype(np.uint8)
    tp = (np.arange(n_kf) % 5 != 1).astype(np.uint8)
    for bt in (0, 256):
        got = rctx.pose_refine_from_quads(*q, cal, R_NEAR, T_NEAR, row_listed=listed, kf_is_tp=tp, block_threads=bt)
        want = orf.refit(*q, cal[0], cal[2], cal[3], R_NEAR, T_NEAR, row_listed=listed, kf_is_tp=tp)
        assert_refined(got, want, f"{rig_name} masks block {bt}")
        assert 2 <= got["n_quads"] < 2049 and got["status"] == 0


def shared_gamma(rig_name, n, seed):
    """n quads in ONE row: every quad has the keyframe mate's Gamma, the normal matrix has rank 3"""
    kfL, kfR, _, cfL, cfR = quads(rig_name, n, 0.0, 0.0) if seed == 0 else sc.noisy_quads(rig_name, n, 0.0, 0.0, seed)[:5]
    rng = np.random.default_rng(seed)
    cl, cr = np.repeat(cfL[:1], n), np.repeat(cfR[:1], n)
    for e in (cl, cr):
        e["x"] += rng.normal(0, 0.2, n)
        e["y"] += rng.normal(0, 0.2, n)
    return kfL[:1].copy(), kfR[:1].copy(), np.array([0, n], dtype=np.int32), cl, cr


R_FAR = op.rot((0.2, 1.0, 0.1), math.radians(20.0)) @ R_GT
BRANCHES = [
    # (what, rig, quads, start pose, parameters, (status, stop_reason) the oracle reaches)
    ("one quad: nothing launched", "euroc", lambda: sc.noisy_quads("euroc", 1, 0.0, 0.0, 0)[:5], (R_NEAR, T_NEAR), {}, (1, 4)),
    ("two quads", "kitti", lambda: sc.noisy_quads("kitti", 2, 0.0, 0.0, 0)[:5], (R_NEAR, T_NEAR), {}, (1, 4)),
    ("no inliers under the start pose", "kitti", lambda: quads("kitti", 300, 0.3, 0.3), (np.eye(3), np.zeros(3)), {}, (1, 4)),
    ("one inlier under the start pose", "euroc", lambda: quads("euroc", 300, 0.3, 0.3), (np.eye(3), np.zeros(3)), {}, (1, 4)),
    ("iterations 0", "kitti", lambda: quads("kitti", 300, 0.3, 0.3), (R_NEAR, T_NEAR), dict(iterations=0), (0, 1)),
    ("iterations 1", "euroc", lambda: quads("euroc", 300, 0.3, 0.3), (R_NEAR, T_NEAR), dict(iterations=1), (0, 1)),
    ("20 degrees off, every quad fitted", "kitti", lambda: quads("kitti", 300, 0.3, 0.3), (R_FAR, T_NEAR),
     dict(max_reproj_error=math.inf), (0, 2)),
    ("20 degrees off, every quad fitted", "euroc", lambda: quads("euroc", 300, 0.3, 0.3), (R_FAR, T_NEAR),
     dict(max_reproj_error=math.inf), (0, 2)),
    ("one Gamma: first pivot fails", "kitti", lambda: shared_gamma("kitti", 40, 0), (R_GT, T_GT), {}, (2, 3)),
    ("one Gamma: first pivot fails", "euroc", lambda: shared_gamma("euroc", 5, 1), (R_GT, T_GT), {}, (2, 3)),
    ("one Gamma: a later pivot fails", "kitti", lambda: shared_gamma("kitti", 8, 0), (R_GT, T_GT), {}, (0, 3)),
    ("least squares", "euroc", lambda: quads("euroc", 300, 0.3, 0.3), (R_NEAR, T_NEAR), dict(huber_px=math.inf), (0, 0)),
    ("step_eps 0", "kitti", lambda: quads("kitti", 300, 0.3, 0.3), (R_NEAR, T_NEAR), dict(step_eps=0.0), (0, 2)),
    ("16 rounds", "kitti", lambda: quads("kitti", 300, 0.3, 0.3), (R_NEAR, T_NEAR), dict(rounds=16), (0, 0)),
    ("16 rounds", "euroc", lambda: quads("euroc", 300, 0.3, 0.3), (R_NEAR, T_NEAR), dict(rounds=16), (0, 2)),
]


@pytest.mark.parametrize("what,rig_name,make,start,kw,reached", BRANCHES, ids=[f"{b[0]} ({b[1]})" for b in BRANCHES])
def test_every_status_and_stop_reason(rctx, what, rig_name, make, start, kw, reached):
    got, ref = both(rctx, rig_name, make(), *start, **kw)
    assert (ref["status"], ref["stop_reason"]) == reached, (what, ref["status"], ref["stop_reason"])
    assert_refined(got, ref, what)
    if got["status"]:                                       # 1 and 2 return the start pose
        assert_bit_equal(got["R"], np.asarray(start[0], dtype=np.float64), "start R")
        assert_bit_equal(got["t"], np.asarray(start[1], dtype=np.float64), "start t")
    if "rounds" in kw:
        assert got["rounds_run"] == kw["rounds"]


def _final_unchanged(c, counts, fin, what):
    from tests.test_gpu_pose import _fetch_counts
    _, q2 = c._temporal_results(0, _fetch_counts(counts), 1, True)
    for k in ("row_ptr", "cf_index", "ncc_left", "sift_left", "score_left", "score_right", "valid"):
        assert_bit_equal(q2["final"][k], fin[k], f"{what}: {k}")


def test_resident_form_equals_the_host_form(rctx):
    c = rctx
    calib, kfL, kfR, fin, counts = resident_chain(c, 2)
    assert counts["n_final"] > 300
    args = (kfL, kfR, fin["row_ptr"], fin["left"], fin["right"])
    start = c.temporal_estimate_pose(calib, rand_seed=7)
    follow = c.temporal_estimate_pose(calib, continue_stream=1)
    assert start["found"]
    # the same two searches with the refit between them: it draws nothing from the context's generator
    again = c.temporal_estimate_pose(calib, rand_seed=7)
    got = c.temporal_refine_pose(calib, start["R"], start["t"])
    assert_same(c.temporal_estimate_pose(calib, continue_stream=1), follow, geom=False)
    assert_same(again, start, geom=False)
    host = c.pose_refine_from_quads(*args, calib, start["R"], start["t"])
    ref = orf.refit(*args, calib[0], calib[2], calib[3], start["R"], start["t"])
    assert_refined(host, ref, "host")
    assert_refined(got, ref, "resident")
    assert got["n_quads"] == counts["n_final"] == len(got["inlier"]) and got["status"] == 0
    assert got["inliers"] == int(got["inlier"].sum())
    _final_unchanged(c, counts, fin, "after the refit")


def test_resident_form_over_ground_truth_rows(rctx):
    from tests.test_gpu_pose_gt import assert_snapshot_unchanged, snapshot
    c = rctx
    kf, cf, _ = cases.RESIDENT["small"]
    load(c, kf)
    c.temporal_set_keyframe()
    load(c, cf)
    counts, q = c.temporal_match(stages=1)
    fin = q["final"]
    kfL, kfR = tc.oracle_mates(kf)
    args = (kfL, kfR, fin["row_ptr"], fin["left"], fin["right"])
    with pytest.raises(EbvoError) as ei:                    # gt_rows on a slot that is not armed
        c.temporal_refine_pose(CALIB, np.eye(3), np.zeros(3), gt_rows=True)
    assert ei.value.status == EBVO_ERR_STATE
    r = cases.resident_reference("small", 1, False)
    c.temporal_set_gt(r["R"], r["t"], r["calib"])
    before = snapshot(c, counts, CALIB)
    f = c.temporal_gt_fetch()
    listed = (np.diff(f["ver_row_ptr"]) > 0).astype(np.uint8)
    on = ot.row_on(f["ver_row_ptr"], None)
    start = c.temporal_estimate_pose_gt(CALIB)
    assert start["found"]
    got = c.temporal_refine_pose(CALIB, start["R"], start["t"], gt_rows=True)
    host = c.pose_refine_from_quads(*args, CALIB, start["R"], start["t"], row_listed=listed, kf_is_tp=on)
    ref = orf.refit(*args, CALIB[0], CALIB[2], CALIB[3], start["R"], start["t"], row_listed=listed, kf_is_tp=on)
    assert_refined(host, ref, "host, masks")
    assert_refined(got, ref, "resident, gt rows")
    assert 2 <= got["n_quads"] < counts["n_final"] == len(got["inlier"])
    # every quad of the armed slot: gt_rows = 0 does not read the armed state
    allq = c.temporal_refine_pose(CALIB, start["R"], start["t"])
    assert_refined(allq, orf.refit(*args, CALIB[0], CALIB[2], CALIB[3], start["R"], start["t"]), "resident, every quad")
    assert allq["n_quads"] == counts["n_final"]
    assert_snapshot_unchanged(c, counts, CALIB, before, "after the refits")


BAD = [dict(rounds=0), dict(rounds=17), dict(iterations=-1), dict(iterations=101), dict(huber_px=0.0), dict(huber_px=-1.0),
       dict(huber_px=np.nan), dict(step_eps=-1e-12), dict(step_eps=np.nan), dict(block_threads=128), dict(block_threads=64),
       dict(block_threads=2048), dict(max_reproj_error=-1.0), dict(max_reproj_error=np.nan)]


def test_refused_calls_leave_the_slot_alone(rctx):
    c = rctx
    calib, kfL, kfR, fin, counts = resident_chain(c, 2)
    args = (kfL, kfR, fin["row_ptr"], fin["left"], fin["right"])
    start = c.temporal_estimate_pose(calib)
    ok = c.temporal_refine_pose(calib, start["R"], start["t"])
    R, t = start["R"], start["t"]
    Rn, ti = R.copy(), t.copy()
    Rn[1, 2] = np.nan
    ti[0] = np.inf
    calls = [(dict(kw), R, t, 0) for kw in BAD] + [({}, Rn, t, 0), ({}, R, ti, 0), ({}, R, t, 99), ({}, R, t, -1)]
    for kw, R0, t0, slot in calls:
        resident = lambda: c.temporal_refine_pose(calib, R0, t0, slot=slot, **kw)
        host = lambda: c.pose_refine_from_quads(*args, calib, R0, t0, **kw)
        for call in (resident,) if slot else (resident, host):
            with pytest.raises(EbvoError) as ei:
                call()
            assert ei.value.status == EBVO_ERR_ARG, (kw, slot)
    bad_cal = (calib[0], calib[1], np.full(9, np.nan), calib[3])
    with pytest.raises(EbvoError) as ei:
        c.temporal_refine_pose(bad_cal, R, t)
    assert ei.value.status == EBVO_ERR_ARG
    with pytest.raises(EbvoError) as ei:                    # a CSR that decreases
        rp = fin["row_ptr"].copy()
        rp[1] = rp[-1]
        assert rp[2] < rp[1]
        c.pose_refine_from_quads(kfL, kfR, rp, fin["left"], fin["right"], calib, R, t)
    assert ei.value.status == EBVO_ERR_ARG
    _final_unchanged(c, counts, fin, "after the refused calls")
    assert_refined(c.temporal_refine_pose(calib, R, t), ok, "after the refused calls")
    assert_same(c.temporal_estimate_pose(calib), start, geom=False)


def test_adapter_returns_the_bits_of_the_python_call(tmp_path):
    """MotionTrackerHIP::refine_Relative_Pose (tests/cpp/refit_demo.cpp) on the temporal quads of a frame against itself moved
    by two pixels: the search's pose, every field of the refit and the mask equal those of the Python binding."""
    from edge_based_visual_odometry_amd.api import Context
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "refit_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "refit_demo.cpp"), "-o", exe, "-L", libdir, "-lebvo_hip",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    h, w = 96, 160
    l, r = synth.stereo_pair("s2", h, w)
    (tmp_path / "l.raw").write_bytes(l.tobytes())
    (tmp_path / "r.raw").write_bytes(r.tobytes())
    out = tmp_path / "out.bin"
    subprocess.check_call([exe, str(tmp_path / "l.raw"), str(tmp_path / "r.raw"), str(h), str(w), str(out)])
    buf = out.read_bytes()
    n = int(np.frombuffer(buf, dtype=np.int64, count=1)[0])
    off = 8
    pose = _lib.PoseResult.from_buffer_copy(buf, off); off += C_SIZE(_lib.PoseResult)
    refined = _lib.PoseRefined.from_buffer_copy(buf, off); off += C_SIZE(_lib.PoseRefined)
    mask = np.frombuffer(buf, dtype=np.uint8, count=n, offset=off); off += n
    assert off == len(buf)
    f, t = 718.856, 0.54
    F = np.array([0, 0, 0, 0, 0, -t / f, 0, t / f, 0], dtype=np.float64)
    K = [f, 0, 607.1928, 0, f, 185.2157, 0, 0, 1]
    calib = (K, K, np.eye(3).ravel(), [t, 0, 0])
    with Context(h, w) as c:
        c.stereo_upload(l, r)
        c.stereo_run(c.default_params(F))
        c.stereo_finalize(calib, use_sift=True)
        c.temporal_set_keyframe()
        c.stereo_upload(np.roll(l, 2, axis=1), np.roll(r, 2, axis=1))
        c.stereo_run(c.default_params(F))
        c.stereo_finalize(calib, use_sift=True)
        counts, _ = c.temporal_match(stages=1)
        start = c.temporal_estimate_pose(calib)
        want = c.temporal_refine_pose(calib, start["R"], start["t"])
    assert n == counts["n_final"] > 50
    assert_bit_equal(np.array(pose.R[:]).reshape(3, 3), start["R"], "search R")
    assert_bit_equal(np.array(pose.t[:]), start["t"], "search t")
    assert_refined(c._refined_dict(refined, mask), want, "adapter")


def C_SIZE(struct):
    import ctypes
    return ctypes.sizeof(struct)
