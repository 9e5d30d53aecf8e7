"""The pose stage under ground truth without a device: the literal restatement (tests/oracle_pose_gt.py: skip rows, sort, search
or cascade) against a second path through tests/oracle_pose.py (the unfiltered search on the compacted arrays, the combined
constraint test), the properties of the cascade's counts, the refused calls of the four symbols, and the adapter compiling
with plain g++."""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib, api
from tests import oracle_pose as op
from tests import oracle_pose_gt as og
from tests.pose_scenes import R_GT, T_GT, rig
from tests.util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("status", "found", "n_quads", "top_n", "iterations", "draws", "hypotheses", "best_inliers", "dynamic_max_iter",
          "best_q1", "best_q2")


@functools.lru_cache(maxsize=None)
def scene(name, n, frac):
    calib = rig(name)
    q = op.synthetic_quads(n, frac, (calib[0], calib[2], calib[3]), R_GT, T_GT, seed=n + int(100 * frac), multi=0.2)
    return calib, q


def masks(n_kf, which):
    i = np.arange(n_kf)
    if which == "third":                                   # every third row off
        m = (i % 3 != 1).astype(np.uint8)
        return m, None
    listed = (i % 5 != 2).astype(np.uint8)                 # row_listed and kf_is_tp differ
    tp = (i % 7 != 3).astype(np.uint8)
    return listed, tp


@pytest.mark.parametrize("which", ["third", "differ"])
@pytest.mark.parametrize("name", ["kitti", "euroc"])
def test_filtered_search_equals_search_on_compacted_rows(name, which):
    calib, (kfL, kfR, rp, cfL, cfR, _) = scene(name, 1000, 0.3)
    listed, tp = masks(len(kfL), which)
    got = og.estimate_pose_gt(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], row_listed=listed, kf_is_tp=tp)
    on = listed.astype(bool) & (tp.astype(bool) if tp is not None else True)
    ckfL, ckfR, crp, ccfL, ccfR, back = og.compact(kfL, kfR, rp, cfL, cfR, on)
    ref = op.estimate_pose(ckfL, ckfR, crp, ccfL, ccfR, calib[0], calib[2], calib[3])
    assert 2 < ref["n_quads"] < int(rp[-1]) and ref["found"]
    for k in FIELDS:
        assert got[k] == ref[k], k
    for k in ("inlier_ratio", "R", "t"):
        assert_bit_equal(np.asarray(got[k], dtype=np.float64), np.asarray(ref[k], dtype=np.float64), k)
    n = ref["n_quads"]
    assert_bit_equal(got["rank_order"][:n], back[ref["rank_order"]].astype(np.int32), "rank_order mapped back")
    assert (got["rank_order"][n:] == -1).all()
    full = np.zeros(int(rp[-1]), dtype=np.uint8)
    full[back] = ref["inlier"]
    assert_bit_equal(got["inlier"], full, "inlier mapped back")
    geom = np.zeros((int(rp[-1]), 12))
    geom[back] = ref["quad_geom"]
    assert_bit_equal(got["quad_geom"], geom, "quad_geom mapped back")


def test_all_rows_equal_the_unfiltered_search():
    calib, (kfL, kfR, rp, cfL, cfR, _) = scene("euroc", 64, 0.3)
    got = og.estimate_pose_gt(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3])
    ref = op.estimate_pose(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3])
    for k in FIELDS:
        assert got[k] == ref[k], k
    for k in ("R", "t", "inlier", "quad_geom", "rank_order"):
        assert_bit_equal(got[k], ref[k], k)


def test_insufficient_rows():
    calib, (kfL, kfR, rp, cfL, cfR, _) = scene("euroc", 64, 0.3)
    n_kf = len(kfL)
    one = np.zeros(n_kf, dtype=np.uint8)
    one[int(np.argmax(np.diff(rp)))] = 1                    # one listed row, of two quads
    for listed, tp in ((one, None), (np.zeros(n_kf, dtype=np.uint8), None), (None, np.zeros(n_kf, dtype=np.uint8))):
        got = og.estimate_pose_gt(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], row_listed=listed, kf_is_tp=tp)
        assert got["status"] == 1 and not got["found"] and got["draws"] == 0 and (got["R"] == np.eye(3)).all()
        c = og.constraint_metrics(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], row_listed=listed, kf_is_tp=tp, n_runs=2)
        assert [r["status"] for r in c["runs"]] == [1, 1] and c["draw_idx"] is None
    assert og.estimate_pose_gt(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], row_listed=one)["n_quads"] == 2


TIGHT = dict(tau_length=0.02, tau_t1=0.01, tau_t2=0.01, tau_tangent=0.02)


@pytest.mark.parametrize("taus", [{}, TIGHT])
@pytest.mark.parametrize("name,n,frac", [("euroc", 1000, 0.3), ("euroc", 1000, 0.6), ("kitti", 1000, 0.3), ("kitti", 64, 0.3)])
def test_cascade_against_the_combined_constraints(name, n, frac, taus):
    calib, (kfL, kfR, rp, cfL, cfR, inl) = scene(name, n, frac)
    every_third = (np.arange(int(rp[-1])) % 3 == 0).astype(np.uint8)
    c = og.constraint_metrics(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], quad_is_tp=every_third, n_runs=2, **taus)
    p = dict(op.DEFAULTS, **taus)
    tau = (p["tau_length"], p["tau_t1"], p["tau_t2"], p["tau_tangent"])
    geom = op.quad_geometry(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3])
    order = op.rank_order(rp)
    rows = [tuple(r) for r in geom.tolist()]
    for r, run in enumerate(c["runs"]):
        st = run["stages"]
        # the last stage's survivors are the draws the search's combined test accepts
        ok = np.array([op.constraints(rows[order[i1]], rows[order[i2]], tau) for i1, i2 in c["draw_idx"][r].tolist()])
        assert_bit_equal((c["draw_stage"][r] & 7) == 4, ok, "survivors of the last stage")
        assert st[4]["surviving"] == int(ok.sum())
        ver = every_third[order[c["draw_idx"][r][:, 0]]] & every_third[order[c["draw_idx"][r][:, 1]]]
        assert_bit_equal((c["draw_stage"][r] >> 7).astype(np.uint8), ver, "veridical bit")
        counts = [s["surviving"] for s in st]
        assert counts[0] == run["draws"] == 5000 and all(a >= b for a, b in zip(counts, counts[1:]))
        assert all(s["veridical"] <= s["surviving"] for s in st)
        for k in range(5):
            assert st[k]["surviving"] == int(((c["draw_stage"][r] & 7) >= k).sum())
        assert st[0]["recall"] == 1.0 and st[0]["precision"] == st[0]["veridical"] / 5000
        assert 0 < st[4]["recall"] <= 1.0
    if taus and name == "euroc":
        assert all(a > b for a, b in zip(counts, counts[1:]))      # the tight set rejects at every stage
    # the first draw is the first draw the search consumes with the same seed
    inf = dict(tau_length=np.inf, tau_t1=np.inf, tau_t2=np.inf, tau_tangent=np.inf, max_iterations=1)
    first = op.estimate_pose(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], **inf)
    assert first["draws"] == 1 and (first["best_q1"], first["best_q2"]) == tuple(c["draw_idx"][0, 0].tolist())
    # the mean over runs, as Print_Quad_Pairs_Metrics_Statistics forms it
    mean = og.mean_over_runs(c["runs"])
    runs = [api._CascadeRun(r["stages"]) for r in c["runs"]]
    assert api.cascade_mean(runs) == mean
    assert mean[2]["veridical"] == (c["runs"][0]["stages"][2]["veridical"] + c["runs"][1]["stages"][2]["veridical"]) / 2.0


@pytest.mark.parametrize("name,n,frac,want", [("euroc", 1000, 0.3, 3367), ("kitti", 1000, 0.3, 3367), ("euroc", 1000, 0.6, 1078),
                                              ("kitti", 64, 0.3, 3530)])
def test_planted_mask_and_tiny_taus(name, n, frac, want):
    """with the planted inliers as b_is_veridical and taus of 1e-6 only the pairs of two true quads survive"""
    calib, (kfL, kfR, rp, cfL, cfR, inl) = scene(name, n, frac)
    tiny = dict(tau_length=1e-6, tau_t1=1e-6, tau_t2=1e-6, tau_tangent=1e-6)
    c = og.constraint_metrics(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], quad_is_tp=inl, **tiny)
    st = c["runs"][0]["stages"]
    assert st[0]["veridical"] == want and st[0]["surviving"] == 5000
    for s in st[1:]:
        assert s["surviving"] == s["veridical"] == want and s["recall"] == 1.0 and s["precision"] == 1.0


def test_no_veridical_quad_gives_nan_recall():
    calib, (kfL, kfR, rp, cfL, cfR, _) = scene("kitti", 64, 0.3)
    c = og.constraint_metrics(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], max_iterations=65)
    st = c["runs"][0]["stages"]
    assert st[0]["veridical"] == 0 and st[0]["precision"] == 0.0 and st[0]["recall"] == 1.0
    assert all(np.isnan(s["recall"]) and s["precision"] == 0.0 for s in st[1:])
    empty = og.constraint_metrics(kfL, kfR, rp, cfL, cfR, calib[0], calib[2], calib[3], max_iterations=0)["runs"][0]
    assert empty["status"] == 0 and empty["draws"] == 0 and np.isnan(empty["stages"][0]["precision"])


def test_struct_sizes_and_names():
    assert ctypes.sizeof(_lib.PoseCascadeStage) == 40 and ctypes.sizeof(_lib.PoseCascadeRun) == 32 + 5 * 40
    assert _lib.PC_STAGE_NAMES == og.STAGE_NAMES and _lib.PC_NUM_STAGES == 5


def test_null_and_bad_arguments_are_refused():
    lib = _lib.load_library()
    p, r, cal = _lib.PoseParams(), _lib.PoseResult(), _lib.StereoCalib()
    lib.ebvo_pose_default_params(ctypes.byref(p))
    rp = np.zeros(1, dtype=np.int32)
    runs = (_lib.PoseCascadeRun * 1)()
    cp, pp, rr = ctypes.byref(cal), ctypes.byref(p), ctypes.byref(r)
    ARG = _lib.EBVO_ERR_ARG
    assert lib.ebvo_pose_from_quads_gt(None, None, None, 0, _lib.ptr(rp), None, None, None, None, cp, pp, rr, None, None, None) == ARG
    assert lib.ebvo_pose_from_quads_gt(None, None, None, 0, None, None, None, None, None, None, None, None, None, None, None) == ARG
    assert lib.ebvo_temporal_estimate_pose_gt(None, 0, cp, pp, rr, None) == ARG
    assert lib.ebvo_temporal_estimate_pose_gt(None, 0, None, None, None, None) == ARG
    assert lib.ebvo_pose_constraint_metrics(None, None, None, 0, _lib.ptr(rp), None, None, None, None, None, cp, pp, 1, runs, None,
                                            None) == ARG
    assert lib.ebvo_pose_constraint_metrics(None, None, None, 0, None, None, None, None, None, None, None, None, 0, None, None,
                                            None) == ARG
    assert lib.ebvo_temporal_pose_constraint_metrics(None, 0, cp, pp, 1, runs, None, None) == ARG
    assert lib.ebvo_temporal_pose_constraint_metrics(None, 0, cp, pp, 0, None, None, None) == ARG


def test_motion_tracker_gt_adapter_builds_with_plain_gxx(tmp_path):
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "pose_gt_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cpp", "pose_gt_demo.cpp"), "-o", exe, "-L", libdir, "-lebvo_hip",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)
