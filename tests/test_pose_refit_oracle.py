"""The refit's CPU restatement (tests/oracle_pose_refit.py) on its own: the deterministic sums against a straight loop, the
noisy and noise-free scenes of tests/pose_refit_scenes.py against the planted motion, and the host pose-error metric.  No GPU."""
import functools
import math
import os
import subprocess

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib, api
from tests import oracle_pose as op
from tests import oracle_pose_refit as orf
from tests import pose_refit_scenes as sc
from tests.pose_scenes import R_GT, T_GT


def straight_sums(terms):
    """the contract's sum, written out lane by lane with scalar additions"""
    n, m = terms.shape
    out = []
    for c in range(m):
        lanes = [0.0] * 1024
        for k in range(n):
            lanes[k % 1024] = lanes[k % 1024] + float(terms[k, c])
        groups = []
        for g in range(16):
            x = lanes[64 * g:64 * g + 64]
            s = 32
            while s >= 1:
                for l in range(s):
                    x[l] = x[l] + x[l + s]
                s //= 2
            groups.append(x[0])
        s = 8
        while s >= 1:
            for l in range(s):
                groups[l] = groups[l] + groups[l + s]
            s //= 2
        out.append(groups[0])
    return np.array(out)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_reduction_equals_a_straight_loop(n):
    rng = np.random.default_rng(n)
    terms = rng.normal(size=(n, 3)) * 10.0 ** rng.integers(-8, 8, size=(n, 3))
    got = orf.virtual_lane_sums(terms)
    ref = straight_sums(terms)
    assert got.tobytes() == ref.tobytes()
    # and it is a sum: any order of 2049 additions stays within n ulps of the largest term
    assert np.abs(got - terms.sum(axis=0)).max() <= n * 2.0 ** -52 * np.abs(terms).max() * n


@functools.lru_cache(maxsize=None)
def scene(rig_name, n, frac, sigma, seed):
    """(quads, search result, refit result) of one scene"""
    K, _, R21, T21 = sc.calib(rig_name)
    q = sc.noisy_quads(rig_name, n, frac, sigma, seed)
    search = op.estimate_pose(*q[:5], K, R21, T21, **sc.SEARCH)
    refit = orf.refit(*q[:5], K, R21, T21, search["R"], search["t"])
    return q, search, refit


@pytest.mark.parametrize("seed", sc.SEEDS)
@pytest.mark.parametrize("n,frac,sigma", sc.NOISY)
@pytest.mark.parametrize("rig_name", sc.RIGS)
def test_noisy_scenes_improve(rig_name, n, frac, sigma, seed):
    _, search, refit = scene(rig_name, n, frac, sigma, seed)
    assert search["found"] and refit["status"] == 0
    e0 = api.pose_error(search["R"], search["t"], R_GT, T_GT)
    e1 = api.pose_error(refit["R"], refit["t"], R_GT, T_GT)
    assert e1["rot_deg"] < e0["rot_deg"], (e0, e1)
    assert e1["trans_abs"] < e0["trans_abs"], (e0, e1)
    assert refit["inliers"] >= search["best_inliers"]
    assert refit["cost_last"] <= refit["cost_first"]
    assert refit["inliers"] == int(refit["inlier"].sum()) and refit["n_quads"] == len(refit["inlier"])


@pytest.mark.parametrize("n", [3, 64, 1000])
@pytest.mark.parametrize("rig_name", sc.RIGS)
def test_noise_free_scenes_stay_exact(rig_name, n):
    _, search, refit = scene(rig_name, n, 0.0 if n == 3 else 0.3, 0.0, 0)
    assert search["found"] and refit["status"] == 0
    assert np.abs(refit["R"] - R_GT).max() < 1e-9 and np.abs(refit["t"] - T_GT).max() < 1e-9
    assert refit["stop_reason"] == orf.STOP_EPS
    assert refit["cost_last"] <= refit["cost_first"]


def test_refit_demo_builds_with_plain_gxx_and_agrees_on_pose_error(tmp_path):
    """tests/cpp/refit_demo.cpp against the C ABI alone; without arguments it needs no device: the default refit options and
    ebvo::pose_error on a quarter turn about z with perpendicular translations of lengths 2 and 3"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(_lib.LIB_PATH)
    exe = str(tmp_path / "refit_demo")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"),
                           os.path.join(root, "tests", "cpp", "refit_demo.cpp"), "-o", exe, "-L", libdir, "-lebvo_hip",
                           f"-Wl,-rpath,{libdir}", "-Wl,-rpath,/opt/rocm/lib"])
    lines = subprocess.check_output([exe], text=True).splitlines()
    assert lines[0] == "rounds 2 iterations 10 huber_px 1.5 step_eps 1e-10 block_threads 0"
    got = [float(v) for v in lines[1].split()[1:]]
    Rz = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    ref = api.pose_error(Rz, [0.0, 2.0, 0.0], np.eye(3), [3.0, 0.0, 0.0])
    for g, k in zip(got, ("rot_deg", "trans_abs", "trans_dir_deg")):
        assert g == pytest.approx(ref[k], rel=1e-15, abs=1e-13), k
    assert ref["rot_deg"] == pytest.approx(90.0, abs=1e-13)


def test_pose_error():
    e = api.pose_error(R_GT, T_GT, R_GT, T_GT)
    assert e["rot_deg"] == 0.0 and e["trans_abs"] == 0.0 and e["trans_dir_deg"] == 0.0
    R = op.rot((0.3, 1.0, -0.2), 0.04) @ R_GT
    e = api.pose_error(R, T_GT, R_GT, T_GT)
    # R_gt^T (Q R_gt) is a rotation by the planted angle about the turned axis
    assert abs(math.radians(e["rot_deg"]) - 0.04) < 1e-12
    e = api.pose_error(R_GT, np.zeros(3), R_GT, T_GT)
    assert math.isnan(e["trans_dir_deg"]) and e["trans_abs"] == pytest.approx(float(np.linalg.norm(T_GT)), abs=1e-15)
    assert math.isnan(api.pose_error(R_GT, T_GT, R_GT, np.zeros(3))["trans_dir_deg"])
    t = np.array([0.0, 2.0, 0.0])
    e = api.pose_error(np.eye(3), t, np.eye(3), np.array([3.0, 0.0, 0.0]))
    assert e["trans_dir_deg"] == pytest.approx(90.0, abs=1e-12) and e["trans_abs"] == pytest.approx(math.sqrt(13.0), abs=1e-15)
    # the independent statement in the oracle agrees
    ref = orf.pose_error(R, t, R_GT, T_GT)
    got = api.pose_error(R, t, R_GT, T_GT)
    for k in ref:
        assert got[k] == pytest.approx(ref[k], rel=1e-12, abs=1e-12), k
