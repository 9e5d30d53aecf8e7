"""Properties of the inverse-depth filter shown on its CPU restatement (tests/oracle_depth.py), without a device: the header
still is ABI 6 and declares the stage; every parity case meets the condition it was built for; a fixed point on noise-free
scenes; recovery of planted disparity noise over four frames on every scene class; the pose errors of the alignment with and
without the refined depths, recorded (DESIGN 8.4 says why nothing is asserted about their order)."""
import os
import re

import numpy as np
import pytest

from tests import align_scenes as asc
from tests import depth_cases as dc
from tests import depth_scenes as ds
from tests import oracle_align as oa
from tests import oracle_depth as od
from tests.util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ebvo_depth_default_params", "ebvo_depth_refine_edges", "ebvo_temporal_refine_depth", "ebvo_temporal_depth_fetch",
               "ebvo_temporal_depth_reset", "ebvo_temporal_use_depth", "ebvo_pose_align_edges_depth")
CASES = dc.cases()


def test_header_is_abi_6_and_declares_the_stage():
    from edge_based_visual_odometry_amd import _lib
    src = open(os.path.join(ROOT, "include", "ebvo_hip.h")).read()
    assert int(re.search(r"#define EBVO_ABI_VERSION (\d+)", src).group(1)) == 6
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name), name
    for struct in ("ebvo_depth_params", "ebvo_depth_refined"):
        assert re.search(rf"\}}\s*{struct};", code), struct
    assert lib.ebvo_abi_version() == 6


def test_defaults_are_the_headers():
    import ctypes

    from edge_based_visual_odometry_amd import _lib
    p = _lib.DepthParams()
    _lib.load_library().ebvo_depth_default_params(ctypes.byref(p))
    assert {k: getattr(p, k) for k in od.DEFAULTS} == od.DEFAULTS and p.block_threads == 0 and p.reserved == 0


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_meets_its_condition(name):
    case = CASES[name]()
    r = dc.run_oracle(case)
    assert case["check"](r), (name, case["note"])
    n = len(case["kf_left"])
    assert r["n_kf"] == n == r["n_dead"] + r["n_updated"] + r["n_restored"]
    assert all(len(r[k]) == n for k in ("lambda_", "info", "n_obs", "flags"))
    live = (r["flags"] & od.DEAD) == 0
    assert np.isfinite(r["lambda_"][live]).all() and (r["info"][live] > 0).all()


def test_lambda_one_changes_no_bit_of_the_alignment():
    case = dc.ac.cases()["n_kf_1025"]()
    args = (case["edges_left"], case["edges_right"], case["img_w"], case["img_h"], case["calib"], case["R0"], case["t0"])
    plain = oa.align(case["kf_left"], case["kf_right"], *args, **case["params"])
    ones = od.align(case["kf_left"], case["kf_right"], np.ones(len(case["kf_left"])), *args, **case["params"])
    for k in ("R", "t", "assoc_left", "assoc_right"):
        assert_bit_equal(ones[k], plain[k], k)
    assert ones["cost_last"] == plain["cost_last"] and ones["steps_kept"] == plain["steps_kept"] > 0
    assert oa.Scene.__name__ == "Scene" and oa.ot.project.__name__ == "project"      # the oracle put back what it borrowed


@pytest.mark.parametrize("rig,seed", ds.FIXED_POINT)
def test_fixed_point(rig, seed):
    """noise-free scene, planted poses, noise-free depth: lambda stays at 1 within 10 x the measured worst case (the residue is
    the arcs' sagitta between two samples 0.5 px apart, not rounding)"""
    sc = ds.scene(rig, seed)
    assert np.abs(sc["lambda_true"] - 1.0).max() == 0.0
    states = ds.fuse(sc)
    worst = max(float(np.abs(s[0] - 1.0).max()) for s in states)
    print(f"fixed point {rig} {seed}: max |lambda - 1| = {worst!r}, updated {states[-1][3]['n_updated']} of {len(sc['kf_left'])}")
    assert worst <= 10.0 * dc.FIXED_POINT_MEASURED
    assert states[-1][3]["n_updated"] > 0.95 * len(sc["kf_left"]) and states[-1][2].max() == ds.FRAMES


def pose_error(R, t, Rg, tg):
    """(rotation angle in degrees, |t - t_gt|)"""
    E = Rg.T @ R
    return float(np.degrees(np.arccos(np.clip((np.trace(E) - 1.0) / 2.0, -1.0, 1.0)))), float(np.linalg.norm(t - tg))


@pytest.mark.parametrize("rig,seed,kind,sigma,clutter", ds.NOISY)
def test_recovery_of_planted_disparity_noise(rig, seed, kind, sigma, clutter):
    """N(0, 0.25 px) on the keyframe's disparities, frames 1 .. 4 fused at their planted poses: the median |lambda - lambda*|
    ends below the median |1 - lambda*| the keyframe started with.  The feedback into the alignment is recorded only."""
    sc = ds.scene(rig, seed, kind, sigma, clutter, sigma_disp=ds.SIGMA_DISP)
    truth = sc["lambda_true"]
    states = ds.fuse(sc)
    start = float(np.median(np.abs(1.0 - truth)))
    meds = [float(np.median(np.abs(s[0] - truth))) for s in states]
    print(f"recovery {rig} {seed} {kind} {sigma} {clutter}: median |1 - l*| {start:.5f}; after 1 .. {ds.FRAMES} frames " +
          " ".join(f"{m:.5f}" for m in meds))
    assert meds[-1] < start
    assert states[-1][3]["n_updated"] > 0.9 * len(truth)
    # feedback: frame 1 aligned from the perturbed start of the alignment's own study, on Gamma and on Gamma / lambda
    (R1, t1), (E0, E1) = sc["poses"][0], sc["frames"][0]
    R0, t0 = asc.perturbed(R1, t1)
    args = (E0, E1, ds.W, ds.H, sc["calib"], R0, t0)
    off = oa.align(sc["kf_left"], sc["kf_right"], *args)
    on = od.align(sc["kf_left"], sc["kf_right"], states[-1][0], *args)
    e_off, e_on = pose_error(off["R"], off["t"], R1, t1), pose_error(on["R"], on["t"], R1, t1)
    print(f"feedback {rig} {seed} {kind} {sigma} {clutter}: without {e_off[0]:.4f} deg {e_off[1]:.5f} m, with {e_on[0]:.4f} deg {e_on[1]:.5f} m")
    assert off["status"] == 0 and on["status"] == 0
