"""The pose prior without a device: the oracle's figures (tests/tprior_cases.EXPECTED), the two conditions that make the
GPU tests (tests/test_gpu_tprior.py) mean something, liveness on hand-made mates, the host arithmetic of predict_pose and
the library's new entry points."""
import ctypes
import re
from pathlib import Path

import numpy as np

from edge_based_visual_odometry_amd import _lib, api
from tests import oracle_tprior as otp
from tests import tgt_cases
from tests import tprior_cases as cases

NEW_SYMBOLS = ("ebvo_temporal_set_prior", "ebvo_temporal_clear_prior", "ebvo_temporal_prior_fetch", "ebvo_tprior_candidates")


def test_library_exports_the_new_entry_points():
    root = Path(_lib.__file__).parent
    lib = ctypes.CDLL(str(root / "libebvo_hip.so"))
    header = (root.parent / "include" / "ebvo_hip.h").read_text()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in _lib.ABI_SYMBOLS and re.search(rf"\bint {name}\(", header), name
    assert hasattr(lib, "ebvo_tprior_default_params") and re.search(r"\bvoid ebvo_tprior_default_params\(", header)
    assert re.search(r"#define EBVO_ABI_VERSION 6\b", header)       # additive: the version stays
    p = _lib.TpriorParams()
    _lib.load_library().ebvo_tprior_default_params(ctypes.byref(p))
    assert (p.img_margin, p.use_orientation) == (0.0, 1)
    # the refusals that need no device
    assert lib.ebvo_temporal_set_prior(None, 0, None, None, None, None) == _lib.EBVO_ERR_ARG
    assert lib.ebvo_temporal_clear_prior(None, 0) == _lib.EBVO_ERR_ARG
    assert lib.ebvo_temporal_prior_fetch(None, 0, None, None, None, None, None) == _lib.EBVO_ERR_ARG


def test_expected_table_is_the_oracles():
    assert cases.table() == cases.EXPECTED


def test_unprimed_match_finds_nothing_true_and_the_true_prior_recovers_it():
    """the two conditions of the GPU tests, with a wide margin: 0, and 1578 of 1649"""
    e = cases.EXPECTED
    assert cases.true_final(cases.unprimed_reference(1)) == 0 == e["unprimed-r30"]["true_final"]
    ref = cases.reference(60.0, 30.0, 1, 1)
    true = cases.true_final(ref)
    assert true >= 1000 and true >= 0.9 * ref["counts"]["n_final"]
    # a tighter radius cuts the candidate list to well under a half and loses no true quad
    tight = cases.reference(60.0, 8.0, 1, 1)
    assert 2 * tight["counts"]["n_candidates"] < ref["counts"]["n_candidates"] and cases.true_final(tight) == true


def test_identity_prior_is_not_the_unprimed_match():
    """The identity prior does NOT reproduce the unprimed match, and no test may ask for that equality: the projection round
    trip (triangulate, project, map the orientation) moves coordinates by about 3e-14 px (more for a mate off its epipolar
    line) and orientations with them, which moves an orientation across the threshold somewhere, and the keyframe's 33
    mismatched mates of negative disparity lie behind the cameras and are not live."""
    kfL, kfR = cases.mates(cases.KF)
    un = cases.unprimed_reference(0)
    for use_orientation in (1, 0):
        ref = cases.reference(0.0, 30.0, use_orientation, 0)
        p = ref["prior"]
        live = p["live"] != 0
        shift = np.abs(np.stack([p["proj_left"][live, 0] - kfL["x"][live], p["proj_left"][live, 1] - kfL["y"][live],
                                 p["proj_right"][live, 0] - kfR["x"][live], p["proj_right"][live, 1] - kfR["y"][live]]))
        # most mates come back within rounding (about 3e-14 px); a mate whose right edge lies off its epipolar line does not
        # triangulate onto both edges and comes back up to half a pixel away
        assert 0.0 < np.median(shift[shift > 0]) < 1e-12 and shift.max() < 1.0
        assert not live[kfR["x"] > kfL["x"]].any() and int((~live).sum()) == 33
        assert (p["depth_left"][~live] < 0).all()
        d = np.diff(ref["row_ptr"]) - np.diff(un["row_ptr"])
        if use_orientation:
            assert (d[live] != 0).any()                            # the mapped orientations decide otherwise on live rows, too
        assert ref["counts"]["n_candidates"] != un["counts"]["n_candidates"]
    assert cases.reference(0.0, 30.0, 1, 0)["counts"]["n_candidates"] == cases.EXPECTED["identity-r30-candidates"]


def test_resident_cases_exercise_what_they_name():
    for name, (px, radius, use_orientation) in cases.RESIDENT.items():
        ref = cases.case_reference(name, 1)
        assert ref["counts"]["n_final"] > 1000 and cases.true_final(ref) > 1000, name
        assert 0 < int(ref["prior"]["live"].sum()) < ref["counts"]["n_kf"], name   # live and non-live rows
        assert not np.diff(ref["row_ptr"])[ref["prior"]["live"] == 0].any(), name
    a, b = cases.case_reference("short-r8", 0), cases.case_reference("own-theta", 0)
    assert a["counts"]["n_candidates"] != b["counts"]["n_candidates"]           # the mapped orientations decide somewhere
    # a radius-8 match needs fewer candidate slots than a radius-30 one keeps headroom for: the capacity test's redo
    big, small = cases.case_reference("true-r30", 0)["counts"]["n_candidates"], a["counts"]["n_candidates"]
    assert big > small + small // 4 + 1024


def test_predict_pose():
    def rot(axis, a):
        c, s = np.cos(a), np.sin(a)
        return {"z": np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]), "x": np.array([[1.0, 0, 0], [0, c, -s], [0, s, c]])}[axis]

    # one earlier pose: the pose itself
    R1, t1 = rot("z", 0.1), np.array([0.3, -0.1, 0.05])
    R, t = api.predict_pose((R1, t1))
    assert (R == R1).all() and (t == t1).all()
    R, t = api.predict_pose((R1, t1), None)
    assert (R == R1).all() and (t == t1).all()
    # hand-composed: the step D = (rot x 0.2, d) takes T1 to T2 = D T1; the prediction is D T2
    D_R, D_t = rot("x", 0.2), np.array([0.05, 0.0, -0.02])
    R2, t2 = D_R @ R1, D_R @ t1 + D_t
    R3, t3 = D_R @ R2, D_R @ t2 + D_t
    R, t = api.predict_pose((R2, t2), (R1, t1))
    assert np.abs(R - R3).max() < 1e-14 and np.abs(t - t3).max() < 1e-14
    # pure translation at constant velocity: 1, 2 -> 3
    R, t = api.predict_pose((np.eye(3), [2.0, 0, 0]), (np.eye(3), [1.0, 0, 0]))
    assert (R == np.eye(3)).all() and (t == [3.0, 0, 0]).all()
    # flat inputs are accepted
    R, t = api.predict_pose((R2.reshape(9), t2), (R1.reshape(9), t1))
    assert np.abs(R - R3).max() < 1e-14


def test_liveness_edge_cases():
    """the border scenes of tests/tgt_cases.py under the identity pose, plus a mate behind the cameras and a NaN mate"""
    for which in cases.BORDER_SCENES:
        s = cases.border_scene(which)
        base = tgt_cases.border_scene(which)
        n = len(base["kf"][0])
        for margin in (0.0, 10.0):
            p = otp.project(s["kfL"], s["kfR"], tgt_cases.B_R, tgt_cases.B_T, tgt_cases.B_CALIB, tgt_cases.B_W, tgt_cases.B_H, margin)
            # the added mates are never live; the first projects onto its own pixel, inside the image: only its depth says no
            assert not p["live"][s["behind"]] and not p["live"][s["nan"]]
            assert p["depth_left"][s["behind"]] < 0 and p["depth_right"][s["behind"]] < 0
            assert abs(p["proj_left"][s["behind"], 0] - 100.0) < 1e-9 and abs(p["proj_left"][s["behind"], 1] - 60.0) < 1e-9
            assert np.isnan(p["proj_left"][s["nan"]]).any()
            # the scene's own mates lie in front of the cameras: live is the in-image test of the ground truth
            tgt = tgt_cases.ot.project(*base["kf"], tgt_cases.B_R, tgt_cases.B_T, tgt_cases.B_CALIB, tgt_cases.B_W, tgt_cases.B_H,
                                       None, margin)
            assert (p["live"][:n] == tgt["in_image"]).all() and (p["depth_left"][:n] > 0).all()
    # at the default margin of 0 every mate of `margin` is live; at the ground truth's 10 px the straddling ones are not
    s = cases.border_scene("margin")
    n = len(tgt_cases.border_scene("margin")["kf"][0])
    live0 = cases.host_reference("border-margin")["live"][:n]
    live10 = cases.host_reference("border-margin", 10.0)["live"][:n]
    assert live0.all() and 0 < live10.sum() < n
    # non-live rows are empty, live rows hold the mates next to the projection
    for which in cases.BORDER_SCENES:
        r = cases.host_reference("border-" + which)
        cnt = np.diff(r["row_ptr"])
        assert not cnt[r["live"] == 0].any() and cnt[r["live"] != 0].all(), which
    # `orient`: the mapped orientation is the mate's own here, so use_orientation changes no row
    a, b = cases.host_reference("border-orient"), cases.host_reference("border-orient", 0.0, 0)
    assert (a["row_ptr"] == b["row_ptr"]).all() and 0 < a["row_ptr"][-1] < 3 * 17


def test_host_scenes_sit_on_the_walks_work_units():
    n = {name: len(cases.host_case(name)["kfL"]) for name in cases.HOST_SCENES}
    assert sorted(set(n.values())) == [1, 3, 63, 64, 65, 257]
    for name in cases.HOST_SCENES:
        r = cases.host_reference(name)
        assert r["live"].any() and r["row_ptr"][-1] > 0, name
    assert not cases.host_reference("kf63")["live"].all()                      # a mate that leaves the image under the pose
