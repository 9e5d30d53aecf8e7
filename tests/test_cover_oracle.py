"""Properties of the keyframe coverage, the switch policy and the pose bookkeeping shown without a device: the header still is
ABI 6 and declares the stage; every parity case of tests/cover_cases.py meets the condition it was built for; the oracle's
own invariants; the policy of the loaded library at every threshold, its precedence and its defaults against the oracle's
table; the study of DESIGN 8.6 on the twelve noisy scenes along eight frames."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import cover_cases as cc
from tests import cover_study as cst
from tests import depth_scenes as ds
from tests import oracle_cover as ocv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ebvo_cover_default_params", "ebvo_keyframe_cover_edges", "ebvo_temporal_keyframe_cover", "ebvo_temporal_cover_size",
               "ebvo_keyframe_policy_default", "ebvo_keyframe_decide", "ebvo_temporal_keyframe_pose", "ebvo_track_default_params",
               "ebvo_temporal_track_frame")
CASES = cc.cases()


def test_header_is_abi_6_and_declares_the_stage():
    from edge_based_visual_odometry_amd import _lib
    src = open(os.path.join(ROOT, "include", "ebvo_hip.h")).read()
    assert int(re.search(r"#define EBVO_ABI_VERSION (\d+)", src).group(1)) == 6
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.load_library()
    for name in NEW_SYMBOLS:
        assert re.search(rf"\b{name}\s*\(", code), name
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name), name
    for struct in ("ebvo_cover_params", "ebvo_keyframe_cover", "ebvo_keyframe_policy", "ebvo_track_params", "ebvo_tracked_frame"):
        assert re.search(rf"\}}\s*{struct};", code), struct
    for name, v in (("EBVO_COVER_DEAD", ocv.DEAD), ("EBVO_COVER_IN_FRAME", ocv.IN_FRAME), ("EBVO_COVER_ASSOCIATED", ocv.ASSOCIATED),
                    ("EBVO_COVER_INLIER", ocv.INLIER), ("EBVO_KF_LOST", ocv.LOST), ("EBVO_KF_LOW_OVERLAP", ocv.LOW_OVERLAP),
                    ("EBVO_KF_LOW_ASSOC", ocv.LOW_ASSOC), ("EBVO_KF_NEW_CONTENT", ocv.NEW_CONTENT), ("EBVO_KF_PARALLAX", ocv.PARALLAX)):
        assert re.search(rf"#define {name} {v}u", code), name
    assert lib.ebvo_abi_version() == 6


def test_defaults_are_the_headers():
    from edge_based_visual_odometry_amd import _lib
    lib = _lib.load_library()
    p = _lib.CoverParams()
    lib.ebvo_cover_default_params(ctypes.byref(p))
    assert {k: getattr(p, k) for k in ocv.DEFAULTS} == ocv.DEFAULTS and p.reserved == 0 and p.pad == 0
    q = _lib.KeyframePolicy()
    lib.ebvo_keyframe_policy_default(ctypes.byref(q))
    assert {k: getattr(q, k) for k in ocv.POLICY} == ocv.POLICY
    assert ctypes.sizeof(_lib.CoverParams) == 64 and ctypes.sizeof(_lib.KeyframeCover) == 4 * (12 + ocv.BINS)
    assert ctypes.sizeof(_lib.KeyframePolicy) == 32
    t = _lib.TrackParams()
    lib.ebvo_track_default_params(ctypes.byref(t))
    assert t.refine_depth == 1 and t.reserved == 0 and t.cover.cover_cell == 32 and t.policy.max_disp_bins == 30
    assert t.align.rounds == 4 and t.depth.iterations == 3 and t.carry.radius == 1.5 and t.finalize.bnb_ratio > 0


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_meets_its_condition(name):
    case = CASES[name]()
    r = cc.run_oracle(case)
    assert case["check"](r), (name, case["note"], {k: r[k] for k in ocv.INT_FIELDS}, r["assoc"][:16], r["flags"][:16])
    assert (case["img_w"], case["img_h"]) == (200, 120)
    n, n0 = len(case["kf_left"]), len(case["edges_left"])
    assert r["n_kf"] == n and r["n_edges"] == n0
    assert all(len(r[k]) == n for k in ("flags", "assoc", "disp")) and len(r["explained"]) == n0
    assert len(r["cell_edges"]) == len(r["cell_explained"]) == r["cw"] * r["ch"]
    # the oracle's own invariants
    fl = r["flags"]
    dead, inf, has, inl = ((fl & b) != 0 for b in (ocv.DEAD, ocv.IN_FRAME, ocv.ASSOCIATED, ocv.INLIER))
    assert (r["n_dead"], r["n_in_frame"], r["n_assoc"], r["n_inliers"]) == tuple(int(v.sum()) for v in (dead, inf, has, inl))
    assert all(fl[dead] == ocv.DEAD) and not (has & ~inf).any() and not (inl & ~has).any()
    assert ((r["assoc"] >= 0) == has).all() and (np.isnan(r["disp"]) == ~inf).all() and (r["disp"][inf] >= 0).all()
    assert int(r["hist"].sum()) == r["n_in_frame"]
    assert r["n_explained"] == int(r["explained"].sum()) == len(set(r["assoc"][has].tolist())) <= r["n_assoc"]
    assert (r["cell_explained"] <= r["cell_edges"]).all() and int(r["cell_edges"].sum()) <= n0
    assert 0 <= r["n_cells_covered"] <= r["n_cells_cur"] <= r["cw"] * r["ch"]
    if r["n_in_frame"]:
        b = r["disp_median_bin"]
        assert 2 * int(r["hist"][:b + 1].sum()) >= r["n_in_frame"] > 2 * int(r["hist"][:b].sum())
    else:
        assert r["disp_median_bin"] == -1


def test_the_cases_cover_what_they_name():
    names = set(CASES)
    assert {f"n_kf_{n}" for n in (1, 63, 64, 65, 1024, 1025)} <= names and {f"n0_{n}" for n in (1, 64, 65)} <= names
    assert {"all_dead", "out_of_frame", "nothing_associated", "shared_edge", "nan_edge", "lambda_given", "lambda_null", "cover_cell_32",
            "cover_cell_7", "cover_cell_500", "min_cell_edges_at", "min_cell_edges_above", "min_cell_explained_at",
            "min_cell_explained_above", "bin_edge_on", "bin_edge_below", "bin_saturated", "inlier_at", "inlier_below", "kitti_all",
            "euroc_all"} <= names
    assert set(cc.PICKED) <= names and "n_kf_1025" in cc.PICKED
    loc = np.array(cc.lattice(1025))
    assert loc[:, 0].max() < 190 and loc[:, 1].max() < 110


def test_lambda_changes_an_association():
    with_l, without = cc.run_oracle(CASES["lambda_given"]()), cc.run_oracle(CASES["lambda_null"]())
    differ = int((with_l["assoc"] != without["assoc"]).sum())
    print(f"associations that differ between Gamma / lambda and Gamma: {differ} of {with_l['n_kf']}")
    assert differ >= 1


# ---- the policy, through the loaded library --------------------------------------------------------------------------------
BASE = dict(n_kf=1000, n_dead=100, n_in_frame=800, n_assoc=600, n_inliers=500, n_edges=3000, n_explained=550, cw=7, ch=4, n_cells_cur=20,
            n_cells_covered=15, disp_median_bin=10)


def lib_decide(cover, **policy):
    from edge_based_visual_odometry_amd import _lib
    lib = _lib.load_library()
    c, p, reasons = _lib.KeyframeCover(), _lib.KeyframePolicy(), ctypes.c_uint32(0xFFFFFFFF)
    lib.ebvo_keyframe_policy_default(ctypes.byref(p))
    for k, v in policy.items():
        setattr(p, k, v)
    for k, v in cover.items():
        setattr(c, k, v)
    d = lib.ebvo_keyframe_decide(ctypes.byref(c), ctypes.byref(p), ctypes.byref(reasons))
    assert (d, reasons.value) == ocv.decide(cover, **policy), (cover, policy)
    return d, reasons.value


def test_policy_keeps_the_base_record():
    assert lib_decide(BASE) == (0, 0)


@pytest.mark.parametrize("reason,at,off", [
    (ocv.LOST, dict(n_assoc=50, n_in_frame=60, n_kf=60, n_dead=0), dict(n_assoc=49, n_in_frame=60, n_kf=60, n_dead=0)),
    (ocv.LOW_OVERLAP, dict(n_in_frame=630, n_assoc=600), dict(n_in_frame=629, n_assoc=600)),                 # 0.7 * 900 = 630
    (ocv.LOW_ASSOC, dict(n_assoc=400), dict(n_assoc=399)),                                                    # 0.5 * 800 = 400
    (ocv.NEW_CONTENT, dict(n_cells_covered=12), dict(n_cells_covered=11)),                                    # 0.6 * 20 = 12
    (ocv.PARALLAX, dict(disp_median_bin=29), dict(disp_median_bin=30)),
])
def test_policy_reason_at_its_threshold_and_one_step_off(reason, at, off):
    """`at`: the count exactly on the threshold (strict <: the reason is not set; PARALLAX is >=: one bin below); `off`: one
    step across it"""
    d, r = lib_decide(dict(BASE, **at))
    assert not r & reason and (d, r) == (0, 0)
    d, r = lib_decide(dict(BASE, **off))
    assert r == reason and d == (2 if reason == ocv.LOST else 1)


def test_policy_share_products_are_formed_in_double():
    """0.55 * 100 rounds to 55.00000000000001 in double: 55 of 100 in frame IS below it, and 0.7 * 90 rounds to 62.99999999999999:
    63 of 90 is NOT below it and neither is -- just -- 62.99999999999999 < 63; the contract's expression, not exact arithmetic"""
    assert 0.55 * 100.0 > 55.0 and 0.7 * 90.0 < 63.0
    c = dict(BASE, n_kf=100, n_dead=0, n_in_frame=55, n_assoc=55)
    assert lib_decide(c, min_assoc=1, min_in_frame_share=0.55) == (1, ocv.LOW_OVERLAP)
    assert lib_decide(dict(c, n_in_frame=56, n_assoc=56), min_assoc=1, min_in_frame_share=0.55) == (0, 0)
    c = dict(BASE, n_kf=90, n_dead=0, n_in_frame=63, n_assoc=63)
    assert lib_decide(c, min_assoc=1) == (0, 0)
    assert lib_decide(dict(c, n_in_frame=62, n_assoc=62), min_assoc=1) == (1, ocv.LOW_OVERLAP)


def test_policy_precedence_lost_over_switch_over_keep():
    every = dict(BASE, n_in_frame=100, n_assoc=10, n_cells_covered=0, disp_median_bin=63)
    d, r = lib_decide(every)
    assert r == ocv.LOST | ocv.LOW_OVERLAP | ocv.LOW_ASSOC | ocv.NEW_CONTENT | ocv.PARALLAX and d == 2
    assert lib_decide(dict(BASE, disp_median_bin=40)) == (1, ocv.PARALLAX)
    assert lib_decide(dict(BASE, disp_median_bin=-1)) == (0, 0)
    empty = dict.fromkeys(BASE, 0)
    assert lib_decide(dict(empty, disp_median_bin=-1)) == (2, ocv.LOST)
    assert lib_decide(dict(empty, disp_median_bin=-1), min_assoc=0) == (0, 0)


def test_policy_refuses_null_and_accepts_null_reasons():
    from edge_based_visual_odometry_amd import _lib
    lib = _lib.load_library()
    c, p = _lib.KeyframeCover(), _lib.KeyframePolicy()
    lib.ebvo_keyframe_policy_default(ctypes.byref(p))
    assert lib.ebvo_keyframe_decide(None, ctypes.byref(p), None) == _lib.EBVO_ERR_ARG
    assert lib.ebvo_keyframe_decide(ctypes.byref(c), None, None) == _lib.EBVO_ERR_ARG
    assert lib.ebvo_keyframe_decide(ctypes.byref(c), ctypes.byref(p), None) == 2


def test_compose_is_the_written_out_product():
    """the numpy restatement of Rk <- R Rk, tk <- mv3(R, tk) + t agrees with the matrix product to rounding and is exact on
    the identity"""
    rng = np.random.default_rng(3)
    R, Rk = (ocv.oa.op.rot(rng.normal(size=3), a) for a in (0.3, -0.7))
    t, tk = rng.normal(size=3), rng.normal(size=3)
    Ro, to = ocv.compose(R, t, Rk, tk)
    assert np.abs(Ro - R @ Rk).max() < 4e-16 and np.abs(to - (R @ tk + t)).max() < 1e-15
    Ri, ti = ocv.compose(R, t, np.eye(3), np.zeros(3))
    assert Ri.tobytes() == np.ascontiguousarray(R).tobytes() and ti.tobytes() == t.tobytes()


# ---- the study of DESIGN 8.6 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(ds.NOISY)))
def test_study_along_the_trajectory(k):
    """what the oracle shows on ALL twelve scenes: the default policy keeps the keyframe at frame 1; the in-frame share at frame
    8 is strictly below the one at frame 1; the median displacement bin never decreases with the frame index.  The covered
    share of the cells is NOT monotone (DESIGN 8.6 reports the rows) and is not asserted.  The shares under the perturbed pose
    are printed beside the planted ones: DESIGN 8.6 records how far they move."""
    rows = cst.rows(k)
    for f, (a, b) in enumerate(rows, 1):
        print(f"scene {k} {ds.NOISY[k]} frame {f}: planted in-frame {a[0]:.4f} assoc {a[1]:.4f} explained {a[2]:.4f} cells {a[3]:.4f} bin {a[4]} "
              f"decision {a[5]} | perturbed {b[0]:.4f} {b[1]:.4f} {b[2]:.4f} {b[3]:.4f} {b[4]} {b[5]}")
    planted = [a for a, _ in rows]
    assert planted[0][5] == 0
    assert planted[-1][0] < planted[0][0]
    bins = [a[4] for a in planted]
    assert all(y >= x for x, y in zip(bins, bins[1:])) and bins[0] >= 0
