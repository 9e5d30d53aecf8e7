"""Properties of the handover of the depths on promotion shown on its CPU restatement (tests/oracle_carry.py), without a
device: the header still is ABI 6 and declares the stage; every parity case meets the condition it was built for; the
oracle's own invariants; a fixed point on noise-free scenes; recovery of planted disparity noise on the new keyframe's mates on
every scene class, with the share of mates it rests on."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import carry_cases as cc
from tests import carry_scenes as cs
from tests import oracle_carry as oc
from tests.util import assert_bit_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ebvo_depth_carry_default_params", "ebvo_depth_carry", "ebvo_temporal_promote_keyframe", "ebvo_temporal_depth_source")
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
    for struct in ("ebvo_depth_carry_params", "ebvo_depth_carried"):
        assert re.search(rf"\}}\s*{struct};", code), struct
    assert re.search(r"#define EBVO_DEPTH_CARRIED 32u", code) and re.search(r"#define EBVO_DEPTH_CARRY_GATED 64u", code)
    assert lib.ebvo_abi_version() == 6


def test_defaults_are_the_headers():
    from edge_based_visual_odometry_amd import _lib
    p = _lib.DepthCarryParams()
    _lib.load_library().ebvo_depth_carry_default_params(ctypes.byref(p))
    assert {k: getattr(p, k) for k in oc.DEFAULTS} == oc.DEFAULTS and p.reserved == 0 and p.pad == 0
    assert ctypes.sizeof(_lib.DepthCarryParams) == 88 and ctypes.sizeof(_lib.DepthCarried) == 32


@pytest.mark.parametrize("name", list(CASES))
def test_every_case_meets_its_condition(name):
    case = CASES[name]()
    r = cc.run_oracle(case)
    assert case["check"](r), (name, case["note"], {k: r[k] for k in oc.INT_FIELDS}, r["src_index"][:16], r["flags"][:16])
    n = len(case["new_left"])
    assert r["n_new"] == n and r["n_old"] == len(case["kf_left"])
    assert r["n_assoc"] == r["n_carried"] + r["n_gated"] == int((r["src_index"] >= 0).sum())
    assert r["n_live"] <= r["n_sources"] <= r["n_old"]
    assert all(len(r[k]) == n for k in ("lambda_", "info", "n_obs", "flags", "src_index"))
    dead = (r["flags"] & oc.DEAD) != 0
    assert r["n_dead"] == int(dead.sum()) and all(r["flags"][dead] == oc.DEAD)
    assert np.isfinite(r["lambda_"]).all() and (r["info"][~dead] > 0).all() and (r["lambda_"][~dead] > 0).all()
    # properties of the fusion: information never falls below the prior's, lambda' lies between the two measurements
    c = (r["flags"] & oc.CARRIED) != 0
    assert int(c.sum()) == r["n_carried"]
    p = dict(oc.DEFAULTS, **case["params"])
    assert (r["info"][c] >= np.minimum(r["info0"][c], p["info_max"])).all()
    lo, hi = np.minimum(1.0, r["lm"][c]), np.maximum(1.0, r["lm"][c])
    assert ((r["lambda_"][c] >= lo) & (r["lambda_"][c] <= hi)).all()
    rest = ~c & ~dead
    assert all(r["lambda_"][rest] == 1.0) and not r["n_obs"][rest].any()
    assert_bit_equal(r["info"][rest], r["info0"][rest], "the prior of a mate that carried nothing")


def test_the_cases_cover_what_they_name():
    names = set(CASES)
    assert {f"n_new_{n}" for n in (1, 63, 64, 65, 1025)} <= names and set(cc.PICKED) <= names and "n_new_1025" in cc.PICKED
    for n in cc.N_NEW:
        loc = np.array(cc.lattice(n))
        assert loc[:, 0].max() < 190 and loc[:, 1].max() < 110


def test_a_k_left_in_place_of_the_true_right_camera_would_show():
    case = CASES["k_left_fails"]()
    K_left, _, R21, T21 = case["calib"]
    wrong = cc.run_oracle(dict(case, calib=(K_left, K_left, R21, T21)))
    right = cc.run_oracle(case)
    assert wrong["lambda_"].tobytes() != right["lambda_"].tobytes()


def test_identity_promotion_hands_lambda_over_bit_for_bit():
    """the same mates promoted under the identity pose with carry = 1: every mate finds itself (d2 = 0), and the depth the old
    keyframe predicts for it is its own refined one.  lm = Gamma_z / (Gamma_z / lambda_i) is two roundings, so it is lambda_i TO
    THE BIT exactly where Gamma_z / lambda_i is exact -- lambda_i a power of two, asserted on such a state -- and within
    2 ulp of lambda_i otherwise (each division is within half an ulp: (1 + e2) / (1 + e1), |e| <= 2^-53).  On the fused
    lambdas of the euroc scene the oracle shows 82 of 600 mates one ulp off and none further."""
    sc, st = cc._scene("euroc")
    sel = np.flatnonzero(np.isfinite(st[0]) & (st[2] > 0))[:600]
    kfL, kfR = sc["kf_left"][sel], sc["kf_right"][sel]
    kw = dict(carry=1.0, gate_sigmas=np.inf)
    two = np.array([0.5, 1.0, 2.0, 0.25, 4.0])[np.arange(len(sel)) % 5]
    r = oc.carry(kfL, kfR, kfL, kfR, cs.W, cs.H, sc["calib"], np.eye(3), np.zeros(3), state=(two, st[1][sel], st[2][sel]), **kw)
    has = r["src_index"] >= 0
    assert has.sum() > 500 and all(r["src_index"][has] == np.flatnonzero(has))
    assert_bit_equal(r["lm"][has], two[has], "lm against lambda_i")
    state = tuple(v[sel] for v in st)
    r = oc.carry(kfL, kfR, kfL, kfR, cs.W, cs.H, sc["calib"], np.eye(3), np.zeros(3), state=state, **kw)
    has = r["src_index"] >= 0
    assert has.sum() > 500 and all(r["src_index"][has] == np.flatnonzero(has)) and (state[0][has] != 1.0).sum() > 400
    off = np.abs(r["lm"][has] - state[0][has]) / np.spacing(state[0][has])
    print(f"identity promotion on fused lambdas: {int((off > 0).sum())} of {int(has.sum())} mates off, the furthest by {off.max()} ulp")
    assert off.max() <= 2.0


@pytest.mark.parametrize("rig,seed", cs.FIXED_POINT)
def test_fixed_point(rig, seed):
    """noise-free scene, frames 1 .. 4 fused and the state carried to frame 4 at the planted poses: the carried lambda' stays
    at 1 within 10 x the measured worst case (sampling geometry, not rounding: tests/carry_scenes.py says which)"""
    sc = cs.scene(rig, seed)
    assert np.abs(sc["new_lambda_true"] - 1.0).max() == 0.0
    _, r = cs.carried(sc)
    c = (r["flags"] & oc.CARRIED) != 0
    worst = float(np.abs(r["lambda_"][c] - 1.0).max())
    print(f"fixed point {rig} {seed}: max |lambda' - 1| = {worst!r} over {int(c.sum())} carried of {len(c)} new mates, gated {r['n_gated']}")
    assert worst <= 10.0 * cs.FIXED_POINT_MEASURED
    assert c.sum() > 0.9 * len(c)


@pytest.mark.parametrize("k", range(len(cs.NOISY)))
def test_recovery_and_carried_share(k):
    """N(0, 0.25 px) on the disparities of BOTH keyframes: over the carried mates the median |lambda' - lambda_true'| ends below
    the median |1 - lambda_true'| of the prior -- the oracle shows it on all twelve scenes -- and at least half the
    measured share of the live new mates is carried"""
    rig, seed, kind, sigma, clutter = cs.NOISY[k]
    sc = cs.scene(rig, seed, kind, sigma, clutter, sigma_disp=cs.SIGMA_DISP)
    _, r = cs.carried(sc)
    truth = sc["new_lambda_true"]
    c, live = (r["flags"] & oc.CARRIED) != 0, (r["flags"] & oc.DEAD) == 0
    prior, after = float(np.median(np.abs(1.0 - truth[c]))), float(np.median(np.abs(r["lambda_"][c] - truth[c])))
    share = float(c.sum()) / float(live.sum())
    print(f"recovery {rig} {seed} {kind} {sigma} {clutter}: carried {int(c.sum())} of {int(live.sum())} live (share {share:.4f}), gated "
          f"{r['n_gated']}; median |1 - l*| {prior:.5f} -> |l' - l*| {after:.5f}")
    assert after < prior
    assert share >= 0.5 * cs.CARRIED_SHARE_MEASURED[k]
