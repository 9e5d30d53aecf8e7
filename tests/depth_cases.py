"""The small parity cases of the inverse-depth filter (tests/test_gpu_depth.py compares the device with tests/oracle_depth.py
on each, bit for bit; tests/test_depth_oracle.py checks without a device that each meets its stated condition).  Every case is
a dict of the arguments of oracle_depth.update / Context.depth_refine_edges plus `note` (the branch it exercises) and `check`
(a predicate on the oracle's result: the condition the case was built for).

Two sources, both of tests/align_cases.py:
- `curves`: the noisy scene per rig with a right camera of its own (true_right, so that K_left in its place fails), the
  association the alignment's oracle makes under the perturbed pose, cut to the sizes the tile and wave edges need;
- `exact`: the rig whose arithmetic is exact, every mate with an edge of its own 0.25 px from its projection in both images,
  under a pose with a translation (under the identity the left camera does not see lambda at all).
"""
import functools
import math

import numpy as np

from tests import align_cases as ac
from tests import oracle_depth as od

N_KF = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)

# Fixed point (tests/test_depth_oracle.py::test_fixed_point): the largest |lambda - 1| the oracle shows on the noise-free scenes
# of tests/depth_scenes.py::FIXED_POINT, fused over four frames at the planted poses.  Measured with tests/oracle_depth.py
# (euroc seed 0; kitti 7.5e-5); the test asserts 10 x this.  It is not rounding: the current frame samples the arcs at other
# parameters, 0.5 px apart, and the chord between two samples leaves the arc by its sagitta, which the short-baseline rig turns
# into the larger lambda.
FIXED_POINT_MEASURED = 0.0003433177593632486


@functools.lru_cache(maxsize=None)
def _assoc(rig):
    """the association of every mate of the rig's scene under the perturbed pose (per mate: independent of the other mates)"""
    sc, order, R0, t0 = ac._base(rig)
    return od.associate(sc["kf_left"], sc["kf_right"], None, sc["edges_left"], sc["edges_right"], ac.asc.W, ac.asc.H, sc["calib"], R0, t0)


def curves(rig="euroc", n_kf=None, state=None, **params):
    sc, order, R0, t0 = ac._base(rig)
    sel = order[:n_kf] if n_kf is not None else order
    a = _assoc(rig)
    return dict(kf_left=sc["kf_left"][sel].copy(), kf_right=sc["kf_right"][sel].copy(), edges_left=sc["edges_left"].copy(),
                edges_right=sc["edges_right"].copy(), assoc_left=a[0][sel].copy(), assoc_right=a[1][sel].copy(), img_w=ac.asc.W,
                img_h=ac.asc.H, calib=sc["calib"], R=R0, t=t0, state=state, params=dict(params))


T_EXACT = (0.02, -0.015, 0.04)


def exact(theta=None, state=None, **params):
    """the exact rig: mate i is associated with its own edge i in both images; the pose translates the camera"""
    c = ac.exact(theta=theta)
    n = len(c["kf_left"])
    own = np.arange(n, dtype=np.int32)
    return dict(kf_left=c["kf_left"], kf_right=c["kf_right"], edges_left=c["edges_left"], edges_right=c["edges_right"], assoc_left=own.copy(),
                assoc_right=own.copy(), img_w=c["img_w"], img_h=c["img_h"], calib=c["calib"], R=np.eye(3), t=np.array(T_EXACT), state=state,
                params=dict(params))


def run_oracle(case, **kw):
    return od.update(case["kf_left"], case["kf_right"], case["edges_left"], case["edges_right"], case["assoc_left"], case["assoc_right"],
                     case["img_w"], case["img_h"], case["calib"], case["R"], case["t"], state=case["state"], **dict(case["params"], **kw))


def _residual0(case):
    """|r| of mate 0's left term at the incoming lambda"""
    return float(abs(run_oracle(case, gate_px=math.inf, iterations=0)["residual_in"][0][0]))


def _gate(inside):
    c = exact()
    rho = _residual0(c)
    c["params"]["gate_px"] = rho if inside else float(np.nextafter(rho, 0.0))
    return c


def _edit(case, **arrays):
    """a case with mates or associations edited by fn(array) in place"""
    for k, fn in arrays.items():
        fn(case[k])
    return case


def _dead(case):
    def left(e):
        e["x"][1] = math.nan

    def right(e):
        e["x"][2] = e["x"][2] - 40.0          # negative disparity: Gamma_z < 0
        e["y"][4] = math.inf
    _edit(case, kf_left=left)
    _edit(case, kf_right=right)
    return case


def _flat_edges(case):
    """every edge along the rig's (horizontal) epipolar direction: n = (sin theta, -cos theta) = (~0, -1) has no component along
    it, and under a translation along the baseline both cameras' j is ~0"""
    for k in ("edges_left", "edges_right"):
        case[k]["theta"][:] = 1e-9
    case["t"] = np.array((0.03, 0.0, 0.0))
    return case


def _second(case):
    """the state one update left, fused again"""
    r = run_oracle(case)
    return dict(case, state=(r["lambda_"], r["info"], r["n_obs"]))


def cases():
    """name -> case (built on demand: the curve scenes and their association cost seconds)"""
    U, R_, D = od.UPDATED, od.RESTORED, od.DEAD
    C = {}
    for n in N_KF:
        for cams in (1, 2):
            C[f"n_kf_{n}_cameras_{cams}"] = lambda n=n, cams=cams: dict(
                curves("euroc", n_kf=n, cameras=cams), note="wave and tile edges: 64-lane trees, 1 / 2 / 3 tiles; one and two cameras",
                check=lambda r, n=n, cams=cams: r["n_kf"] == n and (cams == 2 or r["n_terms"][1] == 0) and (n < 63 or r["n_updated"] > 0))
    C["kitti_all"] = lambda: dict(curves("kitti"), note="every mate of the other rig's scene, its own right camera",
                                  check=lambda r: r["n_updated"] > 1000 and r["n_terms"][1] > 1000)
    C["no_association"] = lambda: dict(_edit(exact(), assoc_left=lambda a: a.__setitem__(slice(0, 3), -1),
                                             assoc_right=lambda a: a.__setitem__(slice(0, 3), -1)),
                                       note="mates without a term in either camera: restored, counted in n_restored",
                                       check=lambda r: all(r["flags"][:3] == R_) and r["n_restored"] >= 3)
    C["left_only"] = lambda: dict(_edit(exact(), assoc_right=lambda a: a.__setitem__(slice(0, 5), -1)),
                                  note="mates seen by the left camera only", check=lambda r: all(r["flags"][:5] == U))
    C["right_only"] = lambda: dict(_edit(exact(), assoc_left=lambda a: a.__setitem__(slice(0, 5), -1)),
                                   note="mates seen by the right camera only", check=lambda r: all(r["flags"][:5] == U))
    C["assoc_null_right"] = lambda: dict(dict(exact(), assoc_right=None), note="a NULL association array: no term in that camera",
                                         check=lambda r: r["n_terms"][1] == 0 and r["n_terms"][0] > 0)
    C["assoc_out_of_range"] = lambda: dict(_edit(exact(), assoc_left=lambda a: a.__setitem__(slice(0, 2), (10 ** 6, -7)),
                                                 assoc_right=lambda a: a.__setitem__(slice(0, 2), (14, -2 ** 31))),
                                           note="indices outside [0, n_c) are no association (14 = n_c exactly)",
                                           check=lambda r: all(r["flags"][:2] == R_))
    C["gate_inside"] = lambda: dict(_gate(True), note="|r| == gate_px survives",
                                    check=lambda r: not r["flags"][0] & od.GATED_LEFT and r["flags"][0] & U)
    C["gate_outside"] = lambda: dict(_gate(False), note="gate_px one double below |r|: the term is dropped and counted",
                                     check=lambda r: r["flags"][0] & od.GATED_LEFT and r["n_gated"][0] >= 1)
    C["gate_small"] = lambda: dict(curves("euroc", n_kf=700, gate_px=0.3), note="a tight gate on the noisy scene: many terms gated, some mates lose both",
                                   check=lambda r: min(r["n_gated"]) > 20 and r["n_restored"] > 0)
    C["gate_inf"] = lambda: dict(curves("euroc", n_kf=300, gate_px=math.inf), note="no gate", check=lambda r: r["n_gated"] == (0, 0))
    C["dead"] = lambda: dict(_dead(exact()), note="Gamma_z <= 0, NaN and inf coordinates: dead, never updated, counted or scaled",
                             check=lambda r: r["n_dead"] == 3 and all(r["flags"][[1, 2, 4]] == D) and all(r["n_obs"][[1, 2, 4]] == 0))
    C["dead_with_state"] = lambda: dict(_second(_dead(exact())), note="a dead mate's incoming state passes through",
                                        check=lambda r: r["n_dead"] == 3 and all(r["lambda_"][[1, 2, 4]] == 1.0))
    C["restored_range"] = lambda: dict(curves("euroc", n_kf=500, lambda_min=0.97, lambda_max=1.03),
                                       note="updates that leave [lambda_min, lambda_max] are restored",
                                       check=lambda r: r["n_restored"] > 50 and r["n_updated"] > 50 and
                                       all(r["lambda_"][(r["flags"] & R_) != 0] == 1.0))
    C["info_clipped"] = lambda: dict(curves("euroc", n_kf=300, info_max=10.0), note="info clipped at info_max (below the prior's)",
                                     check=lambda r: all(r["info"][(r["flags"] & U) != 0] == 10.0))
    C["info_max_inf"] = lambda: dict(curves("euroc", n_kf=300, info_max=math.inf), note="no clip", check=lambda r: r["info"].max() > 10.0)
    C["iterations_0"] = lambda: dict(curves("euroc", n_kf=300, iterations=0), note="no step: info alone is updated",
                                     check=lambda r: all(r["lambda_"] == 1.0) and r["n_updated"] > 100 and r["rms_before"] == r["rms_after"])
    C["iterations_1"] = lambda: dict(curves("euroc", n_kf=300, iterations=1), note="one step", check=lambda r: r["rms_after"] < r["rms_before"])
    C["iterations_16"] = lambda: dict(curves("euroc", n_kf=300, iterations=16), note="the largest accepted step count",
                                      check=lambda r: r["rms_after"] < r["rms_before"])
    C["huber_inf"] = lambda: dict(curves("euroc", n_kf=300, huber_px=math.inf), note="least squares", check=lambda r: r["n_updated"] > 100)
    C["huber_small"] = lambda: dict(curves("euroc", n_kf=300, huber_px=0.05), note="most terms beyond the Huber threshold",
                                    check=lambda r: r["n_updated"] > 100)
    C["flat_edges"] = lambda: dict(_flat_edges(exact()), note="edges along the epipolar direction: j ~ 0, lambda barely moves",
                                   check=lambda r: r["n_updated"] > 0 and float(np.abs(r["lambda_"] - 1.0).max()) < 1e-6)
    C["second_update"] = lambda: dict(_second(curves("euroc", n_kf=1025)), note="an incoming state (lambda, info, n_obs) instead of the prior",
                                      check=lambda r: r["n_obs"].max() == 2)
    C["margin_wide"] = lambda: dict(curves("euroc", n_kf=500, img_margin=50.0), note="projections inside a 50 px margin are not live: no term, not gated",
                                    check=lambda r: r["n_gated"] == (0, 0) or sum(r["n_terms"]) < 700)
    C["sigma_odd"] = lambda: dict(curves("kitti", n_kf=400, sigma_disp_px=0.6, sigma_normal_px=0.13), note="other noise levels",
                                  check=lambda r: r["n_updated"] > 100)
    return C
