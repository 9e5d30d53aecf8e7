"""The small parity cases of the handover of the depths on promotion (tests/test_gpu_carry.py compares the device with
tests/oracle_carry.py on each, bit for bit; tests/test_carry_oracle.py checks without a device that each meets its stated
condition).  Every case is a dict of the arguments of oracle_carry.carry / Context.depth_carry plus `note` (the branch it
exercises) and `check` (a predicate on the oracle's result: the condition the case was built for).  Images are 200 x 120.

Two sources:
- `exact`: the rig of tests/align_cases.py whose arithmetic is exact (f = 128, T21 = (0.5, 0, 0); a mate with d px of
  disparity lies at depth 64 / d, and under the identity pose an old mate projects onto its own left location).  New mates
  are hand-placed around those projections; the ratio of an old mate's disparity to the new one's is lm exactly;
- `curves`: a noisy scene per rig of tests/carry_scenes.py with a right camera of its own (so that K_left in its place
  fails), two frames fused, carried to the last frame under its planted pose.
"""
import functools
import math

import numpy as np

from tests import align_cases as ac
from tests import carry_scenes as cs
from tests import oracle_carry as oc

I3, Z3 = ac.I3, ac.Z3
DISP = (8.0, 16.0, 4.0)      # tests/align_cases.py::exact_mates: the disparity of old mate i is DISP[i % 3]
N_NEW = (1, 63, 64, 65, 1025)


def lattice(n):
    """n left locations on halves, 2.5 px apart in x and 5.5 in y: no two within the default radius of one another"""
    return [(14.0 + 2.5 * (k % 68), 14.5 + 5.5 * (k // 68)) for k in range(n)]


def state_of(n, lam=1.0, info=400.0, n_obs=2):
    return np.full(n, lam), np.full(n, info), np.full(n, n_obs, dtype=np.int32)


def exact(locs=ac.SPREAD, new=None, state="default", R=I3, t=Z3, theta=None, w=200, h=120, **params):
    """old mates at locs; new: rows (x, y, theta, disparity), default one per old mate 0.25 px to the right of its projection
    with the mapped orientation and the old mate's own disparity (lm = 1 under the identity pose)"""
    L, Rt = ac.exact_mates(locs, theta)
    n = len(L)
    pr = ac.exact_projection(L, Rt, R, t, w=w, h=h, margin=0.0)
    if new is None:
        new = [own(pr, i) for i in range(n)]
    nl = ac._edges([(x, y, th) for x, y, th, _ in new])
    nr = ac._edges([(x + d, y, th) for x, y, th, d in new])
    return dict(kf_left=L, kf_right=Rt, new_left=nl, new_right=nr, img_w=w, img_h=h, calib=ac.EXACT_CALIB,
                R=np.array(R, dtype=np.float64), t=np.array(t, dtype=np.float64), state=state_of(n) if isinstance(state, str) else state,
                params=dict(params), proj=pr)


def own(pr, i, dx=0.25, dy=0.0, lm=1.0, dth=0.0):
    """a new mate (dx, dy) from old mate i's projection, its orientation the mapped one + dth, its depth lm times old mate i's"""
    return (float(pr["proj_left"][i, 0]) + dx, float(pr["proj_left"][i, 1]) + dy, float(pr["orient_left"][i]) + dth, DISP[i % 3] / lm)


@functools.lru_cache(maxsize=None)
def _scene(rig):
    sc = cs.scene(rig, 0, "mixed", 0.2, 300, sigma_disp=cs.SIGMA_DISP)
    lam, info, nobs, _ = cs.ds.fuse(sc, 2)[-1]
    return sc, (lam, info, nobs)


def curves(rig="euroc", n_old=None, n_new=None, **params):
    sc, st = _scene(rig)
    R, t = sc["poses"][-1]
    o, m = slice(0, n_old), slice(0, n_new)
    return dict(kf_left=sc["kf_left"][o].copy(), kf_right=sc["kf_right"][o].copy(), new_left=sc["new_left"][m].copy(),
                new_right=sc["new_right"][m].copy(), img_w=cs.W, img_h=cs.H, calib=sc["calib"], R=R, t=t,
                state=tuple(v[o].copy() for v in st), params=dict(params))


def run_oracle(case, **kw):
    return oc.carry(case["kf_left"], case["kf_right"], case["new_left"], case["new_right"], case["img_w"], case["img_h"], case["calib"],
                    case["R"], case["t"], state=case["state"], **dict(case["params"], **kw))


def _with_state(case, **edits):
    """state arrays edited: name -> {index: value}"""
    lam, info, nobs = (v.copy() for v in case["state"])
    for k, arr in (("lam", lam), ("info", info), ("n_obs", nobs)):
        for i, v in edits.get(k, {}).items():
            arr[i] = v
    return dict(case, state=(lam, info, nobs))


def _dead_old(case):
    case["kf_left"]["x"][1] = math.nan
    case["kf_right"]["x"][2] -= 40.0          # negative disparity: Gamma_z < 0
    case["kf_right"]["y"][4] = math.inf
    return case


def _dead_new(case):
    case["new_left"]["y"][0] = math.nan
    case["new_right"]["x"][3] -= 40.0
    case["new_right"]["x"][5] = math.inf
    return case


def _chi(inside):
    """mate 0 at lm = 1.0625, gate_sigmas the smallest double that accepts it (inside) or the one below (outside)"""
    c = exact(new=None)
    pr = c["proj"]
    c = exact(new=[own(pr, 0, lm=1.0625)] + [own(pr, i) for i in range(1, 14)], gate_sigmas=math.inf)
    r = run_oracle(c)
    d, v = float(r["lm"][0]) - 1.0, 1.0 / float(r["info0"][0]) + 1.0 / float(r["im"][0])
    gs = math.sqrt((d * d) / v)
    while not d * d <= (gs * gs) * v:
        gs = float(np.nextafter(gs, math.inf))
    while d * d <= (float(np.nextafter(gs, 0.0)) ** 2) * v:
        gs = float(np.nextafter(gs, 0.0))
    c["params"]["gate_sigmas"] = gs if inside else float(np.nextafter(gs, 0.0))
    return c


def _orient(at_threshold):
    """mate 0's orientation 7 degrees off: orient_thr_deg the folded difference itself (strict <: rejected) or the next double"""
    c = exact()
    pr = c["proj"]
    row = own(pr, 0, dth=math.radians(7.0))
    od = abs((float(pr["orient_left"][0]) - row[2]) * oc.ot.RAD_TO_DEG)
    c = exact(new=[row] + [own(pr, i) for i in range(1, 14)], orient_thr_deg=od if at_threshold else float(np.nextafter(od, math.inf)))
    return c


def _wrap():
    c = exact()
    pr = c["proj"]
    o0, o1 = float(pr["orient_left"][0]), float(pr["orient_left"][1])
    rows = [own(pr, 0, dth=-math.copysign(math.pi - 0.05, o0)), own(pr, 1, dth=-math.copysign(2.0 * math.pi - 0.05, o1))]
    return exact(new=rows + [own(pr, i) for i in range(2, 14)])


def cases():
    """name -> case (built on demand: the curve scenes cost seconds)"""
    D, CA, GA = oc.DEAD, oc.CARRIED, oc.CARRY_GATED
    C = {}
    C["n_old_0"] = lambda: dict(exact(locs=[], new=[(50.0 + 9 * k, 40.0, 1.1, 8.0) for k in range(7)]), note="no old mate: no association launched, every new mate at its prior",
                                check=lambda r: r["n_old"] == 0 and r["n_sources"] == 0 and all(r["flags"] == 0) and all(r["src_index"] == -1) and all(r["info"] > 0))
    C["n_new_0"] = lambda: dict(exact(new=[]), note="no new mate: nothing launched", check=lambda r: r["n_new"] == 0 and r["n_old"] == 14 and r["n_live"] == 0)
    C["null_state"] = lambda: dict(exact(state=None), note="NULL in-state: nothing to carry, the priors alone",
                                   check=lambda r: r["n_sources"] == 0 and r["n_assoc"] == 0 and all(r["lambda_"] == 1.0) and all(r["info"] > 0))
    for n in N_NEW:
        C[f"n_new_{n}"] = lambda n=n: dict(exact(locs=lattice(n)), note="wave edges of the counts: 1, 63, 64, 65 mates; five blocks of 256",
                                           check=lambda r, n=n: r["n_new"] == n == r["n_carried"] and all(r["src_index"] == np.arange(n)))
    C["dead_old"] = lambda: dict(_dead_old(exact()), note="old mates with NaN Gamma, Gamma_z <= 0, inf: no sources; their new mates stay at the prior",
                                 check=lambda r: r["n_sources"] == 11 and all(r["src_index"][[1, 2, 4]] == -1) and all(r["flags"][[1, 2, 4]] == 0))
    C["dead_new"] = lambda: dict(_dead_new(exact()), note="dead new mates: lambda 1, info +0, n_obs 0, flag DEAD, no source",
                                 check=lambda r: r["n_dead"] == 3 and all(r["flags"][[0, 3, 5]] == D) and all(r["info"][[0, 3, 5]] == 0.0)
                                 and all(r["src_index"][[0, 3, 5]] == -1) and r["n_carried"] == 11)
    C["lambda_bad"] = lambda: dict(_with_state(exact(), lam={0: math.nan, 1: 0.0, 2: -1.0, 3: math.inf}, info={4: 0.0, 5: -3.0, 6: math.nan}),
                                   note="lambda NaN, 0, negative, inf; info +0, negative, NaN: not sources",
                                   check=lambda r: r["n_sources"] == 7 and all(r["src_index"][:7] == -1) and all(r["src_index"][7:] >= 0))
    C["min_obs"] = lambda: dict(_with_state(exact(min_obs=2), n_obs={0: 1, 1: 2, 2: 0, 3: 3}), note="n_obs below and at min_obs",
                                check=lambda r: list(r["src_index"][:4]) == [-1, 1, -1, 3] and list(r["n_obs"][:4]) == [0, 2, 0, 3])
    C["min_obs_0"] = lambda: dict(_with_state(exact(min_obs=0), n_obs={0: 0}), note="min_obs 0: a mate that fused nothing but has information is a source",
                                  check=lambda r: r["src_index"][0] == 0 and r["n_obs"][0] == 0 and r["flags"][0] == CA)
    C["margin"] = lambda: dict(exact(locs=[(10.0, 40.0), (10.5, 60.0), (50.0, 10.0), (50.0, 10.5), (190.0, 40.0), (189.5, 60.0), (70.0, 110.0), (70.0, 109.5)]),
                               note="projections on the margin are not live, half a pixel inside they are",
                               check=lambda r: r["n_live"] == 4 and list(r["src_index"]) == [-1, 1, -1, 3, -1, 5, -1, 7])
    C["behind"] = lambda: dict(exact(R=np.diag([-1.0, 1.0, -1.0])), note="the pose turns every point behind the camera: sources, none live",
                               check=lambda r: r["n_sources"] == 14 and r["n_live"] == 0 and r["n_assoc"] == 0)
    C["tie_at_radius"] = lambda: dict(exact(locs=[(30.0, 20.0), (104.0, 66.0), (104.0, 62.0), (150.0, 30.0)], theta=1.2, radius=2.0,
                                            new=[(104.0, 64.0, 1.2, 16.0), (30.0, 22.0, 1.2, 8.0), (150.0, 32.5, 1.2, 8.0)]),
                                      note="two sources at equal d2 = radius^2: accepted, the smaller index wins; 2.5 px away: none",
                                      check=lambda r: list(r["src_index"]) == [1, 0, -1])
    C["radius_below"] = lambda: dict(exact(locs=[(104.0, 66.0)], theta=1.2, radius=float(np.nextafter(2.0, 0.0)), new=[(104.0, 64.0, 1.2, 8.0)]),
                                     note="radius one double below the distance: not a candidate", check=lambda r: list(r["src_index"]) == [-1] and r["n_live"] == 1)
    C["orient_at_threshold"] = lambda: dict(_orient(True), note="orientation difference == orient_thr_deg: rejected (strict <)",
                                            check=lambda r: r["src_index"][0] == -1 and all(r["src_index"][1:] >= 0))
    C["orient_inside"] = lambda: dict(_orient(False), note="orient_thr_deg one double above the difference: accepted", check=lambda r: r["src_index"][0] == 0)
    C["orient_wrap"] = lambda: dict(_wrap(), note="differences of almost 180 and almost 360 degrees fold inside the threshold",
                                    check=lambda r: list(r["src_index"][:2]) == [0, 1])
    C["border_cells"] = lambda: dict(exact(locs=[(1.5, 1.5), (198.5, 118.5), (1.5, 118.5), (198.5, 1.5), (100.0, 60.0)], img_margin=0.0, radius=2.0,
                                           new=[(1.0, 1.0, 1.2, 8.0), (199.5, 119.5, 1.2, 16.0), (0.5, 119.0, 1.2, 4.0), (199.0, 0.5, 1.2, 8.0),
                                                (-0.5, 1.5, 1.2, 8.0), (-4.5, 1.5, 1.2, 8.0), (200.5, 118.5, 1.2, 8.0)], theta=1.2),
                                     note="new mates in the four corner cells (clipped windows), in column 0 from x in (-cell, 0) at d2 == radius^2, and in no cell",
                                     check=lambda r: list(r["src_index"]) == [0, 1, 2, 3, 0, -1, -1] and r["n_dead"] == 0)
    C["one_cell"] = lambda: dict(exact(locs=[(104.5, 64.5), (105.0, 65.0), (105.5, 65.5), (106.0, 66.0), (107.5, 67.5)], theta=1.2,
                                       new=[(105.6, 65.7, 1.2, 8.0), (107.0, 67.0, 1.2, 8.0), (104.0, 64.0, 1.2, 8.0)]),
                                 note="several sources in one cell: the nearest of them", check=lambda r: list(r["src_index"]) == [2, 4, 0])
    C["cell_7"] = lambda: dict(exact(locs=lattice(200), cell_size=7), note="a cell size that divides neither 200 nor 120",
                               check=lambda r: r["n_carried"] == 200)
    C["cell_1_radius_8"] = lambda: dict(exact(locs=lattice(65), cell_size=1, radius=8.0, theta=1.2), note="sr = 8 with cells of 1 px: windows of 17 x 17 cells, several candidates",
                                        check=lambda r: all(r["src_index"] == np.arange(65)))
    C["lm_on_bounds"] = lambda: dict(exact(new=[own(exact()["proj"], 0, lm=0.25), own(exact()["proj"], 1, lm=4.0), own(exact()["proj"], 2, lm=0.125),
                                                own(exact()["proj"], 3, lm=8.0)], gate_sigmas=math.inf),
                                     note="lm == lambda_min and == lambda_max are accepted; 0.125 and 8 are gated",
                                     check=lambda r: list(r["lm"]) == [0.25, 4.0, 0.125, 8.0] and list(r["flags"]) == [CA, CA, GA, GA]
                                     and all(r["lambda_"][2:] == 1.0) and all(r["n_obs"][2:] == 0))
    C["chi_on"] = lambda: dict(_chi(True), note="d d == gate^2 v: accepted", check=lambda r: r["flags"][0] == CA and 1.06 < r["lm"][0] < 1.065)
    C["chi_outside"] = lambda: dict(_chi(False), note="gate_sigmas one double below: gated, the prior", check=lambda r: r["flags"][0] == GA and r["lambda_"][0] == 1.0
                                    and r["n_gated"] == 1 and r["n_assoc"] == 14)
    C["gate_inf"] = lambda: dict(curves("euroc", 700, 700, gate_sigmas=math.inf), note="no chi gate: only the lambda range gates",
                                 check=lambda r: r["n_carried"] > 400)
    C["gate_tight"] = lambda: dict(curves("euroc", 700, 700, gate_sigmas=0.5), note="a tight chi gate on the noisy scene: many gated",
                                   check=lambda r: r["n_gated"] > 50 and r["n_carried"] > 50)
    C["info_max"] = lambda: dict(exact(info_max=10.0), note="h above info_max: clipped", check=lambda r: all(r["info"] == 10.0) and r["n_carried"] == 14)
    C["info_max_inf"] = lambda: dict(exact(info_max=math.inf), note="no clip", check=lambda r: all(r["info"] > r["info0"]))
    C["carry_1"] = lambda: dict(exact(carry=1.0), note="no discount", check=lambda r: r["n_carried"] == 14 and
                                all(r["im"] >= 400.0 * 0.999))
    C["im_overflow"] = lambda: dict(_with_state(exact(), info={0: math.inf, 1: 1e-320, 2: 5e-324}), note="im = +inf and im = +0 (half the smallest denormal): gated; a denormal im still fuses",
                                    check=lambda r: list(r["flags"][:3]) == [GA, CA, GA])
    C["translated"] = lambda: dict(exact(t=(0.02, -0.015, 0.04)), note="a pose with a translation: zp differs from Gamma_z, lm != 1",
                                   check=lambda r: r["n_carried"] >= 10 and (r["lm"][r["src_index"] >= 0] != 1.0).all())
    for rig in ("euroc", "kitti"):
        C[f"{rig}_all"] = lambda rig=rig: dict(curves(rig, None, 1025), note="the all-round scene of the rig, its own right camera, 1025 new mates",
                                               check=lambda r: r["n_carried"] > 800 and r["n_live"] > 1000 and (r["lambda_"] != 1.0).sum() > 800)
    C["k_left_fails"] = lambda: dict(curves("euroc", 300, 300), note="a true right camera: Gamma under K_right := K_left differs",
                                     check=lambda r: r["n_carried"] > 100)
    return C


PICKED = ("n_new_1025", "euroc_all", "tie_at_radius", "chi_outside")   # launch geometry and the second call
