"""The small parity cases of the keyframe coverage (tests/test_gpu_cover.py compares the device with tests/oracle_cover.py on
each, bit for bit; tests/test_cover_oracle.py checks without a device that each meets its stated condition).  Every case is a
dict of the arguments of oracle_cover.cover / Context.keyframe_cover_edges plus `note` (the branch it exercises) and `check` (a
predicate on the oracle's result: the condition the case was built for).  Images are 200 x 120.

Two sources:
- `exact`: the rig of tests/align_cases.py whose arithmetic is exact (f = 128, T21 = (0.5, 0, 0); under the identity pose a
  mate projects onto its own left location, so its displacement is 0), every mate with an edge of its own 0.25 px along the
  normal of its projection;
- `curves`: one noisy scene per rig of tests/depth_scenes.py, the keyframe against its third frame at the planted pose.
"""
import functools
import math

import numpy as np

from tests import align_cases as ac
from tests import depth_scenes as ds
from tests import oracle_cover as ocv

I3, Z3 = ac.I3, ac.Z3
N_KF = (1, 63, 64, 65, 1024, 1025)
N0 = (1, 64, 65)
SHIFT = (0.02, -0.015, 0.04)     # a translation that moves every projection of the exact rig off its keyframe location


def lattice(n):
    """n left locations on halves, 2.5 px apart in x and 5.5 in y: every mate's own edge (0.25 px away) is its nearest"""
    return [(14.0 + 2.5 * (k % 68), 14.5 + 5.5 * (k // 68)) for k in range(n)]


def exact(locs=ac.SPREAD, R=I3, t=Z3, lambda_=None, extra=(), drop_own=(), theta=None, n0=None, **params):
    c = ac.exact(extra_left=extra, locs=locs, drop_own=drop_own, theta=theta)
    E = c["edges_left"] if n0 is None else c["edges_left"][:n0].copy()
    return dict(kf_left=c["kf_left"], kf_right=c["kf_right"], lambda_=lambda_, edges_left=E, img_w=200, img_h=120, calib=ac.EXACT_CALIB,
                R=np.array(R, dtype=np.float64), t=np.array(t, dtype=np.float64), params=dict(params))


@functools.lru_cache(maxsize=None)
def _scene(rig):
    sc = ds.scene(rig, 0, "mixed", 0.2, 300, sigma_disp=ds.SIGMA_DISP)
    lam = ds.fuse(sc, 2)[-1][0]
    return sc, lam


def curves(rig="euroc", frame=3, lambda_=False, n_kf=None, **params):
    sc, lam = _scene(rig)
    R, t = sc["poses"][frame - 1]
    o = slice(0, n_kf)
    return dict(kf_left=sc["kf_left"][o].copy(), kf_right=sc["kf_right"][o].copy(), lambda_=lam[o].copy() if lambda_ else None,
                edges_left=sc["frames"][frame - 1][0].copy(), img_w=ds.W, img_h=ds.H, calib=sc["calib"], R=R, t=t, params=dict(params))


def run_oracle(case, **kw):
    return ocv.cover(case["kf_left"], case["kf_right"], case["lambda_"], case["edges_left"], case["img_w"], case["img_h"], case["calib"],
                     case["R"], case["t"], **dict(case["params"], **kw))


def _dead(case, every=False):
    n = len(case["kf_left"])
    if every:
        case["kf_right"]["x"] -= 40.0            # negative disparity: Gamma_z < 0
        return case
    assert n > 5
    case["kf_left"]["x"][1] = math.nan
    case["kf_right"]["x"][2] -= 40.0
    case["kf_right"]["y"][4] = math.inf
    return case


def _dead_projecting():
    """every mate behind the keyframe's camera (Gamma_z < 0) under a pose that turns it in front of the current one, with an edge
    at each projection: the alignment's association on its own takes them"""
    c = _dead(exact(R=np.diag([-1.0, 1.0, -1.0])), every=True)
    pr = ocv.ot.project(c["kf_left"], c["kf_right"], c["R"], c["t"], c["calib"], 200, 120)
    c["edges_left"] = ac._edges([(float(q[0]), float(q[1]), float(o)) for q, o in zip(pr["proj_left"], pr["orient_left"])])
    return c


def _turned(case, by=0.5):
    case["edges_left"]["theta"] += by
    return case


def _shared():
    """mates 0 at (104, 64) and 14 at (106, 64) without edges of their own, one edge between them that both accept"""
    c = exact(locs=ac.SPREAD + [(106.0, 64.0)], theta=1.2, drop_own=(0, 14))
    o = float(ac.exact_projection(c["kf_left"], c["kf_right"])["orient_left"][0])
    return exact(locs=ac.SPREAD + [(106.0, 64.0)], theta=1.2, drop_own=(0, 14), extra=[(105.0, 64.0, o)])


def _cell_threshold(field, above):
    """min_cell_edges / min_cell_explained exactly at the fullest cell's count, or one above it"""
    base = exact(locs=lattice(200), min_cell_edges=1, min_cell_explained=1)
    top = int(run_oracle(base)["cell_edges" if field == "min_cell_edges" else "cell_explained"].max())
    base["params"][field] = top + (1 if above else 0)
    return base


def _bin_edge(on):
    """bin_px the displacement of mate 0 itself (d / bin_px == 1.0: bin 1) or the next double (the quotient is below 1: bin 0)"""
    c = exact(t=SHIFT)
    d = float(run_oracle(c)["disp"][0])
    assert d > 0.0
    c["params"]["bin_px"] = d if on else float(np.nextafter(d, math.inf))
    return c


def _inlier(at):
    """inlier_px = |r| of mate 0 (strict <: not an inlier) or the next double above it (|r| one ulp below: an inlier)"""
    c = exact()
    r = abs(float(run_oracle(c)["residual"][0]))
    assert 0.2 < r < 0.3
    c["params"]["inlier_px"] = r if at else float(np.nextafter(r, math.inf))
    return c


def _bin_of(r, i, case):
    return r["disp"][i] / dict(ocv.DEFAULTS, **case["params"])["bin_px"]


def cases():
    """name -> case (built on demand: the curve scenes cost seconds)"""
    D, F, A, IN = ocv.DEAD, ocv.IN_FRAME, ocv.ASSOCIATED, ocv.INLIER
    C = {}
    for n in N_KF:
        C[f"n_kf_{n}"] = lambda n=n: dict(exact(locs=lattice(n)), note="wave and block edges of the mate kernel: 1, 63, 64, 65 mates; four and five blocks of 256",
                                          check=lambda r, n=n: r["n_kf"] == n == r["n_in_frame"] == r["n_assoc"] == r["n_explained"] == r["n_inliers"]
                                          and all(r["assoc"] == np.arange(n)) and r["hist"][0] == n and r["disp_median_bin"] == 0)
    for n0 in N0:
        C[f"n0_{n0}"] = lambda n0=n0: dict(exact(locs=lattice(65), n0=n0), note="edge lists of 1, 64 and 65 edges: the wave edges of the edge kernel",
                                           check=lambda r, n0=n0: r["n_edges"] == n0 == r["n_assoc"] == r["n_explained"] and r["n_in_frame"] == 65
                                           and int(r["cell_edges"].sum()) == n0)
    C["n_kf_0"] = lambda: dict(exact(locs=[], extra=[(50.0, 40.0, 1.0)]), note="no mate: nothing launched",
                               check=lambda r: r["n_kf"] == 0 and r["n_edges"] == 1 and r["disp_median_bin"] == -1 and not r["cell_edges"].any())
    C["n0_0"] = lambda: dict(exact(n0=0), note="no edge: nothing launched, a zero record but for the sizes",
                             check=lambda r: r["n_kf"] == 14 and r["n_edges"] == 0 and r["n_in_frame"] == 0 and r["n_dead"] == 0
                             and (r["cw"], r["ch"]) == (7, 4) and r["disp_median_bin"] == -1 and all(r["assoc"] == -1) and np.isnan(r["disp"]).all())
    C["all_dead"] = lambda: dict(_dead(exact(), every=True), note="every mate dead: flags DEAD alone, no bin, no median",
                                 check=lambda r: r["n_dead"] == 14 and all(r["flags"] == D) and r["n_in_frame"] == 0 and r["disp_median_bin"] == -1
                                 and not r["hist"].any() and r["n_explained"] == 0)
    C["dead_but_projecting"] = lambda: dict(_dead_projecting(),
                                            note="Gamma_z < 0 turned in front of the camera: the alignment's association finds the mates' own edges, the coverage does not count them",
                                            check=lambda r: (r["assoc_raw"] >= 0).sum() > 5 and all(r["flags"] == D) and all(r["assoc"] == -1) and r["n_explained"] == 0)
    C["some_dead"] = lambda: dict(_dead(exact()), note="mates with NaN Gamma, Gamma_z <= 0, inf among live ones; their own edges stay unexplained",
                                  check=lambda r: r["n_dead"] == 3 and all(r["flags"][[1, 2, 4]] == D) and r["n_assoc"] == 11 == r["n_explained"]
                                  and np.isnan(r["disp"][[1, 2, 4]]).all())
    C["out_of_frame"] = lambda: dict(exact(t=(100.0, 0.0, 0.0)), note="the pose moves every projection out of the image: live mates, none in frame",
                                     check=lambda r: r["n_dead"] == 0 and r["n_in_frame"] == 0 and not r["flags"].any() and r["disp_median_bin"] == -1
                                     and np.isnan(r["disp"]).all())
    C["behind"] = lambda: dict(exact(R=np.diag([-1.0, 1.0, -1.0])), note="the pose turns every point behind the camera: not in frame",
                               check=lambda r: r["n_in_frame"] == 0 and r["n_dead"] == 0)
    C["nothing_associated"] = lambda: dict(_turned(exact(locs=lattice(65), min_cell_edges=1)), note="every edge half a radian off its mate's orientation: in frame, none associated, no cell covered",
                                           check=lambda r: r["n_in_frame"] == 65 and r["n_assoc"] == 0 == r["n_explained"] and r["n_cells_cur"] > 0
                                           and r["n_cells_covered"] == 0 and all(r["flags"] == F))
    C["shared_edge"] = lambda: dict(_shared(), note="two mates on one edge: it is explained once",
                                    check=lambda r: r["assoc"][0] == r["assoc"][14] >= 0 and r["n_assoc"] == 15 and r["n_explained"] == 14)
    C["nan_edge"] = lambda: dict(exact(extra=[(math.nan, 64.0, 1.0), (50.0, math.inf, 1.0), (-40.0, 30.0, 1.0)]),
                                 note="edges with NaN x, inf y and x left of every cell: in no coarse cell, never explained",
                                 check=lambda r: r["n_edges"] == 17 and int(r["cell_edges"].sum()) == 14 and not r["explained"][14:].any() and r["n_explained"] == 14)
    C["lambda_given"] = lambda: dict(curves("euroc", lambda_=True), note="Gamma / lambda: some association differs from the one on the triangulated Gamma",
                                     check=lambda r: (r["assoc"] != run_oracle(curves("euroc"))["assoc"]).any() and r["n_assoc"] > 300)
    C["lambda_null"] = lambda: dict(curves("euroc"), note="lambda NULL on the same scene", check=lambda r: r["n_assoc"] > 300)
    C["lambda_bad"] = lambda: dict(exact(lambda_=np.array([1.0, math.nan, 0.0, -1.0, math.inf, 2.0] + [1.0] * 8)),
                                   note="lambda NaN, 0, negative, inf of live mates: not in frame; lambda 2 halves the depth and keeps the projection",
                                   check=lambda r: list(r["flags"][1:5]) == [0, 0, 0, 0] and r["n_dead"] == 0 and r["flags"][5] == (F | A | IN) and r["n_in_frame"] == 10)
    for cell, grid in ((32, (7, 4)), (7, (29, 18)), (500, (1, 1))):
        C[f"cover_cell_{cell}"] = lambda cell=cell, grid=grid: dict(curves("kitti", cover_cell=cell), note="coarse cells of 32 px (a partial last column), 7 px and one cell for the image",
                                                                    check=lambda r, grid=grid: (r["cw"], r["ch"]) == grid and 0 < r["n_cells_covered"] <= r["n_cells_cur"] <= grid[0] * grid[1]
                                                                    and int(r["cell_edges"].sum()) == r["n_edges"])
    C["min_cell_edges_at"] = lambda: dict(_cell_threshold("min_cell_edges", False), note="min_cell_edges == the fullest cell's count: that cell counts",
                                          check=lambda r: r["n_cells_cur"] == int((r["cell_edges"] == r["cell_edges"].max()).sum()) >= 1)
    C["min_cell_edges_above"] = lambda: dict(_cell_threshold("min_cell_edges", True), note="one above: no cell counts", check=lambda r: r["n_cells_cur"] == 0 == r["n_cells_covered"] and r["n_explained"] == 200)
    C["min_cell_explained_at"] = lambda: dict(_cell_threshold("min_cell_explained", False), note="min_cell_explained == the best cell's count: covered",
                                              check=lambda r: r["n_cells_covered"] == int((r["cell_explained"] == r["cell_explained"].max()).sum()) >= 1)
    C["min_cell_explained_above"] = lambda: dict(_cell_threshold("min_cell_explained", True), note="one above: no cell is covered", check=lambda r: r["n_cells_covered"] == 0 < r["n_cells_cur"])
    C["bin_edge_on"] = lambda: (lambda c: dict(c, note="d / bin_px == 1.0: bin 1", check=lambda r: _bin_of(r, 0, c) == 1.0 and r["hist"][1] >= 1 and r["n_in_frame"] == int(r["hist"].sum())))(_bin_edge(True))
    C["bin_edge_below"] = lambda: (lambda c: dict(c, note="bin_px the next double: the quotient is below 1, bin 0", check=lambda r: _bin_of(r, 0, c) < 1.0 and r["hist"][0] >= 1))(_bin_edge(False))
    C["bin_saturated"] = lambda: dict(exact(t=SHIFT, bin_px=1e-3), note="a tiny bin_px: every displacement saturates into bin 63",
                                      check=lambda r: r["hist"][63] == r["n_in_frame"] > 0 and r["disp_median_bin"] == 63 and not r["hist"][:63].any())
    C["inlier_at"] = lambda: dict(_inlier(True), note="|r| == inlier_px: not an inlier (strict <)", check=lambda r: r["flags"][0] == (F | A) and r["n_inliers"] < r["n_assoc"])
    C["inlier_below"] = lambda: dict(_inlier(False), note="|r| one ulp below inlier_px: an inlier", check=lambda r: r["flags"][0] == (F | A | IN))
    C["inlier_0"] = lambda: dict(exact(inlier_px=0.0), note="inlier_px 0: no inlier", check=lambda r: r["n_inliers"] == 0 and r["n_assoc"] == 14)
    C["cell_7_radius_2"] = lambda: dict(exact(locs=lattice(200), t=SHIFT, cell_size=7, radius=2.0), note="the alignment's grid at a cell size that divides neither 200 nor 120",
                                        check=lambda r: r["n_assoc"] > 100 and r["disp_median_bin"] >= 0)
    for rig in ("kitti", "euroc"):
        C[f"{rig}_all"] = lambda rig=rig: dict(curves(rig, lambda_=True), note="the all-round noisy scene of the rig against its third frame, on the fused lambda",
                                               check=lambda r: r["n_in_frame"] > 0.5 * r["n_kf"] and r["n_assoc"] > 0.5 * r["n_in_frame"] and r["n_inliers"] > 0.5 * r["n_assoc"]
                                               and r["n_explained"] < r["n_assoc"] and r["disp_median_bin"] > 0 and int((r["hist"] > 0).sum()) > 3)
    return C


PICKED = ("n_kf_1025", "euroc_all", "bin_edge_on", "shared_edge")   # launch geometry and the second call
