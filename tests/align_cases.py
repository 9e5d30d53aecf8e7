"""The small parity cases of the edge alignment (tests/test_gpu_align.py compares the device with tests/oracle_align.py on each,
bit for bit; tests/test_align_oracle.py runs the oracle's properties on some).  Every case is a dict of the arguments of
oracle_align.align / Context.pose_align_edges plus `note`: the branch it exercises.

Two sources:
- `curves`: one noisy scene of tests/align_scenes.py per rig with a right camera of its own (true_right), cut to the sizes the
  kernels' groupings need, started from the perturbed pose;
- `exact`: a rig whose arithmetic is exact (f = 128, principal point (100, 60), R21 = I, T21 = (0.5, 0, 0), mates 8 px
  apart: rho = 8 and every projection under the identity pose is the mate's own left location, on the grid's boundaries when
  the location is), with hand-placed edges around the projections.
"""
import functools
import math

import numpy as np

from tests import align_scenes as asc
from tests import oracle as orc
from tests import oracle_tgt as ot

N_KF = (1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 2049)
QUICK = dict(rounds=2, iterations=4)


@functools.lru_cache(maxsize=None)
def _base(rig):
    sc = asc.scene(rig, 5, "mixed", sigma=0.2, clutter=300, true_right=True)
    order = np.random.default_rng(11).permutation(len(sc["kf_left"]))     # a prefix of the mates spreads over every curve
    R0, t0 = asc.perturbed(sc["R_gt"], sc["t_gt"])
    return sc, order, R0, t0


def curves(rig="euroc", n_kf=None, n0=None, n1=None, **params):
    sc, order, R0, t0 = _base(rig)
    sel = order[:n_kf] if n_kf is not None else order
    E0, E1 = sc["edges_left"], sc["edges_right"]
    return dict(kf_left=sc["kf_left"][sel].copy(), kf_right=sc["kf_right"][sel].copy(),
                edges_left=(E0 if n0 is None else E0[:n0]).copy(), edges_right=(E1 if n1 is None else E1[:n1]).copy(),
                img_w=asc.W, img_h=asc.H, calib=sc["calib"], R0=R0, t0=t0, params=dict(params))


# ---- the exact rig ------------------------------------------------------------------------------------------------------
EXACT_CALIB = (np.array([[128.0, 0, 100.0], [0, 128.0, 60.0], [0, 0, 1.0]]), np.array([[128.0, 0, 100.0], [0, 128.0, 60.0], [0, 0, 1.0]]),
               np.eye(3), np.array([0.5, 0.0, 0.0]))
I3, Z3 = np.eye(3), np.zeros(3)


def _edges(rows):
    e = np.zeros(len(rows), dtype=orc.EDGE_DTYPE)
    for k, (x, y, th) in enumerate(rows):
        e[k] = (x, y, th, k, 0)
    return e


def exact_mates(locs, theta=None):
    """mates at the given left locations (integers or halves) with 8, 16 or 4 px of disparity (mate 0: 8): rho = 8, 4 or 16,
    Gamma = rho K^-1 (x, y, 1), and the projection under the identity pose is (x, y).  theta = None: a different orientation
    per mate, away from the horizontal (where the two tangent planes coincide)"""
    th = [0.9 + 0.23 * (i % 7) if theta is None else theta for i in range(len(locs))]
    L = _edges([(x, y, th[i]) for i, (x, y) in enumerate(locs)])
    R = _edges([(x + (8.0, 16.0, 4.0)[i % 3], y, th[i]) for i, (x, y) in enumerate(locs)])
    return L, R


def exact_projection(L, R, R0=I3, t0=Z3, w=200, h=120, margin=10.0):
    return ot.project(L, R, R0, t0, EXACT_CALIB, w, h, img_margin=margin)


# fourteen mates spread over the image (enough terms for min_terms = 12 with one camera); the crafted cases hang their edges
# on mate 0 at (104, 64): a corner of cells of 1, 2, 4 and 8 px
SPREAD = [(104.0, 64.0), (30.5, 20.0), (60.0, 90.5), (150.0, 30.0), (170.5, 95.0), (45.0, 55.0), (120.0, 100.0), (80.5, 25.5),
          (140.0, 70.0), (25.0, 100.0), (165.0, 50.5), (95.0, 40.0), (55.5, 75.0), (130.0, 15.5)]


def exact(extra_left=(), extra_right=(), locs=SPREAD, drop_own=(), w=200, h=120, R0=I3, t0=Z3, theta=None, **params):
    """every mate but those in drop_own has an edge of its own at its projection + 0.25 px along the normal in both images
    (orientation = the mapped one); extra_*: rows (x, y, theta) appended to the lists"""
    L, R = exact_mates(locs, theta)
    pr = exact_projection(L, R, w=w, h=h)
    rows = [[], []]
    for c, (q, o) in enumerate(((pr["proj_left"], pr["orient_left"]), (pr["proj_right"], pr["orient_right"]))):
        for i in range(len(L)):
            if i not in drop_own:
                rows[c].append((q[i, 0] + 0.25 * math.sin(o[i]), q[i, 1] - 0.25 * math.cos(o[i]), float(o[i])))
    rows[0] += list(extra_left)
    rows[1] += list(extra_right)
    return dict(kf_left=L, kf_right=R, edges_left=_edges(rows[0]), edges_right=_edges(rows[1]), img_w=w, img_h=h, calib=EXACT_CALIB,
                R0=np.array(R0, dtype=np.float64), t0=np.array(t0, dtype=np.float64), params=dict(params))


def _o0():
    """mapped orientation of mate 0 in the left image under the identity pose"""
    L, R = exact_mates(SPREAD)
    return float(exact_projection(L, R)["orient_left"][0])


def _segment_case(k):
    """a cell (cell_size 4: x in [104, 108), y in [64, 68)) holding exactly k edges, the projection of mate 0 on its corner"""
    o = _o0()
    rows = [(104.0 + 0.2 + 3.6 * (j % 6) / 6.0, 64.0 + 0.2 + 3.6 * (j // 6) / 6.0, o) for j in range(k)]
    return exact(extra_left=rows, drop_own=(0,), cameras=1, **QUICK)


def _parallel(n=40):
    """every mate on parallel vertical lines with the same tangent, every edge with the same normal: a rank-deficient H"""
    locs = [(30.0 + 10.0 * (i % 14), 20.0 + 6.0 * (i // 3)) for i in range(n)]
    return exact(locs=locs, theta=math.pi / 2, **QUICK)


def cases():
    """name -> case (built on demand: the curve scenes cost a second)"""
    o = _o0()
    two_pi = 2.0 * math.pi
    C = {}
    for n in N_KF:
        C[f"n_kf_{n}"] = lambda n=n: dict(curves("euroc", n_kf=n, **QUICK), note="16-lane groups, 64-lane trees, 1 / 2 / 3 tiles")
    C["kitti_all"] = lambda: dict(curves("kitti", **QUICK), note="every mate of the scene, three tiles, the other rig")
    C["defaults"] = lambda: dict(curves("euroc", n_kf=700), note="default parameters: four rounds of ten steps")
    for a, b in ((0, None), (None, 0), (1, None), (None, 1), (1, 1), (0, 0)):
        C[f"n0_{a}_n1_{b}"] = lambda a=a, b=b: dict(curves("euroc", n_kf=300, n0=a, n1=b, **QUICK),
                                                   note="edge lists of 0 / 1 / many edges (0, 0: nothing launched, status 1)")
    C["cameras_1"] = lambda: dict(curves("euroc", n_kf=300, cameras=1, **QUICK), note="left image only: the right list is ignored")
    for cell, radius in ((1, 4.0), (4, 4.0), (15, 4.0), (4, 8.0), (1, 8.0), (3, 2.5)):
        C[f"cell_{cell}_radius_{radius}"] = lambda cell=cell, radius=radius: dict(
            curves("euroc", n_kf=400, cell_size=cell, radius=radius, **QUICK), note="cell sizes 1 / 4 / 15; sr = 1, 2, 4, 8; empty cells")
    for k in (16, 17, 33):
        C[f"segment_{k}"] = lambda k=k: dict(_segment_case(k), note="a cell segment of exactly 16 / 17 / 33 edges: full and partial passes of the 16 lanes")
    C["corner_cell"] = lambda: dict(exact(w=105, h=65, img_margin=0.0, min_terms=6, **QUICK),
                                    note="mate 0 projects into the last cell of a 105 x 65 grid (clipped walk); most other mates are outside the image")
    C["cell_boundary"] = lambda: dict(exact(extra_left=[(100.0, 64.0, o), (104.0, 68.0, o)], drop_own=(0,), **QUICK),
                                      note="projection exactly on a cell corner, edges exactly `radius` away in the neighbour cells")
    C["outside_and_nan"] = lambda: dict(exact(extra_left=[(math.nan, 64.0, o), (104.0, math.nan, o), (-0.5, 64.0, o), (250.0, 64.0, o),
                                                          (104.0, -7.0, o), (math.inf, 64.0, o), (104.5, 64.0, math.nan)], **QUICK),
                                        note="edges outside the image, with NaN / inf coordinates or a NaN orientation: never chosen")
    C["behind_camera"] = lambda: dict(exact(R0=np.diag([-1.0, 1.0, -1.0]), **QUICK),
                                      note="the pose turns every point behind the camera: projections land in the image with depth < 0, no term is live")
    C["one_camera_outside"] = lambda: dict(exact(locs=SPREAD + [(187.0, 40.0), (186.5, 80.0)], **QUICK),
                                           note="mates whose right projection (x + 4, x + 8) is outside the margin: live in the left camera only")
    C["same_normal"] = lambda: dict(exact(theta=1.25, **QUICK), note="every normal the same: the first solve hits a non-positive pivot (status 2) or takes a finite step")
    C["tie"] = lambda: dict(exact(extra_left=[(104.0, 66.0, o), (104.0, 62.0, o), (104.0, 66.0, o)], drop_own=(0,), **QUICK),
                            note="equal d2 (two edges at the same place, one mirrored): the smallest index wins")
    C["at_radius"] = lambda: dict(exact(extra_left=[(108.0, 64.0, o), (104.0, 68.25, o)], drop_own=(0,), **QUICK),
                                  note="d2 == radius^2 is accepted, the next double is not")
    C["orientation_only"] = lambda: dict(exact(extra_left=[(104.5, 64.0, o + 0.5), (106.0, 64.0, o)], drop_own=(0,), **QUICK),
                                         note="the nearest edge fails only the orientation test")
    C["orientation_wrap"] = lambda: dict(exact(extra_left=[(104.5, 64.0, o - math.copysign(two_pi - 0.05, o)),
                                                           (105.0, 64.0, o - math.copysign(math.pi - 0.05, o))], drop_own=(0,), **QUICK),
                                         note="orientation differences of almost 360 and almost 180 degrees fold onto the threshold")
    C["stop_cap"] = lambda: dict(curves("euroc", n_kf=500, rounds=2, iterations=1), note="stop reason 1: the step cap")
    C["iterations_0"] = lambda: dict(curves("euroc", n_kf=500, rounds=1, iterations=0), note="no step: the start pose with the association outputs")
    C["min_terms"] = lambda: dict(curves("euroc", n_kf=500, min_terms=5000, **QUICK), note="A < min_terms under the start pose: status 1, reason 4")
    C["few_later"] = lambda: dict(curves("kitti", n_kf=2049, rounds=3, iterations=4, min_terms=4092),
                                  note="the oracle associates 4093, 4093, 4091 terms in the three rounds: reason 4 in the third, status 0")
    C["huber_small"] = lambda: dict(curves("euroc", n_kf=500, huber_px=0.05, **QUICK), note="most terms beyond the Huber threshold")
    C["huber_inf"] = lambda: dict(curves("euroc", n_kf=500, huber_px=math.inf, **QUICK), note="least squares")
    C["far_start"] = lambda: dict(dict(curves("kitti", n_kf=900, rounds=4, iterations=10, radius=8.0, cell_size=4),
                                       **dict(zip(("R0", "t0"), asc.perturbed(asc.ps.R_GT, asc.ps.T_GT, angle=0.03, dt=(0.05, -0.04, 0.08))))),
                                  note="a start far off with a wide radius: wrong associations, the cost may rise (reason 2)")
    C["parallel"] = lambda: dict(_parallel(), note="parallel segments: reason 3 or a finite pose, whichever the oracle produces")
    return C


def run_oracle(case):
    from tests import oracle_align as oa
    return oa.align(case["kf_left"], case["kf_right"], case["edges_left"], case["edges_right"], case["img_w"], case["img_h"], case["calib"],
                    case["R0"], case["t0"], **case["params"])
