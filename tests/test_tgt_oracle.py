"""tests/oracle_tgt.py on the CPU: the restatement of build_Veridical_Quads / orientation_mapping /
Evaluate_Temporal_Edge_Pairs_on_Quads against a known motion, a hand-computed case, the zero-return rule, and the
conditions tests/test_gpu_tgt.py puts on its inputs (tests/tgt_cases.py).  Parity with the reference binary is unpinned (no
reference build here), as for the rest of the temporal path."""
import numpy as np
import pytest

from tests import oracle as orc
from tests import oracle_tgt as ot
from tests import tgt_cases as cases


@pytest.mark.parametrize("name", list(cases.HOST_CASES))
def test_inliers_of_the_known_motion_are_veridical_and_true_positive(name):
    """Every inlier quad whose keyframe mate projects inside the margin is veridical (a quad outside it cannot be, :100-105)
    and a true positive; the outliers, displaced by 5 px or more (> tp_dist = 2), are neither."""
    s, r = cases.host_scene(name), cases.host_reference(name)
    rp, n_kf = s["row_ptr"], len(s["kfL"])
    assert n_kf == cases.HOST_CASES[name][0]
    rows = np.repeat(np.arange(n_kf), np.diff(rp))
    ver = [set(r["ver_idx"][r["ver_row_ptr"][i]:r["ver_row_ptr"][i + 1]].tolist()) for i in range(n_kf)]
    inside = r["in_image"][rows].astype(bool)
    assert inside.sum() >= 0.9 * len(rows)
    for q in range(len(rows)):
        assert (q in ver[rows[q]]) == bool(s["inl"][q] and inside[q]), (name, q)
    # the quads of the scene as a stage list: inliers are true positives, displaced outliers are not
    on = ot.row_on(r["ver_row_ptr"])
    n_tp, flags, m = ot.evaluate_stage(rp, s["cfL"], s["cfR"], on, r)
    assert (flags == (s["inl"].astype(bool) & on[rows].astype(bool))).all()
    assert m["rows"] == int(on.sum()) == m["nonempty"] == m["rows_with_tp"]
    assert m["recall"] == 1.0


def _edges(xy):
    e = np.zeros(len(xy), dtype=orc.EDGE_DTYPE)
    e["x"], e["y"] = [p[0] for p in xy], [p[1] for p in xy]
    return e


def test_five_rows_by_hand():
    """projections at (10 i, 50) left and (10 i - 5, 50) right; tp_dist 2, strict.
    row 0: 2 quads, both TP                      -> recall 1, precision 1,   n 2
    row 1: 3 quads, one TP (one exactly 2 px off: not TP, one far on the right only) -> recall 1, precision 1/3, n 3
    row 2: no quads                              -> recall 0, precision 0,   n 0 (not a matched row)
    row 3: 1 quad, not TP                        -> recall 0, precision 0,   n 1
    row 4: off (no veridical quad): skipped
    recall = (1 + 1 + 0 + 0) / 4, precision = (1 + 1/3 + 0 + 0) / 3, ambiguity = (2 + 3 + 0 + 1) / 3 - 1"""
    pl = np.array([[10.0 * i, 50.0] for i in range(5)])
    pr = pl - [5.0, 0.0]
    rp = np.array([0, 2, 5, 5, 6, 8], dtype=np.int32)
    L = _edges([(0.5, 50.0), (0.0, 51.5), (10.0, 50.0), (12.0, 50.0), (10.0, 50.5), (30.0, 53.0), (40.0, 50.0), (40.0, 50.0)])
    R = _edges([(-5.0, 50.5), (-4.0, 50.0), (5.0, 50.0), (5.0, 50.0), (5.0, 53.0), (25.0, 50.0), (35.0, 50.0), (35.0, 50.0)])
    on = np.array([1, 1, 1, 1, 0], dtype=np.uint8)
    n_tp, flags = ot.evaluate_rows(rp, L, R, on, pl, pr, 2.0)
    assert n_tp.tolist() == [[2, 2], [3, 1], [0, 0], [1, 0], [0, 0]]
    assert flags.tolist() == [1, 1, 1, 0, 0, 0, 0, 0]
    m = ot.metrics(n_tp, on)
    assert (m["rows"], m["nonempty"], m["rows_with_tp"], m["sum_tp"], m["sum_n"]) == (4, 3, 2, 3, 6)
    assert m["recall"] == 2.0 / 4.0
    assert m["precision"] == ((1.0 + 1.0 / 3.0) + 0.0 + 0.0) / 3.0 == m["precision_pair"]
    assert m["ambiguity"] == 6.0 / 3.0 - 1.0


def test_zero_return_rule():
    """no rows, or no non-empty row: the four zeros of :274-278, not NaN"""
    none = ot.metrics(np.zeros((3, 2), dtype=np.int32), np.zeros(3, dtype=np.uint8))
    empty = ot.metrics(np.zeros((3, 2), dtype=np.int32), np.ones(3, dtype=np.uint8))
    assert none["rows"] == 0 and empty["rows"] == 3 and empty["nonempty"] == 0
    for m in (none, empty):
        assert [m[k] for k in ("recall", "precision", "precision_pair", "ambiguity")] == [0.0] * 4


def test_relative_pose_is_get_relative_pose():
    Rs, Rt = cases.ps.R_GT, cases.op.rot((0.1, -0.3, 1.0), 0.2)
    ts, tt = np.array([0.3, -0.1, 2.0]), np.array([-0.2, 0.4, 1.0])
    R, t = ot.relative_pose(Rs, ts, Rt, tt)
    X = np.array([0.7, -0.4, 5.0])                    # a world point seen from both cameras: X_c = R_c X + t_c
    assert np.allclose(R @ (Rs @ X + ts) + t, Rt @ X + tt, atol=1e-12)


def test_border_scenes_reach_their_borders():
    m = cases.border_reference("margin")
    assert m["in_image"].tolist() == [1, 1, 0, 0, 1, 1, 0, 1, 0, 1]         # both sides of every margin, both cameras
    c, s = cases.border_reference("cells"), cases.border_scene("cells")
    qx = (c["proj_left"][:, 0] // cases.B_CELL).astype(int)
    assert qx[0] != qx[1]                                                    # the two projections straddle a cell border
    left_only = len(s["cf"][0]) - 1
    assert left_only not in c["ver_idx"].tolist() and np.diff(c["ver_row_ptr"]).tolist() == [16, 16, 9]
    assert sorted(c["ver_idx"][:16].tolist()) != sorted(c["ver_idx"][16:32].tolist())
    o, so = cases.border_reference("orient"), cases.border_scene("orient")
    degs = (0.0, 5.0, 9.9, 10.1, 15.0, -5.0, -9.9, -10.1, 165.0, 170.1, 175.0, 180.0, 185.0, 189.9, 190.1, -175.0, 90.0)
    want = [abs(d) < 10 or abs(abs(d) - 180) < 10 for d in degs]
    n = len(degs)
    for row in range(3):
        got = set(o["ver_idx"][o["ver_row_ptr"][row]:o["ver_row_ptr"][row + 1]].tolist())
        assert [row * n + k in got for k in range(n)] == want, row
    # the third keyframe mate's orientation maps next to -pi: some accepted offsets wrap past 360 degrees
    d = np.abs(np.degrees(o["orient_left"][2] - so["cf"][0]["theta"][2 * n:3 * n]))
    assert (d > 350).any() and (d < 10).any() and ((d > 170) & (d < 190)).any()


@pytest.mark.parametrize("key", list(cases.EXPECTED))
def test_resident_input_conditions(key):
    """the poses of tests/tgt_cases.py leave rows with a veridical quad that are neither none nor all, and final quads with
    both flags"""
    got = cases.resident_counts(*key)
    assert got == cases.EXPECTED[key]
    assert 0 < got["n_rows"] < got["n_kf"] and 0 < got["n_on"] and got["final_tp"] > 0 and got["final_not_tp"] > 0
