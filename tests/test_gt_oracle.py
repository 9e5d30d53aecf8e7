"""Properties of the ground-truth restatement (tests/oracle_gt.py), the conditions the GPU tests put on their inputs, and
the argument refusals of the new bindings that need no device."""
import ctypes as C
import math

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib
from tests import gt_cases as gc
from tests import oracle_gt as og

K = [100.0, 0, 32.0, 0, 100.0, 24.0, 0, 0, 1]
R = np.eye(3)
T = [-0.5, 0.0, 0.0]


def _edges(pts):
    e = np.zeros(len(pts), dtype=_lib.EDGE_DTYPE)
    e["x"], e["y"], e["theta"] = np.array(pts, dtype=np.float64).T
    return e


def test_bilinear_quirks():
    m = np.arange(48 * 64, dtype=np.float32).reshape(48, 64)
    assert math.isnan(og.bilinear_f32(m, 10.0, 10.5)) and math.isnan(og.bilinear_f32(m, 10.5, 10.0))   # 0 / 0 weights
    assert math.isnan(og.bilinear_f32(m, -0.5, 5.5)) and math.isnan(og.bilinear_f32(m, 63.5, 5.5))     # out of bounds
    assert math.isnan(og.bilinear_f32(m, 5.5, 47.5)) and math.isnan(og.bilinear_f32(m, 5.5, -0.25))
    assert og.bilinear_f32(m, 10.5, 10.5) == (m[10, 10] + m[10, 11] + m[11, 10] + m[11, 11]) / 4
    assert og.bilinear_f32(m, 62.5, 46.5) == (m[46, 62] + m[46, 63] + m[47, 62] + m[47, 63]) / 4        # last cell is in bounds
    assert og.bilinear_f32(m, 10.25, 20.75) == pytest.approx(20.75 * 64 + 10.25, rel=1e-12)


def test_locate_skips_and_geometry():
    d = np.full((48, 64), 4.0, dtype=np.float32)
    d[30:, :] = np.nan
    d[:4, :] = np.inf
    d[20:24, :] = -1.0
    e = _edges([(20.5, 10.5, 1.0), (20.0, 10.5, 1.0), (20.5, 32.5, 1.0), (20.5, 1.5, 1.0), (20.5, 21.5, 1.0),
                (20.5, 10.5, np.deg2rad(3.9)), (20.5, 10.5, np.deg2rad(4.1)), (20.5, 10.5, np.deg2rad(177.0)),
                (20.5, 10.5, np.deg2rad(-176.5)), (20.5, 10.5, np.deg2rad(-175.9))])
    r = og.find_gt_locations(e, d, K, R, T)
    assert r["valid"].tolist() == [1, 0, 0, 0, 0, 0, 1, 0, 0, 1]
    assert r["gt_xy"][0].tolist() == [16.5, 10.5] and r["gt_xy"][1].tolist() == [-1.0, -1.0]           # GT = (x - d, y)
    G = r["gamma_left"][0]
    # rectified pair, both rays through the left inverse: depth = fx * baseline / d, and Gamma reprojects to the edge
    assert G[2] == pytest.approx(100.0 * 0.5 / 4.0, rel=1e-12)
    assert 100.0 * G[0] / G[2] + 32.0 == pytest.approx(20.5, abs=1e-9) and 100.0 * G[1] / G[2] + 24.0 == pytest.approx(10.5, abs=1e-9)
    assert r["gamma_right"][0].tolist() == [G[0] + T[0], G[1], G[2]]


def test_pool_and_tp_strictness():
    L = _edges([(30.0, 10.0, 1.0)])
    lines = np.array([[0.0, 1.0, -10.0]])                                  # y = 10
    gt = np.array([[20.0, 10.0]])
    Rr = _edges([(21.0, 10.0, 1.0), (20.5, 10.25, 1.0), (20.5, 10.5, 1.0), (19.5, 10.0, 1.0 + np.deg2rad(5.5)),
                 (19.25, 9.75, 1.0 + np.deg2rad(4.5)), (20.0, 10.0, 1.0 - 2 * math.pi)])
    p = og.gt_pool(L, Rr, lines, np.ones(1, np.uint8), gt)
    # distance exactly 1.0 is out (<), epipolar distance exactly 0.5 is out (<), 5.5 degrees is out, no wrap-around at 2 pi
    assert p["pool_idx"].tolist() == [1, 4] and p["focused"].tolist() == [1]
    n_tp = og.row_counts(np.array([0, 3]), [21.0, 20.0, 21.5], [10.0, 11.0, 10.0], np.ones(1, np.uint8), gt)
    assert n_tp.tolist() == [[3, 2]]                                       # a centre at exactly 1.0 IS a true positive (<=)
    assert og.gt_pool(L, Rr[:1], lines, np.ones(1, np.uint8), gt)["focused"].tolist() == [0]


def test_metrics_by_hand():
    n_tp = np.array([[4, 1], [0, 0], [9, 9], [2, 0], [3, 3]])
    foc = np.array([1, 1, 0, 1, 1], dtype=np.uint8)
    m = og.metrics(n_tp, foc)
    assert (m["rows"], m["nonempty"], m["rows_with_tp"], m["sum_tp"], m["sum_n"]) == (4, 3, 2, 4, 9)
    assert m["recall"] == 2 / 4 and m["precision"] == ((0.25 + 0.0) + 0.0 + 1.0) / 4
    assert m["precision_pair"] == (0.25 + 0.0 + 1.0) / 3 and m["ambiguity"] == (4.0 + 2.0 + 3.0) / 3
    f = og.metrics(n_tp, foc, drop_empty=True)
    assert f["rows"] == 3 and f["recall"] == 2 / 3 and f["precision"] == f["precision_pair"] == m["precision_pair"]
    e = og.metrics(np.zeros((2, 2), int), np.zeros(2, np.uint8))
    assert e["rows"] == 0 and all(math.isnan(e[k]) for k in ("recall", "precision", "precision_pair", "ambiguity"))
    z = og.metrics(np.zeros((2, 2), int), np.ones(2, np.uint8))
    assert z["recall"] == 0.0 and z["precision"] == 0.0 and math.isnan(z["precision_pair"]) and math.isnan(z["ambiguity"])


@pytest.mark.parametrize("name", list(gc.PAIRS))
def test_input_conditions(name):
    """What tests/test_gpu_gt.py needs of its pairs, from the oracle alone.  Found: s1-200x320 4251 focused / 293 valid
    with an empty pool / Best 1644 with, 2607 without a TP; s2-200x320 11981 / 2106 / 11979, 2; eth3d-942x489 104938 / 14537 /
    104930, 8; kitti 104018 / 13801 / 104016, 2."""
    c = gc.input_conditions(name)
    b = gc.base(name)
    assert c["n_focused"] >= 200
    assert (np.diff(b["pool"]["pool_row_ptr"]) > 0).all()                   # a non-empty pool on every focused row
    assert c["best_rows_with_tp"] >= 1 and c["best_rows_without_tp"] >= 1
    assert c["valid_with_empty_pool"] >= 1
    d = b["disp"]
    assert np.isnan(d).any() and np.isposinf(d).any() and (d < 0).any() and len(np.unique(d[np.isfinite(d)])) > 10


def test_chain_lists_end_in_oracle_chain_final():
    from tests import oracle_chain
    b = gc.base("s1-200x320")
    _, final = gc.stages("s1-200x320", False)
    ref = oracle_chain.stereo_edge_pairs(b["l"], b["r"], b["F"], None, stage1=b)
    assert (final["left_index"] == ref["left_index"]).all() and final["right"].tobytes() == ref["right"].tobytes()


def test_binding_refusals_need_no_device():
    lib = _lib.load_library()
    p = _lib.GtParams()
    lib.ebvo_gt_default_params(C.byref(p))
    assert (p.orient_gate_deg, p.pool_epi_thr, p.pool_dist, p.pool_orient_deg, p.tp_dist) == (4.0, 0.5, 1.0, 5.0, 1.0)
    cal, st = _lib.StereoCalib(), _lib.GtStage()
    d = np.zeros((4, 4), dtype=np.float32)
    assert lib.ebvo_stereo_set_gt(None, 0, _lib.ptr(d), 4, 4, 4, C.byref(cal), C.byref(p)) == _lib.EBVO_ERR_ARG
    assert lib.ebvo_stereo_gt_size(None, 0, None, None, None) == _lib.EBVO_ERR_ARG
    assert lib.ebvo_stereo_gt_fetch(None, 0, None, None, None, None, None, None) == _lib.EBVO_ERR_ARG
    assert lib.ebvo_stereo_gt_metrics(None, 0, None) == _lib.EBVO_ERR_ARG
    assert lib.ebvo_stereo_gt_stage_rows(None, 0, 0, None, 0) == _lib.EBVO_ERR_ARG
    assert lib.ebvo_gt_locate(None, None, 0, _lib.ptr(d), 4, 4, 4, C.byref(cal), C.byref(p), None, None, None, None) == _lib.EBVO_ERR_ARG
    assert lib.ebvo_gt_evaluate_rows(None, None, None, 0, None, None, 1.0, None, C.byref(st)) == _lib.EBVO_ERR_ARG
    from edge_based_visual_odometry_amd.api import Context
    with pytest.raises(TypeError):
        Context._disp(np.zeros((4, 4)))                                     # float64: not the map the reference reads
    assert Context._disp(np.zeros((4, 8), dtype=np.float32)[:, ::2]).flags["C_CONTIGUOUS"]
    assert len(_lib.GT_STAGE_NAMES) == _lib.GT_NUM_STAGES == len(og.STAGE_NAMES) and _lib.GT_STAGE_NAMES == og.STAGE_NAMES
