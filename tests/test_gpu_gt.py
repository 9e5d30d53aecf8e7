"""Ground-truth evaluation on the device (ebvo_stereo_set_gt, ebvo_stereo_gt_fetch / _metrics, ebvo_gt_locate,
ebvo_gt_evaluate_rows) against tests/oracle_gt.py, bit for bit: valid flags, GT locations, both 3-D points, the veridical
pool, the per-row (n, tp) of every stage, the integer totals and the four doubles (recall, precision, pair precision,
ambiguity) -- in both TOED modes (the `ctx` fixture), with use_sift 0 and 1.

Inputs (tests/gt_cases.py; counts found by the oracle, checked without a device in tests/test_gt_oracle.py):
  s1-200x320     4251 focused rows, 293 valid edges with an empty pool, Best: 1644 rows with a TP / 2607 without
  s2-200x320    11981 focused rows, 2106 valid edges with an empty pool, Best: 11979 / 2
  eth3d-942x489 104938 focused rows, 14537 valid edges with an empty pool, Best: 104930 / 8
  kitti         104018 focused rows, 13801 valid edges with an empty pool, Best: 104016 / 2   (the bench pair, 1241x376)
tests/test_gt_oracle.py::test_input_conditions asserts the conditions on all four.
No case is skipped at run time.
"""
import ctypes as C

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib
from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EBVO_ERR_STATE, EbvoError, ptr
from tests import gt_cases as gc
from tests import oracle_gt as og
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu

INT_KEYS = ("rows", "nonempty", "rows_with_tp", "sum_tp", "sum_n")
DBL_KEYS = ("recall", "precision", "precision_pair", "ambiguity")


def _run(ctx, b):
    ctx.stereo_upload(b["l"], b["r"])
    return ctx.stereo_run(ctx.default_params(b["F"]))


def _check_stage(got, ref, what):
    for k in INT_KEYS:
        assert got[k] == ref[k], f"{what}: {k} {got[k]} != oracle {ref[k]}"
    for k in DBL_KEYS:
        assert_bit_equal(np.array([got[k]]), np.array([ref[k]]), f"{what}: {k}")


def _check_arming(ctx, b, c, sz):
    loc, pool = b["loc"], b["pool"]
    nL = len(b["left"])
    assert c.n_left == nL
    assert sz == dict(n_valid=int(loc["valid"].sum()), n_focused=len(pool["focused_index"]), n_pool=len(pool["pool_idx"]))
    f = ctx.stereo_gt_fetch()
    fi = pool["focused_index"]
    assert_bit_equal(f["focused_index"], fi, "focused_index")
    assert_bit_equal(f["gt_xy"], loc["gt_xy"][fi], "gt_xy")
    assert_bit_equal(f["gamma_left"], loc["gamma_left"][fi], "gamma_left")
    assert_bit_equal(f["gamma_right"], loc["gamma_right"][fi], "gamma_right")
    assert_bit_equal(f["pool_row_ptr"], pool["pool_row_ptr"], "pool_row_ptr")
    assert_bit_equal(f["pool_idx"], pool["pool_idx"], "pool_idx")
    return f


@pytest.mark.parametrize("name", list(gc.PAIRS))
def test_chain_metrics_equal_oracle(ctx, name):
    b = gc.base(name)
    nL = len(b["left"])
    ev, final = gc.stages(name, False)
    # the unarmed chain first: its results are the yardstick for "arming changes nothing"
    c = _run(ctx, b)
    counts0, fin0 = ctx.stereo_finalize(b["calib"])
    with pytest.raises(EbvoError) as ei:
        ctx.stereo_gt_metrics()                                   # not armed
    assert ei.value.status == EBVO_ERR_STATE
    sz = ctx.stereo_set_gt(b["disp"], b["calib"])
    _check_arming(ctx, b, c, sz)
    m = ctx.stereo_gt_metrics()
    assert [s["name"] for s in m] == list(og.STAGE_NAMES)
    # armed after the finalisation: only the stages of the run are present
    assert [s["present"] for s in m] == [k in (og.EPIPOLAR, og.DISPARITY, og.ORIENTATION, og.NCC) for k in range(12)]
    for k in (og.EPIPOLAR, og.DISPARITY, og.ORIENTATION, og.NCC):
        _check_stage(m[k], ev[k][1], f"{name} stage {k} after arming")
        assert_bit_equal(ctx.stereo_gt_stage_rows(k, nL), ev[k][0], f"{name} rows of stage {k}")
    # the census' third count is the row length of the resident CSR on every focused row
    o = ctx.stereo_fetch(c)
    foc = b["pool"]["focused"].astype(bool)
    assert (ctx.stereo_gt_stage_rows(og.ORIENTATION, nL)[foc, 0] == np.diff(o["row_ptr"])[foc]).all()
    # the armed chain: same final pairs and counts, byte for byte, and every later stage evaluated
    counts1, fin1 = ctx.stereo_finalize(b["calib"])
    assert counts1 == counts0
    for k in ("left_index", "right", "score", "rows"):
        assert fin1[k].tobytes() == fin0[k].tobytes(), k
    assert_bit_equal(fin1["left_index"], final["left_index"], "final left_index vs oracle")
    m = ctx.stereo_gt_metrics()
    for k in range(12):
        assert m[k]["present"] == (k not in (og.SIFT, og.BNB_SIFT)), k
        if m[k]["present"]:
            _check_stage(m[k], ev[k][1], f"{name} stage {k}")
            src = og.BEST if k == og.FINAL else k
            assert_bit_equal(ctx.stereo_gt_stage_rows(k, nL), ev[src][0], f"{name} rows of stage {k}")
    with pytest.raises(EbvoError) as ei:
        ctx.stereo_gt_stage_rows(og.SIFT, nL)                     # absent, not zero
    assert ei.value.status == EBVO_ERR_STATE


@pytest.mark.parametrize("name", gc.SIFT_PAIRS)
def test_chain_metrics_with_sift(ctx, name):
    b = gc.base(name)
    nL = len(b["left"])
    ev, final = gc.stages(name, True)
    _run(ctx, b)
    counts0, fin0 = ctx.stereo_finalize(b["calib"], use_sift=True)
    _run(ctx, b)                                                 # a new run disarms; arm BEFORE the chain this time
    ctx.stereo_set_gt(b["disp"], b["calib"])
    counts1, fin1 = ctx.stereo_finalize(b["calib"], use_sift=True)
    assert counts1 == counts0
    for k in ("left_index", "right", "score", "rows"):
        assert fin1[k].tobytes() == fin0[k].tobytes(), k
    m = ctx.stereo_gt_metrics()
    assert all(s["present"] for s in m)
    for k in range(12):
        _check_stage(m[k], ev[k][1], f"{name} sift stage {k}")
        src = og.BEST if k == og.FINAL else k
        assert_bit_equal(ctx.stereo_gt_stage_rows(k, nL), ev[src][0], f"{name} rows of stage {k}")
    # a chain without SIFT on the same armed slot: the SIFT stages are absent again, NCC is the run's keep
    ev0, _ = gc.stages(name, False)
    ctx.stereo_finalize(b["calib"], use_sift=False)
    m = ctx.stereo_gt_metrics()
    assert not m[og.SIFT]["present"] and not m[og.BNB_SIFT]["present"]
    _check_stage(m[og.NCC], ev0[og.NCC][1], "NCC without sift")
    _check_stage(m[og.FINAL], ev0[og.FINAL][1], "Final without sift")


def test_evaluate_rows_equals_resident(ctx):
    """ebvo_gt_evaluate_rows on the fetched stage lists = what the armed chain stored."""
    name = "s2-200x320"
    b = gc.base(name)
    nL = len(b["left"])
    c = _run(ctx, b)
    ctx.stereo_set_gt(b["disp"], b["calib"])
    counts, fin = ctx.stereo_finalize(b["calib"])
    m = ctx.stereo_gt_metrics()
    res_ncc, res_best = ctx.stereo_gt_stage_rows(og.NCC, nL), ctx.stereo_gt_stage_rows(og.BEST, nL)
    o = ctx.stereo_fetch(c)
    foc, gt_xy = b["pool"]["focused"], b["loc"]["gt_xy"]
    keep = o["keep"].astype(bool)
    from tests import oracle_chain as oc
    rp = oc.filter_rows(o["row_ptr"], keep)
    n_tp, st = ctx.gt_evaluate_rows(rp, o["right"][o["col_idx"][keep]], foc, gt_xy)
    assert_bit_equal(n_tp, res_ncc, "NCC rows")
    for k in INT_KEYS + DBL_KEYS:
        assert_bit_equal(np.array([st[k]]), np.array([m[og.NCC][k]]), k)
    rp = np.concatenate([[0], np.cumsum(np.bincount(fin["left_index"], minlength=nL))]).astype(np.int32)
    n_tp, st = ctx.gt_evaluate_rows(rp, fin["right"], foc, gt_xy)
    assert_bit_equal(n_tp, res_best, "Best rows")
    for k in INT_KEYS + DBL_KEYS:
        assert_bit_equal(np.array([st[k]]), np.array([m[og.BEST][k]]), k)
    # the host-array calls leave slot 0's pair, results and armed state alone
    ctx.gt_locate(b["left"][:50], b["disp"], b["calib"])
    assert ctx.stereo_gt_metrics() == m
    assert_bit_equal(ctx.stereo_gt_stage_rows(og.BEST, nL), res_best, "Best rows after the host calls")
    assert ctx.stereo_fetch(c)["keep"].tobytes() == o["keep"].tobytes()
    with pytest.raises(EbvoError) as ei:
        ctx.stereo_gt_stage_rows(og.BEST, nL - 1)                 # an array too short for the slot: refused, not overrun
    assert ei.value.status == _lib.EBVO_ERR_CAPACITY
    # no rows at all / no non-empty row: the expression's NaN, reported, not trapped
    n_tp, st = ctx.gt_evaluate_rows(np.zeros(4, np.int32), fin["right"][:0], np.zeros(3, np.uint8), np.zeros((3, 2)))
    assert st["rows"] == 0 and all(np.isnan(st[k]) for k in DBL_KEYS)
    n_tp, st = ctx.gt_evaluate_rows(np.zeros(4, np.int32), fin["right"][:0], np.ones(3, np.uint8), np.zeros((3, 2)))
    assert st["rows"] == 3 and st["recall"] == 0.0 and st["precision"] == 0.0 and np.isnan(st["precision_pair"])


def test_locate_handmade_edges(ctx):
    """Integer, border and out-of-bounds coordinates and the three orientation gates through ebvo_gt_locate."""
    h, w = 40, 60
    disp = og.disparity_map(h, w, 5)
    disp[:, :8] = (5.0 + 0.01 * np.arange(h)[:, None] * np.arange(8)[None, :]).astype(np.float32)
    calib = gc.calib_of("kitti")
    pts = [(10.5, 10.5, 0.5), (10.0, 10.5, 0.5), (10.5, 10.0, 0.5), (0.5, 0.5, 1.0), (-0.5, 5.5, 1.0), (w - 0.5, 5.5, 1.0),
           (w - 1.5, h - 1.5, 1.0), (5.5, h - 0.5, 1.0), (3.25, 7.75, -1.2), (30.5, 13.5, 1.0), (8.5, 20.5, 1.0),
           (20.5, 27.5, 1.0), (12.5, 5.5, np.deg2rad(3.9)), (12.5, 5.5, np.deg2rad(4.1)), (12.5, 5.5, np.deg2rad(176.5)),
           (12.5, 5.5, np.deg2rad(-177.0)), (12.5, 5.5, np.deg2rad(-175.5)), (40.3, 18.6, 2.0), (1e9, 5.5, 1.0)]
    e = np.zeros(len(pts), dtype=_lib.EDGE_DTYPE)
    e["x"], e["y"], e["theta"] = np.array(pts).T
    ref = og.find_gt_locations(e, disp, calib[0], calib[2], calib[3])
    assert 0 < ref["valid"].sum() < len(pts)
    for view in (disp, np.ascontiguousarray(np.pad(disp, ((0, 0), (0, 7))))[:, :w]):   # tight and strided map
        got = ctx.gt_locate(e, view, calib)
        assert_bit_equal(got["valid"], ref["valid"], "valid")
        for k in ("gt_xy", "gamma_left", "gamma_right"):
            assert_bit_equal(got[k], ref[k], k)


def test_arming_state_and_arguments(ctx):
    b = gc.base("s1-200x320")
    lib, cal, p = ctx.lib, ctx._calib(b["calib"]), ctx.gt_params()
    disp = b["disp"]
    h, w = disp.shape

    def arm(d=disp, hh=h, ww=w, stride=w, params=p):
        return lib.ebvo_stereo_set_gt(ctx._ctx, 0, ptr(d), hh, ww, stride, C.byref(cal), C.byref(params))

    ctx.stereo_upload(b["l"], b["r"])
    assert arm() == EBVO_ERR_STATE                                # before a run
    c = _run(ctx, b)
    before = ctx.stereo_fetch(c)
    assert arm(hh=h - 1) == EBVO_ERR_ARG and arm(ww=w + 1) == EBVO_ERR_ARG and arm(stride=w - 1) == EBVO_ERR_ARG
    assert lib.ebvo_stereo_set_gt(ctx._ctx, 0, None, h, w, w, C.byref(cal), C.byref(p)) == EBVO_ERR_ARG
    assert lib.ebvo_stereo_set_gt(ctx._ctx, 0, ptr(disp), h, w, w, None, C.byref(p)) == EBVO_ERR_ARG
    assert lib.ebvo_stereo_set_gt(ctx._ctx, 99, ptr(disp), h, w, w, C.byref(cal), C.byref(p)) == EBVO_ERR_ARG
    for field in ("orient_gate_deg", "pool_epi_thr", "pool_dist", "pool_orient_deg", "tp_dist"):
        for bad in (float("nan"), -0.5):
            assert arm(params=ctx.gt_params(**{field: bad})) == EBVO_ERR_ARG, (field, bad)
    after = ctx.stereo_fetch(c)                                   # the slot's results are intact, and it is not armed
    for k in ("row_ptr", "col_idx", "best", "keep"):
        assert before[k].tobytes() == after[k].tobytes(), k
    with pytest.raises(EbvoError):
        ctx.stereo_gt_size()
    assert arm() == 0
    sz = ctx.stereo_gt_size()
    assert sz["n_focused"] == len(b["pool"]["focused_index"])
    assert arm(params=ctx.gt_params(tp_dist=-1.0)) == EBVO_ERR_ARG and ctx.stereo_gt_size() == sz   # a refused call keeps it armed
    ctx.stereo_upload(b["l"], b["r"])                            # a re-upload disarms
    with pytest.raises(EbvoError) as ei:
        ctx.stereo_gt_size()
    assert ei.value.status == EBVO_ERR_STATE
    _run(ctx, b)
    with pytest.raises(EbvoError):
        ctx.stereo_gt_metrics()                                   # ... and a run does not re-arm
    # the developer key is range-checked
    with pytest.raises(EbvoError) as ei:
        ctx.debug_set(21, 65537)
    assert ei.value.status == EBVO_ERR_ARG
    with pytest.raises(EbvoError) as ei:
        ctx.debug_set(24, 1)                                      # the first key that does not exist (22 / 23 cap the chains' grids)
    assert ei.value.status == EBVO_ERR_ARG


def test_context_destroy_and_recreate_with_gt_buffers():
    from edge_based_visual_odometry_amd.api import Context
    b = gc.base("s1-200x320")
    for _ in range(2):
        with Context(256, 384, device=0) as c2:
            c2.set_slots(2)
            c2.stereo_upload(b["l"], b["r"], slot=1)
            c2.stereo_submit(c2.default_params(b["F"]), slot=1)
            c2.stereo_wait(slot=1)
            sz = c2.stereo_set_gt(b["disp"], b["calib"], slot=1)
            assert sz["n_focused"] == len(b["pool"]["focused_index"])
            with pytest.raises(EbvoError):
                c2.stereo_gt_size(slot=0)                        # arming is per slot


@pytest.mark.parametrize("blocks", [1, 7, 300])
def test_launch_grid_independence(ctx, blocks):
    name = "s1-200x320"
    b = gc.base(name)
    nL = len(b["left"])
    ev, _ = gc.stages(name, False)
    ctx.debug_set(21, blocks)
    try:
        c = _run(ctx, b)
        sz = ctx.stereo_set_gt(b["disp"], b["calib"])
        _check_arming(ctx, b, c, sz)
        ctx.stereo_finalize(b["calib"])
        m = ctx.stereo_gt_metrics()
        for k in range(12):
            if m[k]["present"]:
                _check_stage(m[k], ev[k][1], f"grid {blocks} stage {k}")
                assert_bit_equal(ctx.stereo_gt_stage_rows(k, nL), ev[og.BEST if k == og.FINAL else k][0], f"rows {k}")
    finally:
        ctx.debug_set(21, 0)


def test_chain_without_pairs(ctx):
    """max_disp = 0: the run forms no candidate pair, the pool (which ignores max_disp) still focuses rows.  Every stage of
    the armed chain from the disparity filter on then holds empty lists: rows = the focused rows, nothing else, and 0 / 0
    where the expression divides by the non-empty rows."""
    from tests import oracle as orc
    b = gc.base("s1-200x320")
    nL = len(b["left"])
    foc = b["pool"]["focused"]
    params = ctx.default_params(b["F"])
    params.max_disp = 0.0
    rp, ci = orc.epi_candidates(b["left"], b["right"], b["lines"], 0.5, 0.0, 10.0, stage_mask=1)
    epi = og.metrics(og.row_counts(rp, b["right"]["x"][ci], b["right"]["y"][ci], foc, b["loc"]["gt_xy"]), foc)
    empty = og.metrics(np.zeros((nL, 2), np.int32), foc)
    empty_final = og.metrics(np.zeros((nL, 2), np.int32), foc, drop_empty=True)
    assert epi["sum_n"] > 0 and empty["rows"] == int(foc.sum()) > 0 and empty_final["rows"] == 0
    for use_sift in (False, True):
        ctx.stereo_upload(b["l"], b["r"])
        c = ctx.stereo_run(params)
        assert c.n_pairs == 0 and c.n_left == nL
        sz = ctx.stereo_set_gt(b["disp"], b["calib"])
        assert sz["n_focused"] == empty["rows"]
        counts, fin = ctx.stereo_finalize(b["calib"], use_sift=use_sift)
        assert counts["n_final"] == 0
        m = ctx.stereo_gt_metrics()
        for k in range(12):
            assert m[k]["present"] == (use_sift or k not in (og.SIFT, og.BNB_SIFT)), k
            if m[k]["present"]:
                ref = epi if k == og.EPIPOLAR else empty_final if k == og.FINAL else empty
                _check_stage(m[k], ref, f"stage {k} of a chain without pairs")
        assert m[og.BEST]["recall"] == 0.0 and np.isnan(m[og.BEST]["ambiguity"]) and np.isnan(m[og.FINAL]["recall"])


def test_two_armed_slots_in_flight(ctx):
    """The enqueue-only path a frame loop uses: two slots armed, both finalisation chains submitted before either is waited
    for; each slot reports its own pair's metrics."""
    names = ("s1-200x320", "s2-200x320")
    ctx.set_slots(2)
    for slot, name in enumerate(names):
        b = gc.base(name)
        ctx.stereo_upload(b["l"], b["r"], slot=slot)
        ctx.stereo_submit(ctx.default_params(b["F"]), slot=slot)
    for slot, name in enumerate(names):
        ctx.stereo_wait(slot=slot)
        ctx.stereo_set_gt(gc.base(name)["disp"], gc.base(name)["calib"], slot=slot)
    for slot, name in enumerate(names):
        ctx.stereo_finalize_submit(gc.base(name)["calib"], slot=slot, use_sift=bool(slot))
    with pytest.raises(EbvoError) as ei:
        ctx.stereo_gt_metrics(slot=0)                             # its chain is in flight
    assert ei.value.status == EBVO_ERR_STATE
    for slot, name in reversed(list(enumerate(names))):
        ctx.stereo_finalize_wait(slot=slot)
    for slot, name in enumerate(names):
        ev, _ = gc.stages(name, bool(slot))
        nL = len(gc.base(name)["left"])
        m = ctx.stereo_gt_metrics(slot=slot)
        for k in range(12):
            assert m[k]["present"] == (bool(slot) or k not in (og.SIFT, og.BNB_SIFT)), (slot, k)
            if m[k]["present"]:
                _check_stage(m[k], ev[k][1], f"slot {slot} stage {k}")
                assert_bit_equal(ctx.stereo_gt_stage_rows(k, nL, slot=slot), ev[og.BEST if k == og.FINAL else k][0], f"slot {slot} rows {k}")
