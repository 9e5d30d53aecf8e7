"""Stereo ground truth on the device off the beaten path (gt_kernels.hip; ebvo_stereo_set_gt, ebvo_stereo_gt_*, ebvo_gt_locate,
ebvo_gt_evaluate_rows) against tests/oracle_gt.py, bit for bit, in both TOED modes: sizes, focused_index, gt_xy, both 3-D
points, pool_row_ptr, pool_idx, the per-row (n, tp) of every present stage, the five integers and the four doubles.  Where
a case finalises, the armed chain's final pairs equal the unarmed chain's byte for byte.

Cases (tests/gt_edge_cases.py; every pair is synth.stereo_pair("s2", h, w), 120x200 unless named otherwise: 5125 left and
5117 right edges, 4433 valid at the default gate).  Counts found by the oracle; tests/test_gt_edge_cases.py asserts the
conditions without a device:
  default        3620 focused, 7590 pool entries, longest pool row 6 over 5 chunks; Best 3620 rows, all with a TP
  wide_pool      pool (8, 12, 400): 4412 focused, 401166 pool entries, longest row 150 over 52 chunks, 3 groups of 512
  mid_pool       pool (3, 8, 30), run (2.0, 40, 30), tp_dist 2.5: 4162 focused, longest pool row 34, longest epipolar
                 row 273; Best 4070 rows with a TP of 4140 non-empty (22 empty)
  short_reach    run max_disp 11.5 < the 12-px disparity: disparity stage 136 empty / 2143 without / 1341 with a TP,
                 orientation 1781 / 1019 / 820, NCC 2202 / 599 / 819, Best 2327 / 263 / 1030
  slant          the slanted calibration at defaults: 952 focused of 4433 valid, GT up to 4.34 px off its line
  slant_wide     run epi_thr 2.0, pool (2, 2, 5): 2731 focused; Best 1618 rows with a TP of 2644 non-empty, recall 0.592
  zero_disp      a patch of d = 0 on the Kitti calibration: 108 valid edges with gt_x == x; K^-1's last entry is
                 1 - 2^-53 there, the denominator an ulp and the 3-D points finite (|z| > 1e12)
  zero_disp_exact  the same map with K = (512, 512, 64, 32): the denominator is exactly 0, the points infinite / NaN
  <param>=<v>    one ground-truth parameter at a time: gate 0 / 45 / inf -> 4639 / 2231 / 0 valid; pool_epi_thr 0, pool_dist 0,
                 pool_orient_deg 0 -> 4433 valid, 0 focused; pool_dist inf -> 4144 focused, longest row 26; tp_dist inf -> tp == n
  mask1 .. mask7 37x101, 337 and 352 edges, 103 focused: a dense first list of 352 without bit 1, longest row 231 at mask 2
  size-33x65, size-37x101   38 and 103 focused rows; also in a context sized exactly to the image
No case is skipped at run time.
"""
import functools

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib
from edge_based_visual_odometry_amd._lib import EBVO_ERR_STATE, EbvoError
from edge_based_visual_odometry_amd.api import Context
from tests import gt_edge_cases as ge
from tests import oracle_gt as og
from tests.test_gpu_gt import DBL_KEYS, _check_arming, _check_stage
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu

CHAIN_STAGES = tuple(k for k in range(12) if k not in (og.SIFT, og.BNB_SIFT))
NO_ROWS = og.metrics(np.zeros((0, 2), np.int32), np.zeros(0, np.uint8))       # rows 0 and 0 / 0 four times


def _run(ctx, b):
    ctx.stereo_upload(b["l"], b["r"])
    p = ctx.default_params(b["F"])
    for k in ("epi_thr", "max_disp", "orient_thr_deg"):
        setattr(p, k, b["run"][k])
    p.stage_mask = b["run"]["stage_mask"]
    return ctx.stereo_run(p)


def _check_stages(ctx, b, stages, what):
    """metrics and per-row counts of exactly `stages`; every other stage is absent"""
    nL = len(b["left"])
    m = ctx.stereo_gt_metrics()
    assert [s["present"] for s in m] == [k in stages for k in range(12)], what
    for k in stages:
        _check_stage(m[k], b["ev"][k][1], f"{what} stage {k}")
        src = og.BEST if k == og.FINAL else k
        assert_bit_equal(ctx.stereo_gt_stage_rows(k, nL), b["ev"][src][0], f"{what} rows of stage {k}")
    return m


def _check_case(ctx, name, what=None):
    """run, (finalise unarmed,) arm, compare everything with the oracle, (finalise armed and compare again)"""
    what = what or name
    b = ge.case(name)
    nL = len(b["left"])
    c = _run(ctx, b)
    if b["finalize"]:
        counts0, fin0 = ctx.stereo_finalize(b["calib"])
    sz = ctx.stereo_set_gt(b["disp"], b["calib"], **b["gt"])
    _check_arming(ctx, b, c, sz)
    _check_stages(ctx, b, ge.RUN_STAGES, f"{what} after arming")
    # the census' third count is the row length of the resident CSR on every focused row
    o = ctx.stereo_fetch(c)
    assert_bit_equal(o["row_ptr"], b["row_ptr"], f"{what} row_ptr")
    foc = b["pool"]["focused"].astype(bool)
    assert (ctx.stereo_gt_stage_rows(og.ORIENTATION, nL)[foc, 0] == np.diff(o["row_ptr"])[foc]).all()
    if b["finalize"]:
        counts1, fin1 = ctx.stereo_finalize(b["calib"])
        assert counts1 == counts0
        for k in ("left_index", "right", "score", "rows"):
            assert fin1[k].tobytes() == fin0[k].tobytes(), (what, k)
        assert_bit_equal(fin1["left_index"], b["final"]["left_index"], f"{what} final left_index vs oracle")
        _check_stages(ctx, b, CHAIN_STAGES, what)
    return c


@pytest.mark.parametrize("name", list(ge.CASES))
def test_case_equals_oracle(ctx, name):
    _check_case(ctx, name)


@pytest.mark.parametrize("blocks", [1, 7, 300])
def test_wide_pool_launch_grid(ctx, blocks):
    ctx.debug_set(21, blocks)
    try:
        _check_case(ctx, "wide_pool", f"wide_pool on {blocks} blocks")
    finally:
        ctx.debug_set(21, 0)


@pytest.mark.parametrize("mode", ["strict", "hybrid"])
@pytest.mark.parametrize("name", ge.SIZE_CASES)
def test_context_sized_exactly_to_the_image(name, mode):
    with Context(*ge.CASES[name]["shape"], device=0, toed_mode=mode) as c:
        _check_case(c, name)
        _check_case(c, name)                                     # the second arming of a slot allocates nothing


# --- slot state --------------------------------------------------------------------------------------------------------
def test_rearming_and_size_change_on_one_slot(ctx):
    wide, dflt, small = ge.case("wide_pool"), ge.case("default"), ge.case("mask7")
    nL = len(dflt["left"])
    c = _run(ctx, wide)
    sz = ctx.stereo_set_gt(wide["disp"], wide["calib"], **wide["gt"])
    f = _check_arming(ctx, wide, c, sz)
    assert len(f["pool_idx"]) > 50 * len(dflt["pool"]["pool_idx"])
    # the same slot with the defaults: nothing of the larger pool survives
    sz = ctx.stereo_set_gt(dflt["disp"], dflt["calib"])
    _check_arming(ctx, dflt, c, sz)
    _check_stages(ctx, dflt, ge.RUN_STAGES, "re-armed with defaults")
    ctx.stereo_finalize(dflt["calib"])
    _check_stages(ctx, dflt, CHAIN_STAGES, "re-armed and finalised")
    # arming again forgets the chain's stages
    sz = ctx.stereo_set_gt(dflt["disp"], dflt["calib"])
    _check_arming(ctx, dflt, c, sz)
    _check_stages(ctx, dflt, ge.RUN_STAGES, "armed a third time")
    with pytest.raises(EbvoError) as ei:
        ctx.stereo_gt_stage_rows(og.BEST, nL)
    assert ei.value.status == EBVO_ERR_STATE
    # a pair of another size on the same slot: every array has the new n_left
    c = _run(ctx, small)
    with pytest.raises(EbvoError) as ei:
        ctx.stereo_gt_size()                                      # the new run disarmed the slot
    assert ei.value.status == EBVO_ERR_STATE
    assert c.n_left == len(small["left"]) < nL
    sz = ctx.stereo_set_gt(small["disp"], small["calib"])
    _check_arming(ctx, small, c, sz)
    _check_stages(ctx, small, ge.RUN_STAGES, "after the size change")
    with pytest.raises(EbvoError) as ei:
        ctx.stereo_set_gt(dflt["disp"], dflt["calib"])            # the earlier pair's map no longer fits
    assert ei.value.status == _lib.EBVO_ERR_ARG
    ctx.stereo_finalize(small["calib"])
    _check_stages(ctx, small, CHAIN_STAGES, "finalised after the size change")


def _check_nothing_to_evaluate(ctx, calib, what):
    """no focused row: every stage of the chain reports no rows and 0 / 0"""
    for stages in (ge.RUN_STAGES, CHAIN_STAGES):
        m = ctx.stereo_gt_metrics()
        assert [s["present"] for s in m] == [k in stages for k in range(12)], what
        for k in stages:
            _check_stage(m[k], NO_ROWS, f"{what} stage {k}")
            assert m[k]["rows"] == 0 and all(np.isnan(m[k][d]) for d in DBL_KEYS)
        if stages is ge.RUN_STAGES:
            counts, fin = ctx.stereo_finalize(calib)
    return counts, fin


def test_no_left_edges(ctx):
    b = ge.case("default")
    ctx.stereo_upload(np.full_like(b["l"], 90), b["r"])
    c = ctx.stereo_run(ctx.default_params(b["F"]))
    assert c.n_left == 0 and c.n_right == len(b["right"])
    assert ctx.stereo_set_gt(b["disp"], b["calib"]) == dict(n_valid=0, n_focused=0, n_pool=0)
    f = ctx.stereo_gt_fetch()
    assert f["pool_row_ptr"].tolist() == [0]
    for k in ("focused_index", "gt_xy", "gamma_left", "gamma_right", "pool_idx"):
        assert len(f[k]) == 0, k
    counts, fin = _check_nothing_to_evaluate(ctx, b["calib"], "no left edges")
    assert counts["n_final"] == 0 and len(fin["left_index"]) == 0


def test_no_right_edges(ctx):
    b = ge.case("default")
    nL = len(b["left"])
    ctx.stereo_upload(b["l"], np.full_like(b["r"], 90))
    c = ctx.stereo_run(ctx.default_params(b["F"]))
    assert c.n_left == nL and c.n_right == 0 and c.n_pairs == 0
    empty = og.gt_pool(b["left"], b["right"][:0], b["lines"], b["loc"]["valid"], b["loc"]["gt_xy"])
    sz = ctx.stereo_set_gt(b["disp"], b["calib"])
    assert sz["n_valid"] == int(b["loc"]["valid"].sum()) > 0 and sz["n_focused"] == 0 and sz["n_pool"] == 0
    _check_arming(ctx, dict(left=b["left"], loc=b["loc"], pool=empty), c, sz)
    for k in ge.RUN_STAGES:
        assert not ctx.stereo_gt_stage_rows(k, nL).any(), k
    counts, fin = _check_nothing_to_evaluate(ctx, b["calib"], "no right edges")
    assert counts["n_final"] == 0


def test_no_focused_row(ctx):
    name = "pool_dist=0"
    b = ge.case(name)
    c = _check_case(ctx, name)
    assert ctx.stereo_gt_size()["n_valid"] > 0 and c.n_pairs > 0
    counts, fin = _check_nothing_to_evaluate(ctx, b["calib"], "no focused row")
    assert counts["n_final"] > 0                                  # the chain itself is not affected
    for k in CHAIN_STAGES:
        assert not ctx.stereo_gt_stage_rows(k, len(b["left"])).any(), k


# --- ebvo_gt_evaluate_rows on handmade lists -----------------------------------------------------------------------------
ROW_LENGTHS = (0, 1, 7, 8, 9, 63, 64, 65)
BEYOND_ONE = float(np.nextafter(1.0, 2.0))
OFFSETS = np.array([(0.0, 0.0), (1.0, 0.0), (0.0, -1.0), (BEYOND_ONE, 0.0), (0.0, BEYOND_ONE), (0.6, 0.8), (0.5, 0.5),
                    (0.75, -0.75), (3.0, 4.0), (np.nan, 0.0), (0.0, np.inf), (-np.inf, 2.0), (2.0 ** -30, 0.0)])


def _handmade_rows(nL):
    """A CSR list whose rows mix all the lengths within one wave (eight rows), with one of 1000 every 61 rows and in the
    first wave.  GT points have integer coordinates, (0, 0) on every fourth row, so that gt + 1 and gt + nextafter(1) are
    exact there; a fifth of the rows are not focused and keep their lists."""
    rng = np.random.default_rng(1000 + nL)
    lens = rng.choice(ROW_LENGTHS, nL)
    lens[:12] = (1000, 0, 1, 7, 8, 9, 63, 64, 65, 7, 64, 9)[:nL]
    lens[3 + 61::61] = 1000
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    gt = rng.integers(1, 200, (nL, 2)).astype(np.float64)
    gt[::4] = 0.0
    focused = (rng.random(nL) < 0.8).astype(np.uint8)
    focused[:min(nL, 9)] = 1
    if nL > 12:
        focused[9:12] = 0                                         # non-empty lists on rows that are not focused
    row = np.repeat(np.arange(nL), lens)
    off = OFFSETS[rng.integers(0, len(OFFSETS), len(row))]
    cand = np.zeros(len(row), dtype=_lib.EDGE_DTYPE)
    cand["x"], cand["y"] = gt[row, 0] + off[:, 0], gt[row, 1] + off[:, 1]
    cand["theta"] = rng.uniform(-3, 3, len(row))
    return rp, cand, focused, gt, row


@pytest.mark.parametrize("nL", [1, 31, 32, 33, 4095, 4096, 4097, 8193])
def test_evaluate_rows_handmade(ctx, nL):
    rp, cand, focused, gt, row = _handmade_rows(nL)
    with np.errstate(invalid="ignore"):
        dist = np.sqrt((cand["x"] - gt[row, 0]) ** 2 + (cand["y"] - gt[row, 1]) ** 2)[focused[row] != 0]
    # the inputs hold what the test is about: candidates on the GT point, at exactly tp_dist, one ulp beyond, NaN and inf
    assert (dist == 0.0).any() and (dist == 1.0).any() and (dist == BEYOND_ONE).any() and np.isnan(dist).any() and np.isinf(dist).any()
    if nL > 12:
        assert (np.diff(rp)[focused == 0] > 0).any()              # an unfocused row with a non-empty list
    refs = {}
    for tp_dist in (0.0, 1.0, float("inf")):
        n_tp = og.row_counts(rp, cand["x"], cand["y"], focused, gt, tp_dist)
        refs[tp_dist] = (n_tp, og.metrics(n_tp, focused))
    assert refs[0.0][1]["sum_tp"] < refs[1.0][1]["sum_tp"] < refs[float("inf")][1]["sum_tp"] < refs[1.0][1]["sum_n"]
    for blocks in (0, 1):                                         # 1: one block makes every pass
        ctx.debug_set(21, blocks)
        try:
            for tp_dist, (ref_rows, ref) in refs.items():
                got_rows, got = ctx.gt_evaluate_rows(rp, cand, focused, gt, tp_dist)   # raises if the totals and the rows disagree
                what = f"{nL} rows, tp_dist {tp_dist}, key 21 = {blocks}"
                assert_bit_equal(got_rows, ref_rows, what)
                assert not got_rows[focused == 0].any(), what
                _check_stage(got, ref, what)
        finally:
            ctx.debug_set(21, 0)


# --- ebvo_gt_locate beyond a handful of points ---------------------------------------------------------------------------
H, W = 120, 200
N_LOCATE = 70001
SPECIAL = [(10.5, 10.5), (10.0, 10.5), (10.5, 10.0), (10.0, 10.0), (0.5, 0.5), (0.0, 0.0), (-0.5, 5.5), (W - 0.5, 5.5), (W - 1.0, 5.5),
           (W - 1.5, H - 1.5), (5.5, H - 0.5), (5.5, H - 1.0), (np.nan, 5.5), (5.5, np.nan), (np.inf, 5.5), (5.5, np.inf),
           (-np.inf, 5.5), (5.5, -np.inf), (1e9, 5.5), (5.5, 1e9), (-1e9, -1e9), (np.nan, np.nan)]


@functools.lru_cache(maxsize=None)
def _locate_edges():
    rng = np.random.default_rng(21)
    e = np.zeros(N_LOCATE, dtype=_lib.EDGE_DTYPE)
    e["x"], e["y"] = rng.uniform(-6.0, W + 6.0, N_LOCATE), rng.uniform(-6.0, H + 6.0, N_LOCATE)
    e["theta"] = rng.uniform(-np.pi, np.pi, N_LOCATE)
    e["x"][0], e["y"][0], e["theta"][0] = 150.25, 30.75, 1.0       # n = 1: a valid edge in the ramp region
    sp = np.array(SPECIAL)
    e["x"][1:1 + len(sp)], e["y"][1:1 + len(sp)] = sp[:, 0], sp[:, 1]
    k = 1 + len(sp)
    e["x"][k:k + 60] = np.round(e["x"][k:k + 60])                 # integer x, integer y, both
    e["y"][k + 40:k + 100] = np.round(e["y"][k + 40:k + 100])
    return e


_LOCATE_REF = {}


def _locate_ref(geom, zero_patch, gate, n):
    """the oracle on the first n edges (per-edge work: a prefix of a longer result is the result of the prefix)"""
    key = (geom, zero_patch, gate)
    if key not in _LOCATE_REF or len(_LOCATE_REF[key]["valid"]) < n:
        calib = ge.geometry(geom)[1]
        _LOCATE_REF[key] = og.find_gt_locations(_locate_edges()[:n], ge.disparity((H, W), zero_patch), calib[0], calib[2], calib[3], gate)
    return {k: v[:n] for k, v in _LOCATE_REF[key].items()}


def _check_locate(ctx, disp, geom, zero_patch, gate, n, what):
    ref = _locate_ref(geom, zero_patch, gate, n)
    got = ctx.gt_locate(_locate_edges()[:n], disp, ge.geometry(geom)[1], orient_gate_deg=gate)
    assert_bit_equal(got["valid"], ref["valid"], f"{what}: valid")
    for k in ("gt_xy", "gamma_left", "gamma_right"):
        assert_bit_equal(got[k], ref[k], f"{what}: {k}")
    return ref


@pytest.mark.parametrize("n", [N_LOCATE, 1, 255, 256, 257])
def test_locate_sizes_and_grids(ctx, n):
    disp = ge.disparity((H, W))
    for blocks in (0, 1):
        ctx.debug_set(21, blocks)
        try:
            ref = _check_locate(ctx, disp, "kitti", False, 4.0, n, f"n {n}, key 21 = {blocks}")
        finally:
            ctx.debug_set(21, 0)
    assert ref["valid"][0] == 1
    if n >= 255:
        assert 0 < ref["valid"].sum() < n and not ref["valid"][1:1 + len(SPECIAL)][-10:].any()


def test_locate_gates_maps_and_calibrations(ctx):
    n = 2049
    disp, zero = ge.disparity((H, W)), ge.disparity((H, W), True)
    counts = {}
    for gate in (0.0, 45.0, float("inf")):
        counts[gate] = int(_check_locate(ctx, disp, "kitti", False, gate, n, f"gate {gate}")["valid"].sum())
    assert counts[0.0] > counts[45.0] > counts[float("inf")] == 0
    strided = np.ascontiguousarray(np.pad(disp, ((0, 0), (0, 7)), constant_values=-7.0))[:, :W]
    assert strided.strides[0] == 4 * (W + 7)
    _check_locate(ctx, strided, "kitti", False, 4.0, n, "strided map")
    e = _locate_edges()[:n]
    for geom in ("kitti", "pow2"):
        ref = _check_locate(ctx, zero, geom, True, 4.0, n, f"zero-disparity map, {geom}")
        on_edge = (ref["valid"] != 0) & (ref["gt_xy"][:, 0] == e["x"])
        assert on_edge.sum() >= 5
        if geom == "pow2":
            assert np.isinf(ref["gamma_left"][on_edge]).any() and np.isnan(ref["gamma_right"][on_edge]).any()
        else:
            assert np.isfinite(ref["gamma_left"][on_edge]).all()
    ref = _check_locate(ctx, disp, "slant", False, 4.0, n, "slanted calibration")
    assert ref["valid"].sum() > 100
