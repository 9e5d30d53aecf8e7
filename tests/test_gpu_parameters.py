"""The chains off their default parameters and on their thresholds, against the oracle, bit for bit.

Every other parity test runs the reference's constants.  Here each parameter of ebvo_stereo_params, ebvo_finalize_params
and ebvo_temporal_params moves, one at a time around the defaults, and onto values that realized pairs sit exactly on:

  * the four stereo thresholds set to a realized epipolar distance, disparity, orientation difference and NCC score and
    to the next double; the decision for every pair comes from a plain numpy float64 restatement of the reference's
    expressions as well as from the oracle, and the pairs inside the 2^-50 band of pair_passes (where the device divides
    and takes the square root to decide) are counted: both predicates must have some;
  * sweeps through ebvo_stereo_run, _submit / _wait and the host-buffer, staged and resident candidate searches, every
    stage_mask, +inf thresholds, alternating parameter sets on one slot (graph launches and direct launches);
  * the finalize chain (BNB ratio, second NCC threshold, Gauss-Newton, SIFT) against tests/oracle_chain.py;
  * the temporal quads (cell size, radius, orientation, NCC, the stages after it) against the oracle chain, and a radius
    far wider than the grid;
  * refusals: NaN or negative stereo thresholds and a non-finite grid radius return EBVO_ERR_ARG and leave the slot's
    pair and results as they were.
"""
import functools
import math

import numpy as np
import pytest

from edge_based_visual_odometry_amd import synth
from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, STAGE_ALL, EbvoError, ptr
from tests import oracle as orc
from tests import oracle_chain
from tests.util import assert_bit_equal, assert_edges_equal

pytestmark = pytest.mark.gpu

INF = math.inf
NAN = math.nan
BAND = 2.0 ** -50           # pair_passes decides without dividing outside (1 -+ 2^-50) x the scaled / squared threshold
THRESHOLDS = ("epi_thr", "max_disp", "orient_thr_deg", "ncc_thr")
DEFAULT = dict(epi_thr=0.5, max_disp=25.0, orient_thr_deg=10.0, ncc_thr=0.6)   # ebvo_stereo_default_params
KEYS = ("row_ptr", "col_idx", "sims", "best", "keep")
F_KITTI = synth.fundamental_for("kitti")
# slanted epipolar lines for a 120 x 200 image (the EuRoC F leaves this small synthetic pair without candidates): a small
# rotation and a vertical baseline component, as in tests/test_gpu_match.py
_c, _s = np.cos(0.03), np.sin(0.03)
F_SLANT = synth.fundamental_21((450.0, 450.0, 100.0, 60.0), (460.0, 455.0, 98.0, 63.0),
                               ((_c, -_s, 0.0), (_s, _c, 0.0), (0.0, 0.0, 1.0)), (0.11, 0.02, 0.003))
PAIRS = {"kitti200": (200, 320, F_KITTI), "slant120": (120, 200, F_SLANT), "kitti120": (120, 200, F_KITTI),
         "euroc160": (160, 240, synth.fundamental_for("euroc"))}


def _calib(cfg):
    c = synth.CALIB[cfg]
    return ([c["K"][0], 0, c["K"][2], 0, c["K"][1], c["K"][3], 0, 0, 1],
            [c["K_right"][0], 0, c["K_right"][2], 0, c["K_right"][1], c["K_right"][3], 0, 0, 1], c["R21"], c["T21"])


# --- the oracle's view of a pair --------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair(name):
    """(left image, right image, F, oracle TOED edges of both images, epipolar lines of the left edges)"""
    h, w, F = PAIRS[name]
    l, r = synth.stereo_pair("s2", h, w)
    L, R = orc.toed(l)["edges"], orc.toed(r)["edges"]
    return l, r, F, L, R, orc.epipolar_lines(F, L)


@functools.lru_cache(maxsize=None)
def _olist(name, epi_thr, max_disp, orient_thr_deg, mask=STAGE_ALL):
    _, _, _, L, R, lines = _pair(name)
    return orc.epi_candidates(L, R, lines, epi_thr, max_disp, orient_thr_deg, stage_mask=mask)


@functools.lru_cache(maxsize=None)
def _oracle(name, epi_thr, max_disp, orient_thr_deg, ncc_thr, mask=STAGE_ALL):
    l, r, _, L, R, _ = _pair(name)
    rp, ci = _olist(name, epi_thr, max_disp, orient_thr_deg, mask)
    sims, best, keep, _ = orc.ncc_pairs(l, r, L, R[ci], rp, ncc_thr)
    return dict(row_ptr=rp, col_idx=ci, sims=sims, best=best, keep=keep)


def _thr(**changes):
    t = dict(DEFAULT)
    t.update({k: float(v) for k, v in changes.items()})
    return t


def _params(ctx, F, thr, mask=STAGE_ALL):
    p = ctx.default_params(F)
    for k in THRESHOLDS:
        setattr(p, k, thr[k])
    p.stage_mask = mask
    return p


def _run_pair(ctx, name, thr, mask=STAGE_ALL, how="run"):
    """the resident pipeline on the pair (slot 0): (counts, full fetch)"""
    l, r, F = _pair(name)[:3]
    ctx.stereo_upload(l, r)
    p = _params(ctx, F, thr, mask)
    if how == "run":
        c = ctx.stereo_run(p)
    else:
        ctx.stereo_submit(p, 0)
        c = ctx.stereo_wait(0)
    return c, ctx.stereo_fetch(c)


def _assert_pair(c, out, name, thr, mask=STAGE_ALL, what=""):
    _, _, _, L, R, _ = _pair(name)
    ref = _oracle(name, *(thr[k] for k in THRESHOLDS), mask)
    assert_edges_equal(out["left"], L, f"{what}: left edges")
    assert_edges_equal(out["right"], R, f"{what}: right edges")
    for k in KEYS:
        assert_bit_equal(out[k], ref[k], f"{what}: {k}")
    assert (c.n_left, c.n_right, c.n_pairs, c.n_matches) == (len(L), len(R), len(ref["col_idx"]), int(ref["keep"].sum())), what


# --- 1. thresholds placed on realized values --------------------------------------------------------------------------
def _quantities(L, R, lines, rows, cols):
    """The reference's three quantities (src/Stereo_Matches.cpp:99-101, :545-546, :887-901) in numpy float64: no
    contraction, correctly rounded division and square root -- a restatement of its own, not the oracle's code."""
    a, b, c = lines[rows, 0], lines[rows, 1], lines[rows, 2]
    x, y = R["x"][cols], R["y"][cols]
    num = np.abs((a * x + b * y) + c)
    nrm = np.sqrt(a * a + b * b)
    dx, dy = L["x"][rows] - x, L["y"][rows] - y
    s = dx * dx + dy * dy
    od = np.abs((L["theta"][rows] - R["theta"][cols]) * (180.0 / np.pi))
    od = np.where(od > 180.0, 360.0 - od, od)
    return dict(num=num, nrm=nrm, dist=num / nrm, s=s, disp=np.sqrt(s), od=od)


def _orient_ok(q, o):
    return (q["od"] < o) | (np.abs(q["od"] - 180.0) < o)


def _decide(q, thr):
    """the reference's decision for every pair of the universe, from the numpy quantities"""
    return (q["dist"] < thr["epi_thr"]) & (q["disp"] <= thr["max_disp"]) & _orient_ok(q, thr["orient_thr_deg"])


def _band_counts(q, thr):
    """pairs for which pair_passes takes its exact branch: the orientation passes, both cheap tests leave the pair
    passing or undecided, and the epipolar (resp. disparity) value lies inside the 2^-50 band around its threshold"""
    t = thr["epi_thr"] * q["nrm"]
    e_fast, e_maybe = q["num"] < t * (1.0 - BAND), q["num"] <= t * (1.0 + BAND)
    d2 = thr["max_disp"] * thr["max_disp"]
    d_fast, d_maybe = q["s"] < d2 * (1.0 - BAND), q["s"] <= d2 * (1.0 + BAND)
    ok = _orient_ok(q, thr["orient_thr_deg"]) & e_maybe & d_maybe
    return int((ok & ~e_fast).sum()), int((ok & e_fast & ~d_fast).sum())


@pytest.mark.parametrize("name", ["kitti200", "slant120"])
def test_thresholds_on_realized_values(ctx, name):
    _, _, _, L, R, lines = _pair(name)
    # the universe: every pair within generous epipolar and disparity bounds; every run below lies inside it
    urp, uci = _olist(name, 3.0, 60.0, 10.0, 3)
    rows, cols = oracle_chain.rows_of(urp), uci.astype(np.int64)
    q = _quantities(L, R, lines, rows, cols)
    assert len(cols) > 1000

    def pick(mask, value, target):
        k = np.flatnonzero(mask)
        assert len(k), f"{name}: no pair to place the threshold on"
        return int(k[np.argmin(np.abs(value[k] - target))])

    o_def, e_def, d_def = _orient_ok(q, 10.0), q["dist"] < 0.5, q["disp"] <= 25.0
    wide = dict(epi_thr=3.0, max_disp=60.0)
    near180 = np.abs(q["od"] - 180.0)
    runs = []   # (thresholds, index into the universe, must that pair be listed)
    k = pick(o_def & d_def, q["dist"], 0.5)
    runs += [(_thr(epi_thr=q["dist"][k]), k, False), (_thr(epi_thr=np.nextafter(q["dist"][k], INF)), k, True)]
    k = pick(o_def & e_def & (q["s"] > 0), q["disp"], 12.0)
    runs += [(_thr(max_disp=q["disp"][k]), k, True), (_thr(max_disp=np.nextafter(q["disp"][k], -INF)), k, False)]
    k = pick((q["od"] > 0.5) & (q["od"] < 9.0), q["od"], 5.0)
    runs += [(_thr(orient_thr_deg=q["od"][k], **wide), k, False),
             (_thr(orient_thr_deg=np.nextafter(q["od"][k], INF), **wide), k, True)]
    k = pick((near180 > 0.01) & (near180 < 9.0), near180, 5.0)
    runs += [(_thr(orient_thr_deg=near180[k], **wide), k, False),
             (_thr(orient_thr_deg=np.nextafter(near180[k], INF), **wide), k, True)]
    bands = [0, 0]
    for thr, k, listed in runs:
        what = f"{name} {thr}"
        c, out = _run_pair(ctx, name, thr)
        _assert_pair(c, out, name, thr, what=what)
        i = rows[k]
        assert bool((out["col_idx"][out["row_ptr"][i]:out["row_ptr"][i + 1]] == cols[k]).any()) == listed, what
        # the whole list is the numpy decision on the universe
        ok = _decide(q, thr)
        assert_bit_equal(out["col_idx"], cols[ok].astype(np.int32), f"{what}: numpy decision")
        assert_bit_equal(np.diff(out["row_ptr"]), np.bincount(rows[ok], minlength=len(L)).astype(np.int32), what)
        e, d = _band_counts(q, thr)
        bands[0] += e
        bands[1] += d
    assert bands[0] > 0 and bands[1] > 0, f"pairs inside the 2^-50 band (epipolar, disparity): {bands}"
    # ncc_thr on a realized best score: that pair loses `keep`
    ref = _oracle(name, *DEFAULT.values())
    kept = np.flatnonzero(ref["keep"])
    k = int(kept[np.argmin(np.abs(ref["best"][kept] - 0.8))])
    thr = _thr(ncc_thr=ref["best"][k])
    c, out = _run_pair(ctx, name, thr)
    _assert_pair(c, out, name, thr, what=f"{name} ncc_thr on a best score")
    assert out["keep"][k] == 0 and c.n_matches < int(ref["keep"].sum())
    assert_bit_equal(out["keep"], (out["best"] > thr["ncc_thr"]).astype(np.uint8), "keep = best > ncc_thr")


# --- 2. one parameter at a time, through every entry point ------------------------------------------------------------
SWEEP = ([("epi_thr", v) for v in (0.0, 0.25, 1.5, 3.0, INF)] + [("max_disp", v) for v in (0.0, 8.0, 60.0, 1e4, INF)] +
         [("orient_thr_deg", v) for v in (0.0, 3.0, 30.0, 90.0, 180.0, 200.0)] +
         [("ncc_thr", v) for v in (-1.0, 0.0, 0.3, 0.95, 1.0)])


def _check_candidate_searches(ctx, name, thr, mask):
    """host-buffer ebvo_epi_candidates / _staged and the resident ones on the pair's edge lists, against the oracle"""
    l, r, _, L, R, lines = _pair(name)
    g = (thr["epi_thr"], thr["max_disp"], thr["orient_thr_deg"])
    rp, ci = _olist(name, *g, mask)
    grp, gci = ctx.epi_candidates(L, R, lines, *g, stage_mask=mask)
    assert_bit_equal(grp, rp, "host-buffer row_ptr")
    assert_bit_equal(gci, ci, "host-buffer col_idx")
    tl, tr = ctx.toed_resident(l, 0)[3], ctx.toed_resident(r, 1)[3]
    grp, gci = ctx.epi_candidates_resident(tl, tr, lines, *g, stage_mask=mask)
    assert_bit_equal(grp, rp, "resident row_ptr")
    assert_bit_equal(gci, ci, "resident col_idx")
    if mask != STAGE_ALL:
        return
    rp3, ci3 = _olist(name, *g, 3)
    for where, (srp, sci, sok) in (("staged", ctx.epi_candidates_staged(L, R, lines, *g)),
                                   ("resident staged", ctx.epi_candidates_resident(tl, tr, lines, *g, staged=True))):
        assert_bit_equal(srp, rp3, f"{where} row_ptr (epipolar + disparity)")
        assert_bit_equal(sci, ci3, f"{where} col_idx (epipolar + disparity)")
        assert_bit_equal(sci[sok.astype(bool)], ci, f"{where}: flagged pairs")
    frp, fci = ctx.last_final_lists
    assert_bit_equal(frp, rp, "resident final row_ptr")
    assert_bit_equal(fci, ci, "resident final col_idx")


@pytest.mark.parametrize("param,value", SWEEP, ids=[f"{p}={v}" for p, v in SWEEP])
def test_one_threshold_at_a_time(ctx, param, value):
    thr = _thr(**{param: value})
    for how in ("run", "submit"):
        c, out = _run_pair(ctx, "kitti200", thr, how=how)
        _assert_pair(c, out, "kitti200", thr, what=f"{how} {param}={value}")
    _check_candidate_searches(ctx, "kitti200", thr, STAGE_ALL)


@pytest.mark.parametrize("mask", range(1, 8))
def test_every_stage_mask(ctx, mask):
    name = "kitti200" if mask & 1 else "slant120"    # the lists without the epipolar stage are large: smaller pair
    for how in ("run", "submit"):
        c, out = _run_pair(ctx, name, DEFAULT, mask, how=how)
        _assert_pair(c, out, name, DEFAULT, mask, what=f"{how} mask {mask}")
        assert c.n_pairs > 0
    _check_candidate_searches(ctx, name, DEFAULT, mask)


@pytest.mark.parametrize("graphs", [1, 0], ids=["graph", "direct"])
def test_alternating_parameter_sets_on_one_slot(ctx, graphs):
    sets = [DEFAULT, _thr(epi_thr=1.5, max_disp=8.0, orient_thr_deg=30.0, ncc_thr=0.3),
            _thr(epi_thr=INF, max_disp=60.0, orient_thr_deg=3.0, ncc_thr=0.95)]
    order = [0, 0, 0, 1, 1, 1, 2, 0]        # three equal keys in a row: a capture, then a graph launch
    before = ctx.graph_launches
    ctx.debug_set(10, graphs)
    try:
        for n, s in enumerate(order):
            c, out = _run_pair(ctx, "kitti200", sets[s], how="submit")
            _assert_pair(c, out, "kitti200", sets[s], what=f"submission {n} (set {s})")
    finally:
        ctx.debug_set(10, 1)
    assert (ctx.graph_launches > before) == bool(graphs)


# --- 3. refusals ------------------------------------------------------------------------------------------------------
BAD = [(k, NAN) for k in THRESHOLDS] + [("epi_thr", -1.0), ("max_disp", -5e-7), ("max_disp", -INF), ("orient_thr_deg", -1.0)]


def test_refused_thresholds_leave_the_slot_intact(ctx):
    l, r, F, L, R, lines = _pair("kitti200")
    c0, before = _run_pair(ctx, "kitti200", DEFAULT)
    for param, value in BAD:
        thr = _thr(**{param: value})
        for call in (lambda p: ctx.stereo_submit(p, 0), ctx.stereo_run):
            with pytest.raises(EbvoError) as ei:
                call(_params(ctx, F, thr))
            assert ei.value.status == EBVO_ERR_ARG, (param, value)
        if param != "ncc_thr":
            g = (thr["epi_thr"], thr["max_disp"], thr["orient_thr_deg"])
            for call in (lambda: ctx.epi_candidates(L, R, lines, *g), lambda: ctx.epi_candidates_staged(L, R, lines, *g)):
                with pytest.raises(EbvoError) as ei:
                    call()
                assert ei.value.status == EBVO_ERR_ARG, (param, value)
        # the previous pair still fetches the same bits
        after = ctx.stereo_fetch(c0)
        assert_edges_equal(after["left"], before["left"], f"{param}={value}: left")
        assert_edges_equal(after["right"], before["right"], f"{param}={value}: right")
        for k in KEYS:
            assert_bit_equal(after[k], before[k], f"{param}={value}: {k}")
    c1 = ctx.stereo_run(_params(ctx, F, DEFAULT))            # ... and its images are still resident
    _assert_pair(c1, ctx.stereo_fetch(c1), "kitti200", DEFAULT, what="after the refusals")
    # the resident searches refuse too, and leave the tags valid
    tl, tr = ctx.toed_resident(l, 0)[3], ctx.toed_resident(r, 1)[3]
    for param, value in BAD:
        if param != "ncc_thr":
            thr = _thr(**{param: value})
            with pytest.raises(EbvoError) as ei:
                ctx.epi_candidates_resident(tl, tr, lines, thr["epi_thr"], thr["max_disp"], thr["orient_thr_deg"])
            assert ei.value.status == EBVO_ERR_ARG, (param, value)
    grp, gci = ctx.epi_candidates_resident(tl, tr, lines)
    ref = _oracle("kitti200", *DEFAULT.values())
    assert_bit_equal(grp, ref["row_ptr"], "resident row_ptr after the refusals")
    assert_bit_equal(gci, ref["col_idx"], "resident col_idx after the refusals")


def test_negative_disparity_on_identical_images(ctx):
    """Left = right: every edge has a right edge at its own location (s = 0).  The reference's sqrt(0) <= max_disp
    rejects it for any negative max_disp, a squared test against max_disp^2 accepts it: such a max_disp is refused.
    max_disp = 0 lists exactly the coincident pairs."""
    l = synth.stereo_pair("s2", 120, 200)[0]
    L = orc.toed(l)["edges"]
    lines = orc.epipolar_lines(F_KITTI, L)
    assert len(orc.epi_candidates(L, L, lines, 0.5, -5e-7, 10.0)[1]) == 0
    rp0, ci0 = orc.epi_candidates(L, L, lines, 0.5, 0.0, 10.0)
    assert len(ci0) >= len(L)
    ctx.stereo_upload(l, l)
    with pytest.raises(EbvoError) as ei:
        ctx.stereo_run(_params(ctx, F_KITTI, _thr(max_disp=-5e-7)))
    assert ei.value.status == EBVO_ERR_ARG
    with pytest.raises(EbvoError) as ei:
        ctx.epi_candidates(L, L, lines, 0.5, -5e-7, 10.0)
    assert ei.value.status == EBVO_ERR_ARG
    c = ctx.stereo_run(_params(ctx, F_KITTI, _thr(max_disp=0.0)))
    out = ctx.stereo_fetch(c)
    assert_bit_equal(out["row_ptr"], rp0, "row_ptr at max_disp 0")
    assert_bit_equal(out["col_idx"], ci0, "col_idx at max_disp 0")


# --- 4. finalize ------------------------------------------------------------------------------------------------------
GN_SETS = [(1, 1e-3, 3.0), (3, 0.0, 0.5), (20, 0.5, 10.0)]
FINALIZE = ([dict(bnb_ratio=v) for v in (0.0, 0.5, 1.0)] + [dict(ncc_thr=v) for v in (0.3, 0.8)] +
            [dict(max_iter=a, tol=b, huber_delta=c) for a, b, c in GN_SETS] +
            [dict(use_sift=True, sift_thr=t, bnb_sift=b) for t in (50.0, 1e9) for b in (0.0, 0.8)])
FIN_CALIB = {"kitti120": "kitti", "kitti200": "kitti", "euroc160": "euroc"}
FIN_CASES = [(n, i) for n in ("kitti120", "kitti200") for i in range(len(FINALIZE))] + [("euroc160", i) for i in (0, 4, 7, 11)]


def _fin_id(case):
    return case[0] + "-" + "-".join(f"{k}={v}" for k, v in FINALIZE[case[1]].items())


@functools.lru_cache(maxsize=None)
def _oracle_chain(name, i):
    kw = FINALIZE[i]
    l, r, F, L, R, _ = _pair(name)
    o = _oracle(name, *DEFAULT.values())
    stage1 = dict(left=L, right=R, row_ptr=o["row_ptr"], col_idx=o["col_idx"], best=o["best"], keep=o["keep"])
    return oracle_chain.stereo_edge_pairs(
        l, r, F, _calib(FIN_CALIB[name]), bnb_ratio=kw.get("bnb_ratio", 0.9), ncc_thr=kw.get("ncc_thr", 0.6), stage1=stage1,
        sift=kw.get("use_sift", False), sift_thr=kw.get("sift_thr", 500.0), bnb_sift=kw.get("bnb_sift", 0.4),
        max_iter=kw.get("max_iter", 20), tol=kw.get("tol", 1e-3), huber_delta=kw.get("huber_delta", 3.0))


@pytest.mark.parametrize("case", FIN_CASES, ids=[_fin_id(c) for c in FIN_CASES])
def test_finalize_parameters(ctx, case):
    name, i = case
    kw = FINALIZE[i]
    ref = _oracle_chain(name, i)
    assert ref["counts"]["n_final"] > 0
    calib = _calib(FIN_CALIB[name])
    for how in ("finalize", "submit"):
        _run_pair(ctx, name, DEFAULT)
        if how == "finalize":
            counts, fin = ctx.stereo_finalize(calib, **kw)
        else:
            ctx.stereo_finalize_submit(calib, **kw)
            counts, fin = ctx.stereo_finalize_wait()
        assert counts == ref["counts"], how
        assert_bit_equal(fin["left_index"], ref["left_index"], f"{how}: left_index")
        assert_edges_equal(fin["right"], ref["right"], f"{how}: right centres")
        assert_bit_equal(fin["score"], ref["score"], f"{how}: score")
        assert_bit_equal(fin["rows"], ref["rows"], f"{how}: rows")


def test_finalize_parameters_change_the_result():
    """the cases above are not copies of the default chain (checked on the oracle alone)"""
    base = oracle_chain.stereo_edge_pairs(*_pair("kitti200")[:3], _calib("kitti"))["counts"]
    moved = sum(_oracle_chain("kitti200", i)["counts"] != base for i in range(len(FINALIZE)))
    assert moved >= len(FINALIZE) - 3


# --- 5. temporal ------------------------------------------------------------------------------------------------------
TQ_H, TQ_W = 240, 376
ORACLE_NAME = dict(cell_size="cell", grid_radius="radius", orient_thr_deg="orient_thr_deg", ncc_thr="ncc_thr",
                   sift_thr="sift_thr", bnb_ncc="bnb_ncc", bnb_sift="bnb_sift", max_iter="max_iter", tol="tol",
                   huber_delta="huber")
TEMPORAL = ([dict(cell_size=v) for v in (1, 7, 16, 64, 1000)] + [dict(grid_radius=v) for v in (0.0, 7.5, 30.0, 44.9)] +
            [dict(orient_thr_deg=v) for v in (0.0, 5.0, 45.0, 180.0)] + [dict(ncc_thr=v) for v in (0.5, 0.95)])
TEMPORAL_CHAIN = ([dict(sift_thr=v) for v in (50.0, 1e9)] + [dict(bnb_ncc=a, bnb_sift=b) for a in (0.0, 1.0) for b in (0.0, 1.0)] +
                  [dict(max_iter=a, tol=b, huber_delta=c) for a, b, c in GN_SETS])
_TQ = []    # (mates, images) per distinct set of mates: the detector modes give the same bits, so the oracle runs once


def _tq_inputs(ctx):
    """keyframe = frame 0, current frame = frame 3 of tests/test_gpu_temporal.py's EuRoC-half scene (no undistortion):
    the index of the inputs in _TQ and the mates of both frames as the host sees them"""
    ce = synth.CALIB["euroc"]
    K, Kr = tuple(v / 2 for v in ce["K"]), tuple(v / 2 for v in ce["K_right"])
    F = synth.fundamental_21(K, Kr, ce["R21"], ce["T21"])
    calib = ([K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1], [Kr[0], 0, Kr[2], 0, Kr[1], Kr[3], 0, 0, 1], ce["R21"], ce["T21"])
    mates, imgs = [], []
    for k in (0, 3):
        l, r = synth.stereo_pair("s2", TQ_H, TQ_W, scene=7, noise_base=2 * k, disparity=9)
        l, r = np.roll(l, k, axis=1), np.roll(r, k, axis=1)
        ctx.stereo_upload(l, r)
        c = ctx.stereo_run(ctx.default_params(F))
        left = ctx.stereo_fetch(c)["left"]
        _, fin = ctx.stereo_finalize(calib)
        mates.append((left[fin["left_index"]], fin["right"]))
        imgs.append((l, l, r))
        if k == 0:
            ctx.temporal_set_keyframe()
    for n, (m, _) in enumerate(_TQ):
        if all(oracle_chain._same_edges(a, b) for a, b in zip(m[0] + m[1], mates[0] + mates[1])):
            return n, mates
    _TQ.append((mates, imgs))
    return len(_TQ) - 1, mates


@functools.lru_cache(maxsize=None)
def _temporal_reference(n, items, chain):
    (kf, cf), imgs = _TQ[n]
    kw = {ORACLE_NAME[k]: v for k, v in items}
    return oracle_chain.temporal_reference(*kf, *cf, imgs[0], imgs[1], TQ_W, TQ_H, chain=chain, **kw)


@pytest.mark.parametrize("chain", [False, True], ids=["candidates+ncc", "chain"])
def test_temporal_parameters(ctx, chain):
    n, ((kfL, _), (cfL, _)) = _tq_inputs(ctx)
    assert len(kfL) > 1000 and len(cfL) > 1000
    seen = set()
    for kw in (TEMPORAL_CHAIN if chain else TEMPORAL):
        ref = _temporal_reference(n, tuple(sorted(kw.items())), chain)
        counts, q = ctx.temporal_match(stages=int(chain), **kw)
        bad = oracle_chain.temporal_problems(counts, q, ref)
        assert bad == [], (kw, bad)
        seen.add(tuple(sorted(counts.items())))
    assert len(seen) > len(TEMPORAL_CHAIN if chain else TEMPORAL) // 2     # the parameters do move the results


def _temporal_fetch(ctx, counts):
    m = counts["n_candidates"]
    out = dict(row_ptr=np.zeros(counts["n_kf"] + 1, dtype=np.int32), col_idx=np.zeros(m, dtype=np.int32),
               sim_left=np.zeros(m), sim_right=np.zeros(m), keep=np.zeros(m, dtype=np.uint8))
    ctx._check(ctx.lib.ebvo_temporal_fetch(ctx._ctx, 0, *(ptr(out[k]) for k in ("row_ptr", "col_idx", "sim_left", "sim_right",
                                                                              "keep"))), "ebvo_temporal_fetch")
    return out


@functools.lru_cache(maxsize=None)
def _cover_reference(n, cell, radius):
    (kf, cf), imgs = _TQ[n]
    return oracle_chain.temporal_reference(*kf, *cf, imgs[0], imgs[1], TQ_W, TQ_H, chain=False, cell=cell, radius=radius)


@pytest.mark.parametrize("cell", [15, 4])
def test_temporal_radius_wider_than_the_grid(ctx, cell):
    """grid_radius = 1e6 (ceil(1e6 / cell) cells, far beyond the grid): the device walks the grid only and gives the run
    with the smallest radius that covers the grid, which equals the oracle.  A right mate outside the grid is never a
    candidate.  A non-finite radius is refused and leaves the quads as they were."""
    n, ((kfL, kfR), (cfL, cfR)) = _tq_inputs(ctx)
    gw, gh = (TQ_W + cell - 1) // cell, (TQ_H + cell - 1) // cell

    def cells(v):   # (int)v / cell, truncating towards zero as C does
        return np.trunc(np.trunc(v) / cell).astype(np.int64)

    qx, qy = cells(np.concatenate([kfL["x"], kfR["x"]])), cells(np.concatenate([kfL["y"], kfR["y"]]))
    cover = int(max(np.abs(qx).max(), np.abs(qx - (gw - 1)).max(), np.abs(qy).max(), np.abs(qy - (gh - 1)).max()))
    rx, ry = cells(cfR["x"]), cells(cfR["y"])
    outside = np.flatnonzero((rx < 0) | (rx >= gw) | (ry < 0) | (ry >= gh))    # none in this scene: right centres stay
    ref = _cover_reference(n, cell, float(cover * cell))                          # several px inside the image
    counts_c, q_c = ctx.temporal_match(cell_size=cell, grid_radius=float(cover * cell))
    assert oracle_chain.temporal_problems(counts_c, q_c, ref) == []
    counts_w, q_w = ctx.temporal_match(cell_size=cell, grid_radius=1e6)
    assert counts_w == counts_c and counts_c["n_candidates"] > counts_c["n_kf"]
    for k in ("row_ptr", "col_idx", "sim_left", "sim_right", "keep"):
        assert_bit_equal(q_w[k], q_c[k], f"radius 1e6 vs {cover * cell}: {k}")
    assert not np.isin(q_w["col_idx"], outside).any()
    for bad in (INF, NAN, -1.0):
        with pytest.raises(EbvoError) as ei:
            ctx.temporal_match(cell_size=cell, grid_radius=bad)
        assert ei.value.status == EBVO_ERR_ARG, bad
    after = _temporal_fetch(ctx, counts_w)
    for k in ("row_ptr", "col_idx", "sim_left", "sim_right", "keep"):
        assert_bit_equal(after[k], q_w[k], f"after the refusals: {k}")
