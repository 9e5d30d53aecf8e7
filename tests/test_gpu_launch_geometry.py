"""The pair chain's bits do not depend on how its kernels are launched, nor on where the sizes fall against the kernels'
work units.

Several kernels size their grid from the device (the exact TOED kernels and ncc_tile_kernel: what the chip keeps resident)
or cap it (the counting pass of the candidate search and its per-block partial totals, the latency-bound decide /
cand_scatter / candidates<fill> grids, the persistent Gauss-Newton groups and the active-pair count at which the
refinement changes layout).  The developer keys of ebvo_debug_set move each of these grids; every value below must give
the oracle's bits:

  * the whole resident chain (TOED, candidates, NCC, ebvo_stereo_refine, ebvo_stereo_finalize) at 120x200 and 200x320
    against the oracle, and at KITTI size (bench.py's pair) against the default-geometry run, which is checked against
    the oracle once;
  * the host-buffer entry points at element counts on either side of the kernels' work units (64-edge tiles, 8 / 512
    right edges, the 4096-entry scan tile, the grid-stride wrap of expand_rows / sincos_edges, 32 pairs per GN group);
  * the resident pipeline at image sizes on the edges of what a context accepts;
  * ebvo_debug_set refusing values outside each key's range without changing the context.
"""
import contextlib
import functools

import numpy as np
import pytest

from edge_based_visual_odometry_amd import synth
from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EDGE_DTYPE, EbvoError
from edge_based_visual_odometry_amd.api import Context
from tests import oracle as orc
from tests import oracle_chain
from tests.test_gpu_fullsize import PAIRS, _calib, _oracle, _oracle_chain
from tests.util import assert_bit_equal, assert_edges_equal

pytestmark = pytest.mark.gpu

F_KITTI = synth.fundamental_for("kitti")
CALIB = _calib(PAIRS["kitti"][0])
REFINED = ("alpha", "score", "confidence", "validity", "iters", "refined_xy")
DEFAULTS = {10: 1}   # every other key used here: 0 = the library's own choice


@contextlib.contextmanager
def _keys(c, settings):
    try:
        for k, v in settings.items():
            c.debug_set(k, v)
        yield
    finally:
        for k in settings:
            c.debug_set(k, DEFAULTS.get(k, 0))


@pytest.fixture(scope="module", params=["strict", "hybrid"])
def gctx(request):
    """A context of the geometry tests' own (a changed key can never reach the session context), sized exactly for the
    KITTI pair."""
    c = Context(*synth.SHAPES["kitti"], device=0, toed_mode=request.param)
    yield c
    c.close()


# --- the chain on one pair and what the oracle says it must give ------------------------------------------------------

def _chain(c, l, r, F=F_KITTI, calib=CALIB):
    """upload -> run -> fetch -> refine -> finalize on the resident pair; every output in one dict"""
    c.stereo_upload(l, r)
    cnt = c.stereo_run(c.default_params(F))
    out = c.stereo_fetch(cnt)
    out["counts"] = (cnt.n_left, cnt.n_right, cnt.n_pairs, cnt.n_matches)
    ref = c.stereo_refine(cnt)
    out.update({"gn_" + k: v for k, v in ref.items()})
    fc, fin = c.stereo_finalize(calib)
    out["fin_counts"] = fc
    out.update({"fin_" + k: v for k, v in fin.items()})
    return out


def _refine_expected(o):
    """ebvo_stereo_refine's per-pair outputs: the oracle's refinement of the kept matches, the unrefined record elsewhere"""
    keep = o["keep"].astype(bool)
    n, nL = len(o["col_idx"]), len(o["left"])
    rows = np.repeat(np.arange(nL), np.diff(o["row_ptr"]))
    xy = np.stack([o["right"]["x"][o["col_idx"]], o["right"]["y"][o["col_idx"]]], 1)
    rp = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=nL))]).astype(np.int32)
    ref = orc.gn_refine_stereo(o["l"], o["r"], o["left"], orc.epipolar_lines(o["F"], o["left"]), rp, xy[keep])
    full = dict(alpha=np.zeros(n), score=np.full(n, np.nan), confidence=np.full(n, np.nan),
                validity=np.full(n, 255, dtype=np.uint8), iters=np.zeros(n, dtype=np.int32), refined_xy=xy)
    for k in REFINED:
        full[k][keep] = ref[k]
    return full


def _expected_of(o, chain, refine=True):
    e = dict(left=o["left"], right=o["right"], row_ptr=o["row_ptr"], col_idx=o["col_idx"], sims=o["sims"],
             best=o["best"], keep=o["keep"], counts=(len(o["left"]), len(o["right"]), len(o["col_idx"]),
                                                     int(o["keep"].sum())))
    if refine:
        e.update({"gn_" + k: v for k, v in _refine_expected(o).items()})
    e["fin_counts"] = chain["counts"]
    for k in ("left_index", "right", "score", "rows"):
        e["fin_" + k] = chain[k]
    return e


@functools.lru_cache(maxsize=None)
def _expected(h, w, refine=True):
    """(stage-1 oracle dict, expected chain outputs) of synth.stereo_pair("s2", h, w); refine: with ebvo_stereo_refine's"""
    l, r = synth.stereo_pair("s2", h, w)
    L, R = orc.toed(l)["edges"], orc.toed(r)["edges"]
    lines = orc.epipolar_lines(F_KITTI, L)
    rp, ci = orc.epi_candidates(L, R, lines)
    sims, best, keep, _ = orc.ncc_pairs(l, r, L, R[ci], rp)
    o = dict(l=l, r=r, F=F_KITTI, left=L, right=R, row_ptr=rp, col_idx=ci, sims=sims, best=best, keep=keep)
    chain = oracle_chain.stereo_edge_pairs(l, r, F_KITTI, CALIB, stage1=o)
    return o, _expected_of(o, chain, refine)


@functools.lru_cache(maxsize=None)
def _kitti_expected():
    return _expected_of(_oracle("kitti"), _oracle_chain("kitti"))


def _same(got, exp):
    assert got["counts"] == exp["counts"], (got["counts"], exp["counts"])
    assert_edges_equal(got["left"], exp["left"], "left edges")
    assert_edges_equal(got["right"], exp["right"], "right edges")
    for k in ("row_ptr", "col_idx", "sims", "best", "keep") + tuple("gn_" + k for k in REFINED):
        assert_bit_equal(got[k], exp[k], k)
    assert got["fin_counts"] == exp["fin_counts"], (got["fin_counts"], exp["fin_counts"])
    assert_bit_equal(got["fin_left_index"], exp["fin_left_index"], "fin_left_index")
    assert_edges_equal(got["fin_right"], exp["fin_right"], "fin_right")
    assert_bit_equal(got["fin_score"], exp["fin_score"], "fin_score")
    assert_bit_equal(got["fin_rows"], exp["fin_rows"], "fin_rows")


# --- 1. launch-geometry invariance -------------------------------------------------------------------------------------

# (key, value) one at a time; "kept" values are taken relative to the kept-match count of the pair being refined
SWEEP = ([(11, v) for v in (1, 3, 7, 100, 1021, 8192)] +      # toed_exact_centre grid (hybrid; a no-op in strict)
         [(12, v) for v in (1, 3, 7, 100, 1021, 8192)] +      # toed_exact_mags grid
         [(17, v) for v in (1, 9, 24, 520, 4096)] +            # ncc_tile_kernel grid (multiple of 8, 8 .. EBVO_MATCH_PARTS)
         [(18, v) for v in (1, 3, 7, 512)] +                   # divisor of the decide / cand_scatter / candidates<fill> grids
         [(19, v) for v in (1, 2, 5, 1023, 4096)] +            # blocks (partial totals) of candidates<count>
         [(9, v) for v in (1, 3, 1024, 1 << 20)] +             # persistent GN groups
         [(5, v) for v in (1, 31, 32, 33, "kept-1", "kept", "kept+1")])   # GN rows_below
COMBINED = {
    "minimal": {11: 1, 12: 1, 17: 8, 18: 512, 19: 1, 9: 1},
    "large": {11: 8192, 12: 8192, 17: 4096, 18: 1, 19: 4096, 9: 1 << 20},
}
SETTINGS = [(f"k{k}={v}", {k: v}) for k, v in SWEEP] + list(COMBINED.items())
SETTING_IDS = [s[0] for s in SETTINGS]


@functools.lru_cache(maxsize=None)
def _other_pair(h, w):
    return synth.stereo_pair("s2", h, w, **PAIRS["euroc"][1])


def _scrub(c, h, w):
    """another pair of the same size through the chain first: no entry a kernel fails to write under the grid being tested
    can still hold the expected bits from an earlier run"""
    _chain(c, *_other_pair(h, w))


def _resolve(settings, n_kept):
    offs = {"kept-1": -1, "kept": 0, "kept+1": 1}
    return {k: n_kept + offs[v] if isinstance(v, str) else v for k, v in settings.items()}


@pytest.mark.parametrize("shape", [(120, 200), (200, 320)], ids=["120x200", "200x320"])
@pytest.mark.parametrize("name,settings", SETTINGS, ids=SETTING_IDS)
def test_small_pair_chain_equals_oracle_at_every_grid(gctx, shape, name, settings):
    o, exp = _expected(*shape)
    _scrub(gctx, *shape)
    with _keys(gctx, _resolve(settings, exp["counts"][3])):
        got = _chain(gctx, o["l"], o["r"])
    _same(got, exp)


@pytest.fixture(scope="module")
def kitti_default(gctx):
    """bench.py's pair (PAIRS["kitti"]) through the chain at the library's own grids, once per context"""
    o = _oracle("kitti")
    return _chain(gctx, o["l"], o["r"])


def test_kitti_default_grid_equals_oracle(kitti_default):
    _same(kitti_default, _kitti_expected())
    assert kitti_default["counts"] == (126184, 126340, 581657, 472947)


@pytest.mark.parametrize("name,settings", SETTINGS, ids=SETTING_IDS)
def test_kitti_chain_equals_default_grid_run(gctx, kitti_default, name, settings):
    o = _oracle("kitti")
    _scrub(gctx, *synth.SHAPES["kitti"])
    with _keys(gctx, _resolve(settings, kitti_default["counts"][3])):
        got = _chain(gctx, o["l"], o["r"])
    _same(got, kitti_default)


@pytest.mark.parametrize("graphs", [1, 0], ids=["graph", "direct"])
def test_changed_grid_reaches_the_captured_graph(gctx, graphs):
    """A pair submitted often enough runs as a captured hipGraph.  Grids changed after the capture (ebvo_debug_set bumps
    the settings generation, so the chain is captured again) give the oracle's bits, as graph and as direct launches."""
    o, exp = _expected(120, 200)
    for _ in range(3):
        _same(_chain(gctx, o["l"], o["r"]), exp)
    with _keys(gctx, {10: graphs, **COMBINED["minimal"]}):
        before = gctx.graph_launches
        for _ in range(3):
            _same(_chain(gctx, o["l"], o["r"]), exp)
        assert (gctx.graph_launches > before) == bool(graphs)
    with _keys(gctx, {10: graphs, **COMBINED["large"]}):
        for _ in range(3):
            _same(_chain(gctx, o["l"], o["r"]), exp)
    _same(_chain(gctx, o["l"], o["r"]), exp)


# --- 2. count boundaries through the host-buffer entry points ---------------------------------------------------------

def _rand_edges(rng, n, w, h, margin=0.0):
    e = np.zeros(n, dtype=EDGE_DTYPE)
    e["x"], e["y"] = rng.uniform(margin, w - margin, n), rng.uniform(margin, h - margin, n)
    e["theta"] = rng.uniform(-np.pi, np.pi, n)
    e["index"] = np.arange(n)
    return e


@pytest.mark.parametrize("nL,nR", [(n, 500) for n in (1, 63, 64, 65, 4095, 4096, 4097, 8193)] +
                         [(300, n) for n in (1, 7, 8, 9, 511, 512, 513)])
def test_candidates_at_tile_and_chunk_edges(ctx, nL, nR):
    """64-edge tiles of left edges (and the 4096-entry tile of the row-pointer scan); chunks of 8 and batches of 512
    right edges"""
    rng = np.random.default_rng(nL * 1000 + nR)
    L, R = _rand_edges(rng, nL, 300, 200), _rand_edges(rng, nR, 300, 200)
    L["y"][1::5] += 400.0                             # every fifth row empty: no right edge near its epipolar line
    lines = orc.epipolar_lines(F_KITTI, L)           # y = y_L: rectified
    thr = (20.0 if nR < 64 else 4.0, 150.0, 45.0)     # wide enough that the other rows are mostly non-empty
    rp, ci = orc.epi_candidates(L, R, lines, *thr)
    grp, gci = ctx.epi_candidates(L, R, lines, *thr)
    assert_bit_equal(grp, rp, "row_ptr")
    assert_bit_equal(gci, ci, "col_idx")
    n = np.diff(rp)
    assert (n > 0).any() and (nL == 1 or (n == 0).any())


def _ragged_rows(rng, nL, n_pairs=None):
    per = rng.integers(0, 5, nL)                      # 0 .. 4 candidates a row, empty rows included
    if nL > 1:
        per[rng.choice(nL, max(1, nL // 7), replace=False)] = 0
    if n_pairs is not None:                           # exactly n_pairs in all
        d = n_pairs - int(per.sum())
        pick = rng.permutation(np.flatnonzero(per < 4 if d > 0 else per > 0))[:abs(d)]
        assert len(pick) == abs(d)
        per[pick] += 1 if d > 0 else -1
    return np.concatenate([[0], np.cumsum(per)]).astype(np.int32)


@pytest.mark.parametrize("nL,n_pairs", [(1, None), (255, None), (256, None), (257, None), (131073, None),
                                        (131073, 262144 + 97)])
def test_ncc_pairs_at_grid_stride_edges(ctx, nL, n_pairs):
    """expand_rows_kernel covers at most 512 x 256 rows a sweep and sincos_edges_kernel 1024 x 256 pairs: 131,073 left
    edges and 262,241 pairs make both wrap"""
    rng = np.random.default_rng(nL + 7)
    l, r = synth.stereo_pair("s2", 376, 1241)
    L = _rand_edges(rng, nL, 1241, 376, 2.0)
    rp = _ragged_rows(rng, nL, n_pairs)
    if nL == 1:
        rp = np.array([0, 3], dtype=np.int32)
    rows = np.repeat(np.arange(nL), np.diff(rp))
    Rc = L[rows].copy()                               # candidates near the left edge's mirror location
    Rc["x"] = Rc["x"] - rng.uniform(0, 20, len(Rc))
    Rc["y"] = Rc["y"] + rng.uniform(-0.5, 0.5, len(Rc))
    Rc["theta"] = Rc["theta"] + rng.uniform(-0.2, 0.2, len(Rc))
    Rc["index"] = np.arange(len(Rc))
    if n_pairs is not None:
        assert rp[-1] == n_pairs
    sims, best, keep, _ = ctx.ncc_pairs(l, r, L, Rc, rp)
    osims, obest, okeep, _ = orc.ncc_pairs(l, r, L, Rc, rp)
    assert_bit_equal(sims, osims, "sims")
    assert_bit_equal(best, obest, "best")
    assert_bit_equal(keep, okeep, "keep")
    assert len(keep) == 0 or not np.isnan(osims).all()


@functools.lru_cache(maxsize=None)
def _gn_problem():
    """one left edge per pair: kept matches of a 200x320 pair (left edge, right edge location)"""
    o, _ = _expected(200, 320)
    keep = o["keep"].astype(bool)
    rows = np.repeat(np.arange(len(o["left"])), np.diff(o["row_ptr"]))[keep]
    cand = np.stack([o["right"]["x"][o["col_idx"][keep]], o["right"]["y"][o["col_idx"][keep]]], 1)
    pick = np.random.default_rng(4).permutation(len(rows))[:1025]
    L = o["left"][rows[pick]].copy()
    return o["l"], o["r"], L, orc.epipolar_lines(F_KITTI, L), cand[pick]


def _gn_compare(c, n):
    l, r, L, lines, cand = _gn_problem()
    assert len(L) >= n
    rp = np.arange(n + 1, dtype=np.int32)
    out = c.gn_refine_stereo(l, r, L[:n], lines[:n], rp, cand[:n])
    ref = orc.gn_refine_stereo(l, r, L[:n], lines[:n], rp, cand[:n])
    for k in REFINED:
        assert_bit_equal(out[k], ref[k], k)
    return out


@pytest.mark.parametrize("n", [1, 31, 32, 33, 1025])
def test_gn_refine_at_group_edges(ctx, n):
    """32 pairs per group of the persistent eight-lanes launch"""
    out = _gn_compare(ctx, n)
    if n > 32:
        assert (out["validity"] == 1).any()


@pytest.mark.parametrize("rows_below", [39, 40, 41])
def test_gn_refine_across_the_layout_switch(gctx, rows_below):
    """40 pairs with the switch to the eight-lanes layout just below, at and just above the pair count"""
    with _keys(gctx, {5: rows_below}):
        _gn_compare(gctx, 40)


# --- 3. image-size edges through the resident pipeline -----------------------------------------------------------------

SIZE_EDGES = [(32, 32), (32, 33), (33, 64), (47, 95), (64, 97), (512, 32), (32, 1280), (512, 1280)]


def _stage_same(got, exp):
    """everything but the device refinement (the chain's own refinement is inside the finalize outputs)"""
    assert got["counts"] == exp["counts"], (got["counts"], exp["counts"])
    assert_edges_equal(got["left"], exp["left"], "left edges")
    assert_edges_equal(got["right"], exp["right"], "right edges")
    for k in ("row_ptr", "col_idx", "sims", "best", "keep"):
        assert_bit_equal(got[k], exp[k], k)
    assert got["fin_counts"] == exp["fin_counts"], (got["fin_counts"], exp["fin_counts"])
    for k in ("left_index", "score", "rows"):
        assert_bit_equal(got["fin_" + k], exp["fin_" + k], "fin_" + k)
    assert_edges_equal(got["fin_right"], exp["fin_right"], "fin_right")


def _run_chain(c, o):
    c.stereo_upload(o["l"], o["r"])
    cnt = c.stereo_run(c.default_params(F_KITTI))
    out = c.stereo_fetch(cnt)
    out["counts"] = (cnt.n_left, cnt.n_right, cnt.n_pairs, cnt.n_matches)
    out["fin_counts"], fin = c.stereo_finalize(CALIB)
    out.update({"fin_" + k: v for k, v in fin.items()})
    return out


@pytest.mark.parametrize("shape", SIZE_EDGES, ids=[f"{h}x{w}" for h, w in SIZE_EDGES])
def test_image_size_edges_equal_oracle(ctx, shape):
    """the smallest image, odd sizes, strips at the context's limits and an image that fills the context exactly"""
    o, exp = _expected(*shape, refine=False)
    _stage_same(_run_chain(ctx, o), exp)
    assert exp["counts"][3] > 0                 # not vacuous: every one of these pairs keeps matches


@pytest.mark.parametrize("mode", ["strict", "hybrid"])
@pytest.mark.parametrize("shape", [(37, 101), (33, 65)], ids=["37x101", "33x65"])
def test_context_sized_exactly_to_an_odd_image(shape, mode):
    o, exp = _expected(*shape, refine=False)
    with Context(*shape, device=0, toed_mode=mode) as c:
        _stage_same(_run_chain(c, o), exp)
        _stage_same(_run_chain(c, o), exp)      # the second run of a slot takes other paths (no allocation)
    assert exp["counts"][3] > 0


# --- 4. ebvo_debug_set refuses values outside each key's range ---------------------------------------------------------

REFUSED = [(18, 513), (18, 1 << 30), (11, 65537), (12, 65537), (11, 1 << 30), (9, (1 << 20) + 1), (19, 4097),
           (10, 2), (4, 2), (7, 2), (8, 1), (8, 4), (13, 2), (14, 2), (6, 0), (99, 0), (-1, 0), (5, -1), (17, -8)]


def test_debug_set_refuses_out_of_range_values(gctx):
    o, exp = _expected(120, 200)
    for key, value in REFUSED:
        with pytest.raises(EbvoError) as ei:
            gctx.debug_set(key, value)
        assert ei.value.status == EBVO_ERR_ARG, (key, value)
    got = _chain(gctx, o["l"], o["r"])
    _same(got, exp)
    # the bounds themselves are accepted
    with _keys(gctx, {18: 512, 11: 65536, 12: 65536, 9: 1 << 20, 19: 4096}):
        _same(_chain(gctx, o["l"], o["r"]), exp)
