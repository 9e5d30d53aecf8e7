"""The two photometric Gauss-Newton refinements (ebvo_gn_refine_stereo, ebvo_stereo_refine, the refinement inside
ebvo_stereo_finalize; ebvo_gn_refine_temporal) on the hand-over between the stereo layouts, on size edges and on extreme
content -- validity, iters, alpha, score, refined_xy and confidence (temporal: validity, iters, disp, score) against the
oracle, bit for bit, with no tolerance anywhere.  Every input is numpy and oracle output (tests/gn_cases.py;
tests/test_gn_cases.py re-derives each case's condition without a GPU); no device output is passed to the oracle.  The
refinement does not depend on the detector mode, so one context of this file's own is used: the developer keys set here never
reach the session context, and every one of them is restored in a finally.

The developer keys of ebvo_debug_set that steer the stereo refinement (refine_gn_stereo_enqueue):
  5   rows_below (default 65536).  While more than rows_below pairs are active, an iteration is one launch of gn_iter_kernel
      (one thread per pair); then ONE gn_rows_persistent_kernel (eight lanes per pair) runs every remaining pair to its end.
      That kernel finds its own starting list -- the last non-empty counts[it] -- and returns when that list holds more than
      rows_below pairs (the thread layout ran it).  At the default no problem below ~65 k pairs ever runs the thread layout,
      the mixed path, the equality n_active == rows_below, or "the thread layout ran the last list".
  9   most workgroups of the persistent launch (default 1024; 32 eight-lane groups each).  At 1, 32 groups walk the whole list
      (group g: g, g + 32, ...): dozens of pairs per group where the default gives each group one.
  4   1 = the thread layout for every iteration;  7   1 = the row layout as a launch per iteration (mode 2 of
      gn_iter_rows_kernel when thread-layout launches ran before it);  8   waves per SIMD of the persistent kernel (2 | 3);
  23  cap on the grids of the finalize chain: with key 5 low it reaches gn_iter_kernel's grid-stride loop and the alternating
      scratch words of block_append_slot.
What the inputs reach: steps_pair fills both 11-bit gradient fields of gn_pack_kernel's records (+-1020, every sign
combination, pixels 0 and 255); half_flat_pair stops pairs on H < 1e-8 (validity 2) at iterations 0 .. 18, so outputs are
written by an iteration that is not the first; the size cases sit around 8 lanes, 32 groups and 256 threads per block, 32 left
edges per block of gn_left_kernel, 64 columns per block of gn_pack_kernel, with empty rows at either end, the smallest
accepted image and row-strided images."""
import contextlib

import numpy as np
import pytest

from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, GnParams, ptr
from edge_based_visual_odometry_amd.api import Context
from tests import finalize_cases as fc
from tests import gn_cases as gc
from tests import oracle as orc
from tests import test_gpu_finalize_edges as fe
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu

KEY_DEFAULTS = {4: 0, 5: 0, 7: 0, 8: 2, 9: 0, 23: 0}
STEREO_FIELDS = ("validity", "iters", "alpha", "score", "refined_xy", "confidence")
TEMPORAL_FIELDS = ("validity", "iters", "disp", "score")
LAYOUTS = {"rows": 0, "threads": 1}                     # developer key 4


@pytest.fixture(scope="module")
def gctx():
    c = Context(128, 256, device=0)
    yield c
    c.close()


@contextlib.contextmanager
def keys(c, **kv):
    """keys(c, k5=1, k9=2): developer keys for the block, all of this file's keys back at their defaults after it"""
    try:
        for k, v in kv.items():
            c.debug_set(int(k[1:]), v)
        yield
    finally:
        for k, v in KEY_DEFAULTS.items():
            c.debug_set(k, v)


def stereo(c, case, **kw):
    return c.gn_refine_stereo(case["l"], case["r"], case["L"], case["lines"], case["rp"], case["cand"], **kw)


def temporal(c, case, **kw):
    return c.gn_refine_temporal(case["kf_img"], case["cf_img"], case["kf"], case["cf"], case["init"], **kw)


def same(out, ref, fields, what):
    assert set(fields) <= set(out)
    for k in fields:
        assert_bit_equal(out[k], ref[k], f"{what}: {k}")


def check_stereo(c, case, what, ref=None, **kw):
    ref = gc.stereo_ref(case, **kw) if ref is None else ref
    same(stereo(c, case, **kw), ref, STEREO_FIELDS, what)
    return ref


def check_temporal(c, case, what, ref=None, **kw):
    ref = gc.temporal_ref(case, **kw) if ref is None else ref
    same(temporal(c, case, **kw), ref, TEMPORAL_FIELDS, what)
    return ref


# --- A. stereo layout hand-over -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["all", "all-1", "equal", "equal-1", "one"])
def test_hand_over_on_the_profile(gctx, which):
    case, ref = gc.half_flat_case(), gc.named_ref("half_flat")
    thr, _ = gc.thresholds(gc.profile(ref, gc.GN_DEFAULT["max_iter"]))
    k5 = thr[which]
    for k9 in (0, 1, 2, 7):
        for k8 in (2, 3):
            with keys(gctx, k5=k5, k9=k9, k8=k8):
                check_stereo(gctx, case, f"key 5 = {k5} ({which}), key 9 = {k9}, key 8 = {k8}", ref)
    with keys(gctx, k5=k5, k7=1):
        check_stereo(gctx, case, f"key 5 = {k5} ({which}), key 7 = 1", ref)
    check_stereo(gctx, case, f"defaults after key 5 = {k5}", ref)


@pytest.mark.parametrize("name", ["half_flat", "steps"])
def test_hand_over_under_parameters(gctx, name):
    """rows_below = n_pairs - 1, so the thread layout runs iteration 0 and every later one that enters with all pairs:
    tol = 0 on the step pair keeps all 20 there and the persistent launch must leave every output alone; tol = inf finishes
    every pair in iteration 0; max_iter = 1 has no second list"""
    case = getattr(gc, name + "_case")()
    k5 = len(case["cand"]) - 1
    for kw in (dict(tol=0.0), dict(tol=np.inf), dict(max_iter=1), dict(max_iter=2)):
        ref = gc.named_ref(name, **kw)
        for k9 in (0, 1):
            with keys(gctx, k5=k5, k9=k9):
                check_stereo(gctx, case, f"{name} {kw} key 5 = {k5}, key 9 = {k9}", ref, **kw)
        with keys(gctx, k5=k5, k7=1):
            check_stereo(gctx, case, f"{name} {kw} key 5 = {k5}, key 7 = 1", ref, **kw)
        check_stereo(gctx, case, f"{name} {kw} defaults", ref, **kw)


def test_resident_refine_hand_over(gctx):
    """ebvo_stereo_refine on the resident 96 x 160 pair: n_pairs counts the un-kept pairs too, so with rows_below between the
    kept count and n_pairs every thread-layout launch is made and returns at once"""
    cnt = fe.run_pair(gctx, "default")                            # (asserts the device's first stage equal to the oracle's)
    s = fc.stage1("default")
    L, R, lines = fc.edges("default")
    keep = s["keep"].astype(bool)
    kept, n_pairs = int(keep.sum()), len(keep)
    assert 0 < kept < n_pairs - 2 and (cnt.n_pairs, cnt.n_matches) == (n_pairs, kept)
    l, r = fc.images("default")
    xy = np.stack([R["x"][s["col_idx"]], R["y"][s["col_idx"]]], 1)
    from tests import oracle_chain
    ref = orc.gn_refine_stereo(l, r, L, lines, oracle_chain.filter_rows(s["row_ptr"], keep), xy[keep])
    for k5 in ((kept + n_pairs) // 2, kept // 2, kept, 0):
        for k9 in (0, 1):
            with keys(gctx, k5=k5, k9=k9):
                dev = gctx.stereo_refine(cnt)
            what = f"resident, key 5 = {k5}, key 9 = {k9}"
            same({k: dev[k][keep] for k in STEREO_FIELDS}, ref, STEREO_FIELDS, what)
            assert (dev["validity"][~keep] == 255).all() and np.isnan(dev["score"][~keep]).all(), what
            assert np.isnan(dev["confidence"][~keep]).all() and not dev["iters"][~keep].any() and not dev["alpha"][~keep].any(), what
            assert_bit_equal(dev["refined_xy"][~keep], xy[~keep], what + ": unrefined locations")


@pytest.mark.parametrize("which", ["one", "mid"])
def test_finalize_chain_hand_over(gctx, which):
    """the refinement inside ebvo_stereo_finalize with the thread layout running down to k5 active pairs, under capped grids:
    gn_iter_kernel's grid-stride loop takes many turns, block_append_slot's scratch words alternate.  k5 = 1 keeps all 20
    iterations in the thread layout; the other value is the active count of the chain's own refinement on entering a mid
    iteration (tests/gn_cases.py: chain_thresholds, from the oracle), so the hand-over falls on the equality there."""
    k5 = dict(zip(("one", "mid"), gc.chain_thresholds()[0]))[which]
    fe.run_pair(gctx, "default")
    n_bnb = fc.chain("default")["counts"]["n_bnb"]
    assert n_bnb > 3 * 256 * 4                                     # more than one turn per block under caps 1 and 3

    def stale():
        """The chain reads only the refined locations, and nothing resets those between runs: after a run on the same pair
        they already hold the right values, and a launch that wrongly skipped its pairs would go unseen.  A chain of ONE
        iteration (compared with the oracle's, too) leaves other locations there first."""
        fe.finalize(gctx, "default", what="one iteration", max_iter=1)

    for k23 in (0, 1, 3):
        stale()
        with keys(gctx, k5=k5, k23=k23):
            counts, _ = fe.finalize(gctx, "default", what=f"key 5 = {k5}, key 23 = {k23}")
    stale()
    with keys(gctx, k5=k5, k9=1):
        fe.finalize(gctx, "default", what=f"key 5 = {k5}, key 9 = 1")
    stale()
    with keys(gctx, k5=k5, k9=1, k23=3):
        fe.finalize(gctx, "default", what=f"key 5 = {k5}, key 9 = 1, key 23 = 3", sift=True)
    assert counts["n_final"] > 1000
    stale()
    fe.finalize(gctx, "default", what="defaults")


# --- B. size edges ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_stereo_pair_and_edge_counts(gctx, layout):
    base = gc.s2_case()
    cases = {f"{n} pairs": gc.sub_case(base, n_pairs=n) for n in gc.PAIR_COUNTS}
    cases.update({f"{n} left edges": gc.sub_case(base, nL=n) for n in gc.LEFT_COUNTS})
    cases.update(gc.row_shape_cases())
    with keys(gctx, k4=LAYOUTS[layout]):
        for what, case in cases.items():
            check_stereo(gctx, case, f"{layout}, {what}")


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_temporal_item_counts(gctx, layout):
    base = gc.temporal_s2_case()
    with keys(gctx, k4=LAYOUTS[layout]):
        for n in gc.PAIR_COUNTS:
            check_temporal(gctx, gc.temporal_sub(base, n), f"{layout}, {n} items")


@pytest.mark.parametrize("shape", gc.SMALL_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_small_and_strided_images(gctx, layout, shape):
    case, tcase = gc.small_case(*shape), gc.temporal_small_case(*shape)
    with keys(gctx, k4=LAYOUTS[layout]):
        ref = check_stereo(gctx, case, f"{layout}, {shape}")
        check_stereo(gctx, dict(case, l=gc.strided(case["l"]), r=gc.strided(case["r"], pad=3)), f"{layout}, {shape}, strided", ref)
        ref = check_temporal(gctx, tcase, f"{layout}, {shape}")
        strided = dict(tcase, kf_img=gc.strided(tcase["kf_img"], pad=5), cf_img=gc.strided(tcase["cf_img"]))
        check_temporal(gctx, strided, f"{layout}, {shape}, strided", ref)


# --- C. content ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_step_images_and_borders(gctx, layout):
    """gradient fields at +-1020 in every sign combination, patches clamped at the four borders and corners, finite
    coordinates at +-1e6 and +-1e15 (stereo: these clamp onto a constant patch and stop at once with validity 2, so they
    check the clamp alone; the temporal starts there iterate on, gn_cases.border_points)"""
    case, tcase = gc.with_border_candidates(gc.steps_case()), gc.with_border_starts(gc.temporal_steps_case())
    with keys(gctx, k4=LAYOUTS[layout]):
        for kw in ({}, dict(huber_delta=40.0)):
            check_stereo(gctx, case, f"{layout}, steps {kw}", **kw)
            check_temporal(gctx, tcase, f"{layout}, temporal steps {kw}", **kw)
    if layout == "rows":
        with keys(gctx, k7=1):
            check_stereo(gctx, case, "rows per iteration, steps")
            check_temporal(gctx, tcase, "rows per iteration, temporal steps")


# --- D. parameters ------------------------------------------------------------------------------------------------------
PARAMS = [dict(max_iter=m) for m in (1, 2, 3, 64)] + [dict(tol=t) for t in (0.0, 1e-12, np.inf)] + [dict(huber_delta=d) for d in (1e-3, np.inf)]


@pytest.mark.parametrize("name", ["s2", "half_flat"])
def test_parameters(gctx, name):
    case, tcase = getattr(gc, name + "_case")(), getattr(gc, f"temporal_{name}_case")()
    for kw in PARAMS:
        check_stereo(gctx, case, f"{name} {kw}", gc.named_ref(name, **kw), **kw)
        check_temporal(gctx, tcase, f"temporal {name} {kw}", gc.named_ref("temporal_" + name, **kw), **kw)


REFUSED = [dict(max_iter=0), dict(tol=-1.0), dict(tol=np.nan), dict(huber_delta=0.0), dict(huber_delta=-3.0), dict(huber_delta=np.nan)]


def test_refused_parameters_write_nothing(gctx):
    case, tcase = gc.sub_case(gc.s2_case(), n_pairs=33), gc.temporal_sub(gc.temporal_s2_case(), 33)
    l, r = case["l"], case["r"]
    h, w = l.shape
    L, lines, rp, cand = (np.ascontiguousarray(case[k]) for k in ("L", "lines", "rp", "cand"))
    kf, cf, init = (np.ascontiguousarray(tcase[k]) for k in ("kf", "cf", "init"))
    lib = gctx.lib
    for kw in REFUSED:
        p = GnParams()
        lib.ebvo_gn_default_params(p)
        for k, v in kw.items():
            setattr(p, k, v)
        outs = [np.full(33, -4.25), np.full(33, 7.5), np.full(33, 0.125), np.full(33, 77, np.uint8), np.full(33, -9, np.int32),
                np.full((33, 2), 3.5)]
        before = [a.tobytes() for a in outs]
        rc = lib.ebvo_gn_refine_stereo(gctx._ctx, ptr(l), ptr(r), h, w, l.strides[0], r.strides[0], ptr(L), len(L), ptr(lines), ptr(rp),
                                       ptr(cand), p, *[ptr(a) for a in outs])
        assert rc == EBVO_ERR_ARG and [a.tobytes() for a in outs] == before, kw
        ki, ci = tcase["kf_img"], tcase["cf_img"]
        outs = [np.full((33, 2), 3.5), np.full(33, 7.5), np.full(33, 77, np.uint8), np.full(33, -9, np.int32)]
        before = [a.tobytes() for a in outs]
        rc = lib.ebvo_gn_refine_temporal(gctx._ctx, ptr(ki), ptr(ci), h, w, ki.strides[0], ci.strides[0], ptr(kf), ptr(cf), ptr(init), 33,
                                         p, *[ptr(a) for a in outs])
        assert rc == EBVO_ERR_ARG and [a.tobytes() for a in outs] == before, kw
    check_stereo(gctx, case, "after the refusals")
    check_temporal(gctx, tcase, "after the refusals")
