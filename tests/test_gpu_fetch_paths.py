"""What a caller RECEIVES from a completed pair, by every path that hands results back, against a plain numpy restatement of
the full fetch.

The pair chain's bits are pinned elsewhere (test_gpu_fullsize.py, test_gpu_launch_geometry.py compare ebvo_stereo_fetch with
the oracle).  A frame loop and bench.py read them other ways, each with kernels, layouts and slot state of its own:

  * the staged fetch (ebvo_stereo_fetch_begin / _end), 31 selections;
  * the compact fetch (ebvo_stereo_fetch_compact_begin / _end), 31 selections: (x, y) pairs, orientations, CSR, best and the
    keep flags as a bit mask, packed on the copy stream by pack_results_kernel;
  * the pushed view (EBVO_PAIR_PUSH) and the packed block (EBVO_PAIR_PACK), written by the chain's push_results_kernel.

compact_reference() / staged_reference() build what each path must deliver from ONE full fetch of the same pair, which is
compared with the oracle once per pair and TOED mode.  The pairs sit on the kernels' edges: n_pairs % 64 in {0, 1, 63}
(keep-bit words; n_pairs % 4 in {0, 1, 3} for the push kernel's 16-byte tails), the KITTI bench pair (581,657 pairs: the
grid-stride loop of pack_results_kernel, capped at 2048 x 256 threads, runs), no candidate pairs, no edges at all.
Sequences of fetches on one pair, slot reuse across sizes and refused calls that must leave the slot as it was follow.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib, synth
from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EBVO_ERR_STATE, EbvoError
from edge_based_visual_odometry_amd.api import Context, ptr
from tests import oracle as orc
from tests.test_gpu_fullsize import _oracle as _fullsize_oracle
from tests.util import assert_edges_equal

pytestmark = pytest.mark.gpu

F = synth.fundamental_for("kitti")
KITTI_HW = synth.SHAPES["kitti"]
RING_HW = (200, 320)

XY, THETA, CSR, BEST, KEEP_BITS = _lib.COMPACT_XY, _lib.COMPACT_THETA, _lib.COMPACT_CSR, _lib.COMPACT_BEST, _lib.COMPACT_KEEP_BITS
NO_SIMS, PUSH, PUSH_THETA, PACK = _lib.PAIR_NO_SIMS, _lib.PAIR_PUSH, _lib.PAIR_PUSH_THETA, _lib.PAIR_PACK

# n_pairs on a 64-pair word edge (found with the oracle over synth.stereo_pair scenes, noise seeds and sizes; disparity 10):
# name -> (scene, noise_base, h, w, n_pairs).  Asserted, so that a change to synth cannot move them off the edge unnoticed.
EDGE_PAIRS = {
    "pairs64k": (3, 0, 64, 96, 3520),
    "pairs64k+1": (3, 2, 96, 160, 12097),
    "pairs64k+63": (3, 5, 72, 120, 5759),
}
SMALL = ["ring", *EDGE_PAIRS, "flat_right", "flat"]

# submission flags: 0, NO_SIMS, PUSH, PUSH|PUSH_THETA, PACK, PACK|PUSH_THETA, the last four also with NO_SIMS
FLAG_SETS = [f | n for n in (0, NO_SIMS) for f in (0, PUSH, PUSH | PUSH_THETA, PACK, PACK | PUSH_THETA)]
# packed-path selections first: a THETA selection of a PACK pair without PUSH_THETA packs on the copy stream, and what a
# fetch of that pair reads afterwards is the business of test_pack_pair_fetched_with_and_without_theta
ALL_COMPACT = sorted(range(1, 32), key=lambda w: (bool(w & THETA), w))
ALL_STAGED = list(range(1, 32))
KITTI_COMPACT = [_lib.COMPACT_DEFAULT, KEEP_BITS, _lib.COMPACT_ALL, THETA]
KITTI_STAGED = [_lib.FETCH_DEFAULT, _lib.FETCH_ALL]


def _flag_id(flags):
    names = [n for n, b in (("no_sims", NO_SIMS), ("push", PUSH), ("pack", PACK), ("theta", PUSH_THETA)) if flags & b]
    return "+".join(names) or "plain"


@functools.lru_cache(maxsize=None)
def _images(name):
    h, w = RING_HW
    if name == "kitti":
        return synth.stereo_pair("s2", *KITTI_HW, scene=7, noise_base=0, disparity=12)
    if name in EDGE_PAIRS:
        scene, noise, h, w, _ = EDGE_PAIRS[name]
        return synth.stereo_pair("s2", h, w, scene=scene, noise_base=noise, disparity=10)
    ring = synth.stereo_pair("s2", h, w, scene=3, noise_base=0, disparity=10)    # test_gpu_ingest.py's first ring pair
    if name == "ring":
        return ring
    if name == "flat_right":
        return ring[0], np.full((h, w), 128, dtype=np.uint8)
    assert name == "flat"
    return np.full((h, w), 77, dtype=np.uint8), np.full((h, w), 128, dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    if name == "kitti":
        return _fullsize_oracle("kitti")                # shared with the full-size tests (same pair, brute force once)
    l, r = _images(name)
    L, R = orc.toed(l)["edges"], orc.toed(r)["edges"]
    rp, ci = orc.epi_candidates(L, R, orc.epipolar_lines(F, L))
    sims, best, keep, _ = orc.ncc_pairs(l, r, L, R[ci], rp)
    return dict(left=L, right=R, row_ptr=rp, col_idx=ci, sims=sims, best=best, keep=keep)


@pytest.fixture(scope="module", params=["strict", "hybrid"])
def c(request):
    ctx = Context(*KITTI_HW, device=0, toed_mode=request.param)
    ctx.set_slots(3)
    yield ctx
    ctx.close()


def _submit(c, flags, slot):
    p = c.default_params(F)
    p.reserved = flags
    c.stereo_submit(p, slot=slot)
    cnt = c.stereo_wait(slot=slot)
    return (cnt.n_left, cnt.n_right, cnt.n_pairs, cnt.n_matches)


_FULL = {}


def _full(c, name):
    """(counts, full fetch) of the pair, flags 0, compared with the oracle once per pair and TOED mode"""
    key = (c.toed_mode, name)
    if key not in _FULL:
        c.stereo_upload(*_images(name), slot=0)
        p = c.default_params(F)
        c.stereo_submit(p, slot=0)
        cnt = c.stereo_wait(slot=0)
        full = c.stereo_fetch(cnt, slot=0)
        o = _oracle(name)
        assert_edges_equal(full["left"], o["left"], f"{name}: left edges")
        assert_edges_equal(full["right"], o["right"], f"{name}: right edges")
        for k in ("row_ptr", "col_idx", "sims", "best", "keep"):
            _same_bits(full[k], o[k], f"{name}: {k} vs oracle")
        counts = (cnt.n_left, cnt.n_right, cnt.n_pairs, cnt.n_matches)
        assert counts == (len(o["left"]), len(o["right"]), len(o["col_idx"]), int(o["keep"].sum()))
        if name == "kitti":
            assert counts == (126184, 126340, 581657, 472947)
        elif name in EDGE_PAIRS:
            assert cnt.n_pairs == EDGE_PAIRS[name][4]
        elif name == "flat_right":
            assert cnt.n_left > 0 and cnt.n_right == 0 and cnt.n_pairs == 0
        elif name == "flat":
            assert counts == (0, 0, 0, 0)
        _FULL[key] = (counts, full)
    return _FULL[key]


# --- what every path must hand back ---------------------------------------------------------------------------------------
def compact_reference(full, what):
    """the compact view of a selection `what`, from a full fetch: absent arrays are None"""
    n = len(full["col_idx"])
    out = dict(n_pairs=n, n_matches=int(np.count_nonzero(full["keep"])))
    for side in ("left", "right"):
        e = full[side]
        out[side + "_xy"] = np.stack([e["x"], e["y"]], axis=1) if what & XY else None
        out[side + "_theta"] = np.ascontiguousarray(e["theta"]) if what & THETA else None
    out["row_ptr"] = full["row_ptr"] if what & CSR else None
    out["col_idx"] = full["col_idx"] if what & CSR else None
    out["best"] = full["best"] if what & BEST else None
    out["keep_bits"] = None
    if what & KEEP_BITS:
        words = 2 * ((n + 63) // 64)
        flags = np.zeros(32 * words, dtype=np.uint8)
        flags[:n] = full["keep"] != 0                   # the bits above n_pairs in the last word are zero
        out["keep_bits"] = np.packbits(flags, bitorder="little").view(np.uint32)
    return out


def staged_reference(full, what):
    f = _lib
    return dict(left=full["left"] if what & f.FETCH_EDGES else None, right=full["right"] if what & f.FETCH_EDGES else None,
                row_ptr=full["row_ptr"] if what & f.FETCH_CSR else None, col_idx=full["col_idx"] if what & f.FETCH_CSR else None,
                sims=full["sims"] if what & f.FETCH_SIMS else None, best=full["best"] if what & f.FETCH_BEST else None,
                keep=full["keep"] if what & f.FETCH_KEEP else None)


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, f"{what}: {a.dtype}{a.shape} vs {b.dtype}{b.shape}"
    u = np.dtype(f"u{a.dtype.itemsize}")
    bad = a.view(u) != b.view(u)
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ; first at {np.argwhere(bad)[0]}"


def _same_compact(v, ref, where):
    assert (v["n_pairs"], v["n_matches"]) == (ref["n_pairs"], ref["n_matches"]), where
    for k in ("left_xy", "right_xy", "left_theta", "right_theta", "row_ptr", "col_idx", "best", "keep_bits"):
        if ref[k] is None:
            assert v[k] is None, f"{where}: {k} delivered, not selected"
        else:
            assert v[k] is not None, f"{where}: {k} selected, not delivered"
            _same_bits(v[k], ref[k], f"{where}: {k}")
    if ref["keep_bits"] is not None and ref["n_pairs"] % 64:
        pad = np.unpackbits(v["keep_bits"].view(np.uint8), bitorder="little")[ref["n_pairs"]:]
        assert not pad.any(), f"{where}: padding bits above n_pairs are set"


def _same_staged(v, ref, where):
    for k in ("left", "right", "row_ptr", "col_idx", "sims", "best", "keep"):
        if ref[k] is None:
            assert v[k] is None, f"{where}: {k} delivered, not selected"
        elif k in ("left", "right"):
            assert v[k] is not None, f"{where}: {k} selected, not delivered"
            assert_edges_equal(v[k], ref[k], f"{where}: {k}")
        else:
            assert v[k] is not None, f"{where}: {k} selected, not delivered"
            _same_bits(v[k], ref[k], f"{where}: {k}")


# the views point into the slot's page-locked arena, which the next call reuses: copy them at once
def _copied(view):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in view.items()}


def _compact(c, slot, what):
    c.stereo_fetch_compact_begin(slot=slot, what=what)
    return _copied(c.stereo_fetch_compact_end(slot=slot))


def _staged(c, slot, what):
    c.stereo_fetch_begin(slot=slot, what=what)
    return _copied(c.stereo_fetch_end(slot=slot))


def _pushed(c, slot):
    return _copied(c.stereo_pushed_view(slot=slot))


def _refused(status, call):
    with pytest.raises(EbvoError) as e:
        call()
    assert e.value.status == status


def _pushed_what(flags):
    return _lib.COMPACT_ALL if flags & PUSH_THETA else _lib.COMPACT_DEFAULT


# --- the matrix: pairs x submission flags x selections ------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAG_SETS, ids=_flag_id)
@pytest.mark.parametrize("name", SMALL + ["kitti"])
def test_every_path_delivers_the_full_fetch(c, name, flags):
    """Three submissions on one slot (the third at the latest is the captured graph), every selection of the compact and the
    staged fetch after each; PUSH pairs through the pushed view too; PACK pairs once more with a forced overflow"""
    counts, full = _full(c, name)
    compact_sel, staged_sel = (KITTI_COMPACT, KITTI_STAGED) if name == "kitti" else (ALL_COMPACT, ALL_STAGED)
    compact_refs = {w: compact_reference(full, w) for w in compact_sel}
    c.stereo_upload(*_images(name), slot=1)
    graphs = c.graph_launches
    for k in range(4 if flags & PACK else 3):
        where = f"{name} {_flag_id(flags)} submission {k}"
        if k == 3:
            c.debug_set(1, 1)          # the next result is treated as overflowed: matching half re-enqueued, packed again
        assert _submit(c, flags, 1) == counts, where
        if k == 2:
            assert c.graph_launches > graphs, f"{where}: no submission was a graph launch"
        if flags & PUSH:
            _same_compact(_pushed(c, 1), compact_reference(full, _pushed_what(flags)), f"{where} pushed view")
        else:
            _refused(EBVO_ERR_STATE, lambda: c.stereo_pushed_view(slot=1))
        for w in compact_sel:
            _same_compact(_compact(c, 1, w), compact_refs[w], f"{where} compact {w}")
        for w in staged_sel:
            if (w & _lib.FETCH_SIMS) and (flags & NO_SIMS):
                _refused(EBVO_ERR_STATE, lambda: c.stereo_fetch_begin(slot=1, what=w))
            else:
                _same_staged(_staged(c, 1, w), staged_reference(full, w), f"{where} staged {w}")


# --- sequences of fetches on one completed pair ---------------------------------------------------------------------------
def _sequence(c, name, flags, steps, slot=1):
    """steps: ("compact", what) / ("staged", what) / ("pushed", None) / ("full", None), each compared as it comes"""
    counts, full = _full(c, name)
    c.stereo_upload(*_images(name), slot=slot)
    assert _submit(c, flags, slot) == counts
    for i, (kind, what) in enumerate(steps):
        where = f"{name} {_flag_id(flags)} step {i}: {kind} {what}"
        if kind == "compact":
            _same_compact(_compact(c, slot, what), compact_reference(full, what), where)
        elif kind == "staged":
            _same_staged(_staged(c, slot, what), staged_reference(full, what), where)
        elif kind == "pushed":
            _same_compact(_pushed(c, slot), compact_reference(full, _pushed_what(flags)), where)
        else:
            cnt = _lib.StereoCounts()
            cnt.n_left, cnt.n_right, cnt.n_pairs, cnt.n_matches = counts
            out = c.stereo_fetch(cnt, slot=slot)
            _same_staged(out, staged_reference(full, _lib.FETCH_ALL), where)


def test_pack_pair_fetched_with_and_without_theta(c):
    """A PACK pair without PUSH_THETA asked for orientations packs on the copy stream, into the staging the chain packed into:
    the fetches after it must not read that staging as the chain's block"""
    steps = [("compact", _lib.COMPACT_ALL), ("compact", _lib.COMPACT_DEFAULT), ("compact", KEEP_BITS), ("compact", _lib.COMPACT_ALL)]
    for name in ("ring", "kitti"):
        _sequence(c, name, PACK, steps)


def test_pack_theta_pair_sequence(c):
    steps = [("compact", _lib.COMPACT_DEFAULT), ("compact", _lib.COMPACT_ALL), ("compact", THETA)]
    for name in ("ring", "kitti"):
        _sequence(c, name, PACK | PUSH_THETA, steps)


@pytest.mark.parametrize("flags", [0, PACK, PACK | PUSH_THETA], ids=_flag_id)
def test_compact_staged_compact_full(c, flags):
    steps = [("compact", _lib.COMPACT_DEFAULT), ("staged", _lib.FETCH_ALL), ("compact", _lib.COMPACT_DEFAULT), ("full", None)]
    _sequence(c, "ring", flags, steps)


@pytest.mark.parametrize("flags", [PUSH, PUSH | PUSH_THETA], ids=_flag_id)
def test_pushed_view_around_a_compact_fetch(c, flags):
    steps = [("pushed", None), ("compact", _lib.COMPACT_ALL), ("pushed", None), ("staged", _lib.FETCH_ALL), ("pushed", None)]
    _sequence(c, "ring", flags, steps)


def test_slot_reuse_across_sizes(c):
    """KITTI, 200x320, KITTI again on one slot, all PACK: whole arrays, so that stale bytes of the larger pair would show"""
    steps = [("compact", _lib.COMPACT_DEFAULT), ("staged", _lib.FETCH_ALL), ("compact", _lib.COMPACT_ALL)]
    for name in ("kitti", "ring", "kitti"):
        _sequence(c, name, PACK, steps, slot=2)


# --- refused calls change nothing ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _other_pair():
    # kept alive for the module: a library that took the refused upload half-way would still read existing memory
    return synth.stereo_pair("s2", *RING_HW, scene=4, noise_base=20, disparity=10)   # test_gpu_ingest.py's second ring pair


def _upload_async(c, slot, h, w, stride_left, stride_right):
    l, r = _other_pair()
    return c.lib.ebvo_stereo_upload_async(c._ctx, slot, ptr(l), ptr(r), h, w, stride_left, stride_right)


def _upload_slot(c, slot, h, w, stride_left, stride_right):
    l, r = _other_pair()
    return c.lib.ebvo_stereo_upload_slot(c._ctx, slot, ptr(l), ptr(r), h, w, stride_left, stride_right)


def _submit_raw(c, flags):
    p = c.default_params(F)
    p.reserved = flags
    return c.lib.ebvo_stereo_submit(c._ctx, 2, C.byref(p))


H, W = RING_HW
# id -> (flags of the resident pair, the call on slot 2, its status).  Every argument here is refused on the host.
REFUSED = {
    "upload_async_stride_left": (0, lambda c: _upload_async(c, 2, H, W, W - 1, W), EBVO_ERR_ARG),
    "upload_async_stride_right": (0, lambda c: _upload_async(c, 2, H, W, W, W - 1), EBVO_ERR_ARG),
    "upload_async_h31": (0, lambda c: _upload_async(c, 2, 31, W, W, W), EBVO_ERR_ARG),
    "upload_async_bad_slot": (0, lambda c: _upload_async(c, 3, H, W, W, W), EBVO_ERR_ARG),
    "upload_slot_stride_right": (0, lambda c: _upload_slot(c, 2, H, W, W, W - 1), EBVO_ERR_ARG),
    "submit_push_and_pack": (PACK, lambda c: _submit_raw(c, PUSH | PACK), EBVO_ERR_ARG),
    "fetch_what_0": (0, lambda c: c.lib.ebvo_stereo_fetch_begin(c._ctx, 2, 0), EBVO_ERR_ARG),
    "fetch_what_32": (0, lambda c: c.lib.ebvo_stereo_fetch_begin(c._ctx, 2, 32), EBVO_ERR_ARG),
    "compact_what_0": (PACK, lambda c: c.lib.ebvo_stereo_fetch_compact_begin(c._ctx, 2, 0), EBVO_ERR_ARG),
    "compact_what_32": (PACK, lambda c: c.lib.ebvo_stereo_fetch_compact_begin(c._ctx, 2, 32), EBVO_ERR_ARG),
    "fetch_sims_after_no_sims": (NO_SIMS, lambda c: c.lib.ebvo_stereo_fetch_begin(c._ctx, 2, _lib.FETCH_SIMS), EBVO_ERR_STATE),
}


@pytest.mark.parametrize("case", list(REFUSED))
def test_refused_call_changes_nothing(c, case):
    flags, call, status = REFUSED[case]
    counts, full = _full(c, "ring")
    staged_what = _lib.FETCH_DEFAULT if flags & NO_SIMS else _lib.FETCH_ALL

    def results_unchanged(where):
        _same_compact(_compact(c, 2, _lib.COMPACT_ALL), compact_reference(full, _lib.COMPACT_ALL), where)
        _same_staged(_staged(c, 2, staged_what), staged_reference(full, staged_what), where)

    c.stereo_upload(*_images("ring"), slot=2)
    assert _submit(c, flags, 2) == counts
    assert call(c) == status, case
    results_unchanged(f"{case}: results after the refused call")
    assert _submit(c, flags, 2) == counts, f"{case}: counts of the re-submitted pair"   # the images are still resident
    results_unchanged(f"{case}: results of the re-submitted pair")


def test_empty_pair_on_a_fresh_slot():
    """A pair without edges fetched before the slot has ever held results: selected arrays are empty, not NULL"""
    l, r = (np.full((64, 96), v, dtype=np.uint8) for v in (77, 128))
    with Context(64, 96, device=0) as fresh:
        fresh.stereo_upload(l, r)
        assert _submit(fresh, 0, 0) == (0, 0, 0, 0)
        v = _compact(fresh, 0, _lib.COMPACT_XY)
        assert v["left_xy"].shape == v["right_xy"].shape == (0, 2) and v["row_ptr"] is None
        v = _staged(fresh, 0, _lib.FETCH_EDGES)
        assert len(v["left"]) == len(v["right"]) == 0 and v["row_ptr"] is None
