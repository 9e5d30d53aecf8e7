"""The stage-wise host-array calls take slot 0 through host_slot(): they give the resident pair up, reuse its named buffers and
run inside a HostCall that waits for their copies on every return.  Every comparison here is against the same call on a fresh
context, bit for bit (the other GPU tests pin those results to the oracles):

  interleaved calls          the nineteen entry points on one context with lists of 3, 300, 1, 65, 0 and 3 elements: a 256-thread
                             block boundary, a 64-lane boundary, the empty list, a smaller call in buffers a larger one grew
  capacity, then reuse       ebvo_toed / ebvo_toed_pair / ebvo_epi_candidates[_staged] one short of room: counts and row_ptr
                             written, lists untouched, every input overwritten at once, then the same call with room
  slot in flight             every call refused while a submitted pair runs; the pair's results are those of an undisturbed run
  what happens to the pair   which forms of which call leave ebvo_stereo_fetch_slot working afterwards (the table is written
                             out below from the documented order of refusals, not computed)
  optional outputs           each optional output left out, one at a time

The pair is synth's "s2" at 96 x 160; lists are its own TOED edges cut to length, with two candidates per row."""
import ctypes as C
import functools

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib, synth
from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EBVO_ERR_CAPACITY, EBVO_ERR_STATE, EBVO_OK, EDGE_DTYPE, ptr
from edge_based_visual_odometry_amd.api import Context

pytestmark = pytest.mark.gpu

H, W = 96, 160
CAP = H * W
NMAX = 300
LENGTHS = (3, 300, 1, 65, 0, 3)
SENTINEL = 0x5A     # what every output holds before a call
UNPINNED = ("t_conv", "t_nms")     # device times: returned, never compared
KITTI = synth.CALIB["kitti"]
K33 = np.array([[KITTI["K"][0], 0.0, KITTI["K"][2]], [0.0, KITTI["K"][1], KITTI["K"][3]], [0.0, 0.0, 1.0]])
CALIB = (K33, K33, KITTI["R21"], KITTI["T21"])
F21 = synth.fundamental_21(KITTI["K"], KITTI["K"], KITTI["R21"], KITTI["T21"])


def blank(shape, dtype):
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8)[...] = SENTINEL
    return a


def arg(out, key, skip):
    return None if key in skip else ptr(out[key])


def at(a, ctype):
    return a.ctypes.data_as(C.POINTER(ctype))


def gn_params(c):
    p = _lib.GnParams()
    c.lib.ebvo_gn_default_params(C.byref(p))
    return p


# ---- inputs ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _images():
    return synth.stereo_pair("s2", H, W)


@functools.lru_cache(maxsize=None)
def _edges():
    """the pair's own TOED edges, from a context that makes no other call"""
    left, right = _images()
    with Context(H, W, device=0) as c:
        rc, out = toed_pair(c, dict(left=left, right=right, hw=np.array([H, W])))
    assert rc == EBVO_OK
    return out["out_left"][:out["n_kept"][0]].copy(), out["out_right"][:out["n_kept"][1]].copy()


@functools.lru_cache(maxsize=None)
def _tables():
    rng = np.random.default_rng(7)
    return dict(patches=(rng.random((4, 2 * NMAX, 98)) * 255).astype(np.float32), scores=rng.random(2 * NMAX),
                desc=rng.integers(0, 256, (3 * NMAX, 256)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _scene(n):
    left, right = _images()
    EL, ER = _edges()
    assert len(EL) >= n and len(ER) >= 1
    T = _tables()
    L, R, cand = EL[:n], np.resize(ER, n), np.resize(ER, 2 * n)     # two candidates per row
    lines = np.zeros((n, 3))
    F9 = np.ascontiguousarray(F21, dtype=np.float64).reshape(9)
    assert _lib.load_library().ebvo_epipolar_lines(ptr(F9), ptr(L), n, ptr(lines)) == EBVO_OK
    s = dict(left=left, right=right, hw=np.array([H, W]), L=L, R=R, lines=lines, row_ptr=2 * np.arange(n + 1, dtype=np.int32),
             cand=cand, cand_xy=np.stack([cand["x"], cand["y"]], axis=1), scores=T["scores"][:2 * n],
             pA=T["patches"][0, :n, :49], pB=T["patches"][1, :n, :49], qkfL=T["patches"][0, :n], qkfR=T["patches"][1, :n],
             qcfL=T["patches"][2, :n], qcfR=T["patches"][3, :n], desc_l=T["desc"][:n], desc_c=T["desc"][n:3 * n],
             init_disp=np.full((n, 2), 0.25), K4=np.array([100.0, 100.0, 80.0, 48.0]),
             dist=np.array([-0.1, 0.02, 0.001, -0.001, 0.0]))
    return {k: np.ascontiguousarray(v) for k, v in s.items()}


def scene(n):
    """a private copy of the inputs of every call for lists of n"""
    return {k: v.copy() for k, v in _scene(n).items()}


def full_scene():
    """every left edge against every right edge (the lists of the capacity tests)"""
    EL, ER = _edges()
    return scene(min(len(EL), len(ER), NMAX))


def mask_rows(a, rp, cnt):
    """the slots of a row past its count are unspecified: back to the sentinel"""
    for i in range(len(cnt)):
        a[rp[i] + cnt[i]:rp[i + 1]].view(np.uint8)[...] = SENTINEL


# ---- the nineteen entry points: (context, scene, what to leave out) -> (return code, outputs) -----------------------------
def toed(c, s, skip=(), cap=CAP):
    h, w = (int(v) for v in s["hw"])
    out = dict(out=blank(cap, EDGE_DTYPE), all4=blank((CAP, 4), np.float64), n_kept=blank(1, np.int32), n_total=blank(1, np.int32),
               t_conv=blank(1, np.float64), t_nms=blank(1, np.float64))
    rc = c.lib.ebvo_toed(c._ctx, ptr(s["left"]), h, w, w, arg(out, "out", skip), 0 if "out" in skip else cap, at(out["n_kept"], C.c_int),
                         at(out["n_total"], C.c_int), arg(out, "all4", skip), CAP,
                         None if "t_conv" in skip else at(out["t_conv"], C.c_double),
                         None if "t_nms" in skip else at(out["t_nms"], C.c_double))
    return rc, out


def toed_pair(c, s, skip=(), cap=CAP):
    h, w = (int(v) for v in s["hw"])
    out = dict(out_left=blank(cap, EDGE_DTYPE), out_right=blank(cap, EDGE_DTYPE), n_kept=blank(2, np.int32), n_total=blank(2, np.int32))
    rc = c.lib.ebvo_toed_pair(c._ctx, ptr(s["left"]), ptr(s["right"]), h, w, w, w, arg(out, "out_left", skip), arg(out, "out_right", skip),
                              cap, at(out["n_kept"], C.c_int), at(out["n_total"], C.c_int))
    return rc, out


def _epi(c, s, skip, cap, staged):
    """both passes as the wrappers make them (cap None: the first pass sizes the list); cap given: the second pass alone"""
    n, p = len(s["L"]), c.default_params()
    out = dict(row_ptr=blank(n + 1, np.int32), n_pairs=blank(1, np.int64))

    def call(col, orient, room):
        head = (c._ctx, ptr(s["L"]), n, ptr(s["R"]), len(s["R"]), ptr(s["lines"]), p.epi_thr, p.max_disp, p.orient_thr_deg)
        tail = (room, at(out["n_pairs"], C.c_int64))
        if staged:
            return c.lib.ebvo_epi_candidates_staged(*head, ptr(out["row_ptr"]), col, orient, *tail)
        return c.lib.ebvo_epi_candidates(*head, p.stage_mask, ptr(out["row_ptr"]), col, *tail)

    if cap is None:
        rc = call(None, None, 0)
        if rc != EBVO_OK:
            return rc, out
        cap = int(out["n_pairs"][0])
    out["col_idx"] = blank(cap, np.int32)
    if staged:
        out["orient_ok"] = blank(cap, np.uint8)
    if "col_idx" in skip:     # legal without room only: the sizing pass again
        return call(None, None, 0), out
    return call(ptr(out["col_idx"]), ptr(out["orient_ok"]) if staged else None, cap), out


def epi_candidates(c, s, skip=(), cap=None):
    return _epi(c, s, skip, cap, False)


def epi_candidates_staged(c, s, skip=(), cap=None):
    return _epi(c, s, skip, cap, True)


def sobel_gradients(c, s, skip=()):
    h, w = (int(v) for v in s["hw"])
    out = dict(gx=blank((H, W), np.float32), gy=blank((H, W), np.float32))
    return c.lib.ebvo_sobel_gradients(c._ctx, ptr(s["left"]), h, w, w, ptr(out["gx"]), ptr(out["gy"])), out


def gn_refine_stereo(c, s, skip=()):
    h, w = (int(v) for v in s["hw"])
    n, m = len(s["L"]), len(s["cand"])
    out = dict(alpha=blank(m, np.float64), score=blank(m, np.float64), confidence=blank(m, np.float64), validity=blank(m, np.uint8),
               iters=blank(m, np.int32), refined_xy=blank((m, 2), np.float64))
    rc = c.lib.ebvo_gn_refine_stereo(c._ctx, ptr(s["left"]), ptr(s["right"]), h, w, w, w, ptr(s["L"]), n, ptr(s["lines"]),
                                     ptr(s["row_ptr"]), ptr(s["cand_xy"]), C.byref(gn_params(c)), *(arg(out, k, skip) for k in out))
    return rc, out


def edge_patches(c, s, skip=()):
    h, w = (int(v) for v in s["hw"])
    out = dict(patches=blank((len(s["L"]), 98), np.float32))
    return c.lib.ebvo_edge_patches(c._ctx, ptr(s["left"]), h, w, w, ptr(s["L"]), len(s["L"]), ptr(out["patches"])), out


def ncc_pairs(c, s, skip=()):
    h, w = (int(v) for v in s["hw"])
    n, m = len(s["L"]), len(s["cand"])
    out = dict(left_patches=blank((n, 98), np.float32), sims=blank((m, 4), np.float64), best=blank(m, np.float64), keep=blank(m, np.uint8))
    rc = c.lib.ebvo_ncc_pairs(c._ctx, ptr(s["left"]), ptr(s["right"]), h, w, w, w, ptr(s["L"]), n, None if "Rc" in skip else ptr(s["cand"]),
                              ptr(s["row_ptr"]), c.default_params().ncc_thr, *(arg(out, k, skip) for k in out))
    return rc, out


def ncc_patches(c, s, skip=()):
    n = len(s["pA"])
    out = dict(sim=blank(n, np.float64))
    return c.lib.ebvo_ncc_patches(c._ctx, ptr(s["pA"]), ptr(s["pB"]), n, ptr(out["sim"])), out


def ncc_quads(c, s, skip=()):
    n = len(s["qkfL"])
    out = dict(sim_left=blank(n, np.float64), sim_right=blank(n, np.float64), keep=blank(n, np.uint8))
    rc = c.lib.ebvo_ncc_quads(c._ctx, ptr(s["qkfL"]), ptr(s["qkfR"]), ptr(s["qcfL"]), ptr(s["qcfR"]), n, 0.5, ptr(out["sim_left"]),
                              ptr(out["sim_right"]), ptr(out["keep"]))
    return rc, out


def gn_refine_temporal(c, s, skip=()):
    h, w = (int(v) for v in s["hw"])
    n = len(s["L"])
    out = dict(disp=blank((n, 2), np.float64), score=blank(n, np.float64), validity=blank(n, np.uint8), iters=blank(n, np.int32))
    rc = c.lib.ebvo_gn_refine_temporal(c._ctx, ptr(s["left"]), ptr(s["right"]), h, w, w, w, ptr(s["L"]), ptr(s["R"]), ptr(s["init_disp"]), n,
                                       C.byref(gn_params(c)), *(arg(out, k, skip) for k in out))
    return rc, out


def _row_select(c, s, call):
    n, m = len(s["L"]), len(s["cand"])
    out = dict(new_count=blank(n, np.int32), order=blank(m, np.int32))
    rp = s["row_ptr"].copy()
    rc = call(ptr(out["new_count"]), ptr(out["order"]))
    if rc == EBVO_OK:
        mask_rows(out["order"], rp, out["new_count"])
    return rc, out


def bnb_test(c, s, skip=()):
    return _row_select(c, s, lambda cnt, order: c.lib.ebvo_bnb_test(c._ctx, ptr(s["row_ptr"]), len(s["L"]), ptr(s["scores"]), 0.8, 1, cnt,
                                                                    order))


def keep_best(c, s, skip=()):
    return _row_select(c, s, lambda cnt, order: c.lib.ebvo_keep_best(c._ctx, ptr(s["row_ptr"]), len(s["L"]), ptr(s["scores"]), cnt, order))


def epipolar_shift(c, s, skip=()):
    out = dict(shifted=blank(len(s["cand"]), EDGE_DTYPE))
    rc = c.lib.ebvo_epipolar_shift(c._ctx, ptr(s["cand"]), ptr(s["lines"]), ptr(s["row_ptr"]), len(s["L"]), ptr(out["shifted"]))
    return rc, out


def cluster_rows(c, s, skip=()):
    n, m = len(s["L"]), len(s["cand"])
    out = dict(new_count=blank(n, np.int32), centres=blank(m, EDGE_DTYPE), cluster_of=blank(m, np.int32))
    rp = s["row_ptr"].copy()
    rc = c.lib.ebvo_cluster_rows(c._ctx, ptr(s["cand"]), ptr(s["row_ptr"]), n, 0, 0, *(ptr(out[k]) for k in out))
    if rc == EBVO_OK:
        mask_rows(out["centres"], rp, out["new_count"])
    return rc, out


def finalize_pairs(c, s, skip=()):
    n = len(s["L"])
    out = dict(out16=blank((n, 16), np.float64))
    return c.lib.ebvo_finalize_pairs(c._ctx, C.byref(c._calib(CALIB)), ptr(s["L"]), ptr(s["R"]), n, ptr(out["out16"])), out


def sift_descriptors(c, s, skip=()):
    h, w = (int(v) for v in s["hw"])
    n = len(s["L"])
    out = dict(desc=blank((n, 256), np.float32))
    return c.lib.ebvo_sift_descriptors(c._ctx, ptr(s["left"]), h, w, w, ptr(s["L"]), n, ptr(out["desc"])), out


def sift_min_distances(c, s, skip=()):
    out = dict(dist=blank(len(s["desc_c"]), np.float64))
    rc = c.lib.ebvo_sift_min_distances(c._ctx, ptr(s["desc_l"]), len(s["desc_l"]), ptr(s["desc_c"]), ptr(s["row_ptr"]), ptr(out["dist"]))
    return rc, out


def undistort(c, s, skip=()):
    """into rows 16 bytes wider than the image: the padding keeps its sentinels"""
    h, w = (int(v) for v in s["hw"])
    out = dict(out=blank((H, W + 16), np.uint8))
    return c.lib.ebvo_undistort(c._ctx, ptr(s["left"]), h, w, w, ptr(s["K4"]), ptr(s["dist"]), 5, ptr(out["out"]), W + 16), out


CALLS = dict(toed=toed, toed_pair=toed_pair, epi_candidates=epi_candidates, epi_candidates_staged=epi_candidates_staged,
             sobel_gradients=sobel_gradients, gn_refine_stereo=gn_refine_stereo, edge_patches=edge_patches, ncc_pairs=ncc_pairs,
             ncc_patches=ncc_patches, ncc_quads=ncc_quads, gn_refine_temporal=gn_refine_temporal, bnb_test=bnb_test, keep_best=keep_best,
             epipolar_shift=epipolar_shift, cluster_rows=cluster_rows, finalize_pairs=finalize_pairs, sift_descriptors=sift_descriptors,
             sift_min_distances=sift_min_distances, undistort=undistort)
assert len(CALLS) == 19
IMAGE_ONLY = ("toed", "toed_pair", "sobel_gradients", "undistort")     # no list: one result whatever the length
OPTIONAL = dict(ncc_pairs=("left_patches", "sims", "best", "keep"), toed=("all4", "t_conv", "t_nms", "out"),
                toed_pair=("out_left", "out_right"), epi_candidates=("col_idx",))


@functools.lru_cache(maxsize=None)
def _fresh(name, n, **kw):
    with Context(H, W, device=0) as c:
        rc, out = CALLS[name](c, scene(n), **kw)
    assert rc == EBVO_OK, (name, n, rc)
    return out


def fresh(name, n, **kw):
    """the call on a context that has made no other"""
    return _fresh(name, 0 if name in IMAGE_ONLY else n, **kw)


def assert_same(got, ref, what, but=()):
    assert set(got) == set(ref), what
    for k in ref:
        if k in but or k in UNPINNED:
            continue
        a, b = got[k], ref[k]
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
        assert a.tobytes() == b.tobytes(), (what, k)


def overwrite(s):
    for a in s.values():
        a.view(np.uint8)[...] = 0xFF


def untouched(out, but=()):
    return all((a.view(np.uint8) == SENTINEL).all() for k, a in out.items() if k not in but)


@pytest.fixture(scope="module")
def hctx():
    with Context(H, W, device=0) as c:
        yield c


@functools.lru_cache(maxsize=None)
def pair_ref():
    """the resident pair on a context that makes no other call"""
    left, right = _images()
    with Context(H, W, device=0) as c:
        c.stereo_upload(left, right)
        counts = c.stereo_run(c.default_params(F21))
        return c.stereo_fetch(counts, patches=True)


# ---- interleaved calls -------------------------------------------------------------------------------------------------------
def test_interleaved_calls_reuse_the_pair_buffers(hctx):
    for step, n in enumerate(LENGTHS):
        for name, call in CALLS.items():
            rc, got = call(hctx, scene(n))
            assert rc == EBVO_OK, (name, n, rc, hctx.lib.ebvo_last_error(hctx._ctx))
            assert_same(got, fresh(name, n), f"step {step}: {name} with {n}")


# ---- capacity refusal, then reuse --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toed", "toed_pair"])
def test_a_toed_capacity_refusal_writes_the_counts_and_no_edge(hctx, name):
    ref = fresh(name, 0)
    kept = int(ref["n_kept"].max())
    assert kept >= 1
    s = scene(0)
    rc, out = CALLS[name](hctx, s, cap=kept - 1)
    overwrite(s)                                           # nothing of the refused call may still be reading the inputs
    assert rc == EBVO_ERR_CAPACITY
    assert (out["n_kept"] == ref["n_kept"]).all() and (out["n_total"] == ref["n_total"]).all()
    assert untouched(out, but=("n_kept", "n_total") + UNPINNED), "the refused call wrote an edge"
    rc, got = CALLS[name](hctx, scene(0))
    assert rc == EBVO_OK
    assert_same(got, ref, f"{name} after the capacity refusal")


@pytest.mark.parametrize("name", ["epi_candidates", "epi_candidates_staged"])
def test_a_candidate_capacity_refusal_writes_the_rows_and_no_list(hctx, name):
    n = len(full_scene()["L"])
    ref = fresh(name, n)
    total = int(ref["n_pairs"][0])
    assert total >= 1
    s = full_scene()
    rc, out = CALLS[name](hctx, s, cap=total - 1)
    overwrite(s)
    assert rc == EBVO_ERR_CAPACITY
    assert out["n_pairs"][0] == total and (out["row_ptr"] == ref["row_ptr"]).all()
    assert untouched(out, but=("n_pairs", "row_ptr")), "the refused call wrote a list"
    # the sizing pass: no room and no list asked for
    sized = dict(row_ptr=blank(n + 1, np.int32), n_pairs=blank(1, np.int64))
    s, p = full_scene(), hctx.default_params()
    head = (hctx._ctx, ptr(s["L"]), n, ptr(s["R"]), n, ptr(s["lines"]), p.epi_thr, p.max_disp, p.orient_thr_deg)
    if name == "epi_candidates":
        rc = hctx.lib.ebvo_epi_candidates(*head, p.stage_mask, ptr(sized["row_ptr"]), None, 0, at(sized["n_pairs"], C.c_int64))
    else:
        rc = hctx.lib.ebvo_epi_candidates_staged(*head, ptr(sized["row_ptr"]), None, None, 0, at(sized["n_pairs"], C.c_int64))
    assert rc == EBVO_OK and sized["n_pairs"][0] == total and (sized["row_ptr"] == ref["row_ptr"]).all()
    rc, got = CALLS[name](hctx, full_scene(), cap=total)
    assert rc == EBVO_OK
    assert_same(got, ref, f"{name} after the capacity refusal")


# ---- slot in flight ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CALLS))
def test_a_call_is_refused_while_slot_0_is_in_flight(hctx, name):
    left, right = _images()
    ref_pair = pair_ref()
    hctx.stereo_upload(left, right)
    hctx.stereo_submit(hctx.default_params(F21))
    try:
        s = scene(3)
        rc, out = CALLS[name](hctx, s)
        overwrite(s)
        assert rc == EBVO_ERR_STATE
        assert untouched(out), "the refused call wrote an output"
    finally:
        counts = hctx.stereo_wait()
    got_pair = hctx.stereo_fetch(counts, patches=True)
    assert_same(got_pair, ref_pair, f"the pair {name} was refused under")
    rc, got = CALLS[name](hctx, scene(3))
    assert rc == EBVO_OK
    assert_same(got, fresh(name, 3), f"{name} after the state refusal")


# ---- what happens to the pair ------------------------------------------------------------------------------------------------
KEPT, GONE = EBVO_OK, EBVO_ERR_STATE     # what ebvo_stereo_fetch_slot answers after the call
TAKEN = (EBVO_OK, GONE)                  # the call ran (or had nothing to do) after it took the slot
LATE = (EBVO_ERR_ARG, GONE)              # refused after the slot was taken
EARLY = (EBVO_ERR_ARG, KEPT)             # refused on its arguments or its size: pair untouched
# form -> (return code of the call, return code of the fetch).  Forms: normal (3 elements), empty (0 elements), bad_size
# (h = 16), bad_csr (row_ptr[0] = 1), and one array left out of a non-empty call
PAIR_TABLE = dict(
    toed=dict(normal=TAKEN, bad_size=EARLY),
    toed_pair=dict(normal=TAKEN, bad_size=EARLY),
    epi_candidates=dict(normal=TAKEN, empty=TAKEN),
    epi_candidates_staged=dict(normal=TAKEN, empty=TAKEN),
    sobel_gradients=dict(normal=TAKEN, bad_size=EARLY),
    gn_refine_stereo=dict(normal=TAKEN, empty=TAKEN, bad_size=EARLY, bad_csr=LATE, alpha=LATE),
    edge_patches=dict(normal=TAKEN, empty=TAKEN, bad_size=EARLY),
    ncc_pairs=dict(normal=TAKEN, empty=TAKEN, bad_size=EARLY, bad_csr=LATE, Rc=LATE),
    ncc_patches=dict(normal=TAKEN, empty=(EBVO_OK, KEPT)),
    ncc_quads=dict(normal=TAKEN, empty=(EBVO_OK, KEPT)),
    gn_refine_temporal=dict(normal=TAKEN, empty=TAKEN, bad_size=EARLY, disp=LATE),
    bnb_test=dict(normal=TAKEN, empty=TAKEN, bad_csr=EARLY),
    keep_best=dict(normal=TAKEN, empty=TAKEN, bad_csr=EARLY),
    epipolar_shift=dict(normal=TAKEN, empty=TAKEN, bad_csr=EARLY),
    cluster_rows=dict(normal=TAKEN, empty=TAKEN, bad_csr=EARLY),
    finalize_pairs=dict(normal=TAKEN, empty=TAKEN),
    sift_descriptors=dict(normal=TAKEN, empty=TAKEN, bad_size=EARLY),
    sift_min_distances=dict(normal=TAKEN, empty=TAKEN, bad_csr=EARLY),
    undistort=dict(normal=TAKEN, bad_size=EARLY),
)
assert set(PAIR_TABLE) == set(CALLS)


@pytest.mark.parametrize("name", list(CALLS))
def test_what_a_call_does_to_the_resident_pair(hctx, name):
    left, right = _images()
    for form, (want_rc, want_fetch) in PAIR_TABLE[name].items():
        hctx.stereo_upload(left, right)
        hctx.stereo_run(hctx.default_params(F21))
        s, skip = scene(0 if form == "empty" else 3), ()
        if form == "bad_size":
            s["hw"][0] = 16
        elif form == "bad_csr":
            s["row_ptr"][0] = 1
        elif form not in ("normal", "empty"):
            skip = (form,)
        rc, _ = CALLS[name](hctx, s, skip)
        assert rc == want_rc, (name, form, rc)
        got = hctx.lib.ebvo_stereo_fetch_slot(hctx._ctx, 0, None, None, None, None, None, None, None, None)
        assert got == want_fetch, (name, form, got)


# ---- optional outputs --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,left_out", [(n, k) for n, keys in OPTIONAL.items() for k in keys])
def test_an_optional_output_left_out(hctx, name, left_out):
    ref = fresh(name, 65)
    rc, got = CALLS[name](hctx, scene(65), (left_out,))
    assert rc == EBVO_OK
    assert_same(got, ref, f"{name} without {left_out}", but=(left_out,))
    assert (got[left_out].view(np.uint8) == SENTINEL).all(), "an output that was not passed"
