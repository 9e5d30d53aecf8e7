"""The host-array calls that leave slot 0's state alone share one staging buffer (Slot::host_up) and one scope object that
waits for their copies on every return.  Every comparison here is against the same call on a fresh context, bit for bit (the
other GPU tests pin those results to the oracles):

  one buffer, many callers   the ten entry points interleaved on one context with lists of 3, 300, 1, 65, 0 and 3 elements: the
                             buffer grows, then a smaller call of another layout reuses the larger stale one
  error, then reuse          ebvo_tgt_veridical / ebvo_tprior_candidates refused for capacity or for slot 0 in flight, every input
                             overwritten at once, then the same call again
  optional outputs           each optional output left out, one at a time

Images are 64 x 48 with cells of 8; the mates and edges are tests/align_cases.py's exact rig on a lattice."""
import ctypes as C
import functools

import numpy as np
import pytest

from edge_based_visual_odometry_amd import _lib, synth
from edge_based_visual_odometry_amd._lib import EBVO_ERR_CAPACITY, EBVO_ERR_STATE, EBVO_OK, ptr
from edge_based_visual_odometry_amd.api import Context
from tests import align_cases as ac

pytestmark = pytest.mark.gpu

W, H, CELL = 64, 48, 8
LENGTHS = (3, 300, 1, 65, 0, 3)
POSE_R, POSE_T = np.eye(3), np.array([0.002, -0.001, 0.0005])
SENTINEL = 0x5A     # what every output holds before a call


def locs(n):
    """n left locations inside the 10 px margin of a 64 x 48 image, one px apart in x and three in y"""
    return [(12.0 + (k % 40), 12.5 + 3.0 * (k // 40)) for k in range(n)]


@functools.lru_cache(maxsize=None)
def _scene(n, n_cf):
    c = ac.exact(locs=locs(max(n, n_cf)), w=W, h=H)
    kfL, kfR, cfL, cfR = c["kf_left"][:n], c["kf_right"][:n], c["edges_left"][:n_cf], c["edges_right"][:n_cf]
    k = np.arange(n)
    yy, xx = np.mgrid[0:H, 0:W]
    two = 2 * np.arange(n + 1, dtype=np.int32)             # two candidates per row
    cand = np.repeat(cfL[:n] if n_cf >= n else kfL, 2)
    cand["x"][1::2] += 0.5
    s = dict(kfL=kfL, kfR=kfR, cfL=cfL, cfR=cfR, lam=1.0 + 0.01 * (k % 5), assoc=np.where(k < n_cf, k, -1).astype(np.int32),
             lam_in=1.0 + 0.02 * (k % 3), info_in=0.5 + 0.25 * (k % 4), nobs_in=(k % 3).astype(np.int32),
             disp=(8.0 + 0.05 * ((xx + 2 * yy) % 7)).astype(np.float32), row_ptr=two, cand=cand, cand_r=np.repeat(kfR, 2),
             focused=(k % 5 != 0).astype(np.uint8), row_on=(k % 4 != 1).astype(np.uint8),
             xy_l=np.stack([kfL["x"], kfL["y"]], axis=1), xy_r=np.stack([kfR["x"], kfR["y"]], axis=1),
             gamma=np.stack([(kfL["x"] - 100.0) / 16.0, (kfL["y"] - 60.0) / 16.0, np.full(n, 8.0)], axis=1))
    return {k: np.ascontiguousarray(v) for k, v in s.items()}


def scene(n, n_cf=None):
    """a private copy of the inputs: n keyframe mates, n_cf current-frame mates / edges (default n)"""
    return {k: v.copy() for k, v in _scene(n, n if n_cf is None else n_cf).items()}


def blank(shape, dtype):
    a = np.empty(shape, dtype=dtype)
    a.view(np.uint8)[...] = SENTINEL
    return a


def arg(out, key, skip):
    return None if key in skip else ptr(out[key])


def common(c):
    return c._calib(ac.EXACT_CALIB), np.ascontiguousarray(POSE_R).reshape(9), np.ascontiguousarray(POSE_T)


# ---- the ten entry points: (context, scene, what to leave out) -> (return code, outputs) ---------------------------------
def align(c, s, skip=()):
    cal, R, t = common(c)
    n, p, r = len(s["kfL"]), c.align_params(rounds=2, iterations=3, cell_size=CELL, radius=4.0, min_terms=6), _lib.AlignedPose()
    out = dict(assoc_left=blank(n, np.int32), assoc_right=blank(n, np.int32))
    rc = c.lib.ebvo_pose_align_edges_depth(c._ctx, ptr(s["kfL"]), ptr(s["kfR"]), ptr(s["lam"]), n, ptr(s["cfL"]), len(s["cfL"]),
                                           ptr(s["cfR"]), len(s["cfR"]), W, H, C.byref(cal), C.byref(p), ptr(R), ptr(t), C.byref(r),
                                           arg(out, "assoc_left", skip), arg(out, "assoc_right", skip))
    return rc, dict(out, record=bytes(r))


def depth(c, s, skip=()):
    cal, R, t = common(c)
    n, p, r = len(s["kfL"]), c.depth_params(), _lib.DepthRefined()
    out = dict(lambda_=blank(n, np.float64), info=blank(n, np.float64), n_obs=blank(n, np.int32), flags=blank(n, np.uint8))
    sin = (None, None, None) if "state_in" in skip else (ptr(s["lam_in"]), ptr(s["info_in"]), ptr(s["nobs_in"]))
    rc = c.lib.ebvo_depth_refine_edges(c._ctx, ptr(s["kfL"]), ptr(s["kfR"]), n, ptr(s["cfL"]), len(s["cfL"]), ptr(s["cfR"]),
                                       len(s["cfR"]), ptr(s["assoc"]), ptr(s["assoc"]), W, H, C.byref(cal), C.byref(p), ptr(R), ptr(t),
                                       *sin, *(ptr(out[k]) for k in ("lambda_", "info", "n_obs", "flags")), C.byref(r))
    return rc, dict(out, record=bytes(r))


def carry(c, s, skip=()):
    cal, R, t = common(c)
    n, nn, p, r = len(s["kfL"]), len(s["cfL"]), c.depth_carry_params(cell_size=CELL, radius=4.0), _lib.DepthCarried()
    out = dict(lambda_=blank(nn, np.float64), info=blank(nn, np.float64), n_obs=blank(nn, np.int32), flags=blank(nn, np.uint8),
               src_index=blank(nn, np.int32))
    sin = (None, None, None) if "state_in" in skip else (ptr(s["lam_in"]), ptr(s["info_in"]), ptr(s["nobs_in"]))
    rc = c.lib.ebvo_depth_carry(c._ctx, ptr(s["kfL"]), ptr(s["kfR"]), n, *sin, ptr(s["cfL"]), ptr(s["cfR"]), nn, W, H, C.byref(cal),
                                C.byref(p), ptr(R), ptr(t), *(ptr(out[k]) for k in ("lambda_", "info", "n_obs", "flags", "src_index")),
                                C.byref(r))
    return rc, dict(out, record=bytes(r))


def cover(c, s, skip=()):
    cal, R, t = common(c)
    n, n0, p, r = len(s["kfL"]), len(s["cfL"]), c.cover_params(cell_size=CELL, radius=4.0, cover_cell=16), _lib.KeyframeCover()
    nc = ((W + 15) // 16) * ((H + 15) // 16)
    out = dict(flags=blank(n, np.uint8), assoc=blank(n, np.int32), disp=blank(n, np.float64), explained=blank(n0, np.uint8),
               cell_edges=blank(nc, np.int32), cell_explained=blank(nc, np.int32))
    rc = c.lib.ebvo_keyframe_cover_edges(c._ctx, ptr(s["kfL"]), ptr(s["kfR"]), ptr(s["lam"]), n, ptr(s["cfL"]), n0, W, H, C.byref(cal),
                                         C.byref(p), ptr(R), ptr(t), C.byref(r), *(arg(out, k, skip) for k in out))
    return rc, dict(out, record=bytes(r))


def gt_locate(c, s, skip=()):
    cal, n = c._calib(ac.EXACT_CALIB), len(s["kfL"])
    out = dict(valid=blank(n, np.uint8), gt_xy=blank((n, 2), np.float64), gamma_left=blank((n, 3), np.float64),
               gamma_right=blank((n, 3), np.float64))
    rc = c.lib.ebvo_gt_locate(c._ctx, ptr(s["kfL"]), n, ptr(s["disp"]), H, W, W, C.byref(cal), None, ptr(out["valid"]),
                              arg(out, "gt_xy", skip), arg(out, "gamma_left", skip), arg(out, "gamma_right", skip))
    return rc, out


def gt_rows(c, s, skip=()):
    n, g = len(s["kfL"]), _lib.GtStage()
    out = dict(n_tp=blank((n, 2), np.int32))
    rc = c.lib.ebvo_gt_evaluate_rows(c._ctx, ptr(s["row_ptr"]), ptr(s["cand"]), n, ptr(s["focused"]), ptr(s["xy_l"]), 1.0,
                                     arg(out, "n_tp", skip), C.byref(g))
    return rc, dict(out, record=bytes(g))


def tgt_grid(c, s, skip=()):
    n, g = len(s["kfL"]), _lib.GtStage()
    out = dict(n_tp=blank((n, 2), np.int32))
    rc = c.lib.ebvo_tgt_grid_rows(c._ctx, ptr(s["kfL"]), ptr(s["kfR"]), n, ptr(s["cfL"]), ptr(s["cfR"]), len(s["cfL"]), W, H, CELL, 12.0,
                                  ptr(s["row_on"]), ptr(s["xy_l"]), ptr(s["xy_r"]), 2.0, arg(out, "n_tp", skip), C.byref(g))
    return rc, dict(out, record=bytes(g))


def _two_pass(c, s, skip, cap, flag, rows, lst, call):
    """both passes as the wrappers make them (cap None: the first pass sizes the list); cap given: the second pass alone"""
    n = len(s["kfL"])
    out = {flag: blank(n, np.uint8), "proj_left": blank((n, 2), np.float64), "proj_right": blank((n, 2), np.float64),
           "orient_left": blank(n, np.float64), "orient_right": blank(n, np.float64), rows: blank(n + 1, np.int32)}
    outs = [arg(out, k, skip) for k in out]
    count = C.c_int64(-7)
    if cap is None:
        rc = call(outs, None, 0, count)
        if rc != EBVO_OK:
            return rc, dict(out, n=count.value)
        cap = count.value
    out[lst] = blank(cap, np.int32)
    rc = call(outs, arg(out, lst, skip), cap, count)
    return rc, dict(out, n=count.value)


def tgt_veridical(c, s, skip=(), cap=None):
    cal, R, t = common(c)
    p = c.tgt_params()
    return _two_pass(c, s, skip, cap, "in_image", "ver_row_ptr", "ver_idx", lambda outs, lst, room, count: c.lib.ebvo_tgt_veridical(
        c._ctx, ptr(s["kfL"]), ptr(s["kfR"]), ptr(s["gamma"]), len(s["kfL"]), ptr(s["cfL"]), ptr(s["cfR"]), len(s["cfL"]), W, H, CELL,
        ptr(R), ptr(t), C.byref(cal), C.byref(p), *outs, lst, room, C.byref(count)))


def tprior(c, s, skip=(), cap=None):
    cal, R, t = common(c)
    p = c.tprior_params()
    return _two_pass(c, s, skip, cap, "live", "row_ptr", "col_idx", lambda outs, lst, room, count: c.lib.ebvo_tprior_candidates(
        c._ctx, ptr(s["kfL"]), ptr(s["kfR"]), len(s["kfL"]), ptr(s["cfL"]), ptr(s["cfR"]), len(s["cfL"]), W, H, CELL, 12.0, 10.0, ptr(R),
        ptr(t), C.byref(cal), C.byref(p), *outs, lst, room, C.byref(count)))


def tgt_rows(c, s, skip=()):
    n, g = len(s["kfL"]), _lib.GtStage()
    out = dict(n_tp=blank((n, 2), np.int32), is_tp=blank(2 * n, np.uint8))
    rc = c.lib.ebvo_tgt_evaluate_rows(c._ctx, ptr(s["row_ptr"]), ptr(s["cand"]), ptr(s["cand_r"]), n, ptr(s["row_on"]), ptr(s["xy_l"]),
                                      ptr(s["xy_r"]), 2.0, arg(out, "n_tp", skip), arg(out, "is_tp", skip), C.byref(g))
    return rc, dict(out, record=bytes(g))


CALLS = dict(align=align, depth=depth, carry=carry, cover=cover, gt_locate=gt_locate, gt_rows=gt_rows, tgt_grid=tgt_grid,
             tgt_veridical=tgt_veridical, tprior=tprior, tgt_rows=tgt_rows)
OPTIONAL = dict(align=("assoc_left", "assoc_right"), depth=("state_in",), carry=("state_in",),
                cover=("flags", "assoc", "disp", "explained", "cell_edges", "cell_explained"),
                gt_locate=("gt_xy", "gamma_left", "gamma_right"), gt_rows=("n_tp",), tgt_grid=("n_tp",),
                tgt_veridical=("in_image", "proj_left", "proj_right", "orient_left", "orient_right", "ver_row_ptr"),
                tprior=("live", "proj_left", "proj_right", "orient_left", "orient_right", "row_ptr"), tgt_rows=("n_tp", "is_tp"))
INPUTS = {"state_in"}      # an optional input: leaving it out changes the result, so the fresh call leaves it out too


@functools.lru_cache(maxsize=None)
def fresh(name, n, n_cf=None, skip=frozenset()):
    """the call on a context that has made no other"""
    with Context(H, W, device=0) as c:
        rc, out = CALLS[name](c, scene(n, n_cf), skip)
    assert rc == EBVO_OK, (name, n, rc)
    return out


def assert_same(got, ref, what, but=()):
    assert set(got) == set(ref), what
    for k in ref:
        if k in but:
            continue
        a, b = got[k], ref[k]
        if isinstance(a, np.ndarray):
            assert a.dtype == b.dtype and a.shape == b.shape, (what, k)
            a, b = a.tobytes(), b.tobytes()
        assert a == b, (what, k)


@pytest.fixture(scope="module")
def hctx():
    with Context(H, W, device=0) as c:
        yield c


# ---- one buffer, many callers ---------------------------------------------------------------------------------------------
def test_interleaved_calls_share_the_buffer(hctx):
    for step, n in enumerate(LENGTHS):
        for name, call in CALLS.items():
            rc, got = call(hctx, scene(n))
            assert rc == EBVO_OK, (name, n, rc, hctx.lib.ebvo_last_error(hctx._ctx))
            assert_same(got, fresh(name, n), f"step {step}: {name} with {n}")


# ---- error, then reuse -----------------------------------------------------------------------------------------------------
def overwrite(s):
    for a in s.values():
        a.view(np.uint8)[...] = 0xFF


def untouched(out, but=()):
    return all((a.view(np.uint8) == SENTINEL).all() for k, a in out.items() if isinstance(a, np.ndarray) and k not in but)


@pytest.mark.parametrize("name", ["tgt_veridical", "tprior"])
def test_a_capacity_error_leaves_the_next_call_alone(hctx, name):
    ref = fresh(name, 5, 7)
    assert ref["n"] >= 1
    s = scene(5, 7)
    rc, out = CALLS[name](hctx, s, cap=ref["n"] - 1)
    overwrite(s)                                           # nothing of the refused call may still be reading the inputs
    assert rc == EBVO_ERR_CAPACITY and out["n"] == ref["n"]
    rc, got = CALLS[name](hctx, scene(5, 7), cap=ref["n"])
    assert rc == EBVO_OK
    assert_same(got, ref, f"{name} after the capacity error")


@pytest.mark.parametrize("name", ["tgt_veridical", "tprior"])
def test_a_state_error_comes_before_any_device_work(name):
    ref = fresh(name, 5, 7)
    k = synth.CALIB["kitti"]
    F = synth.fundamental_21(k["K"], k["K"], k["R21"], k["T21"])
    left, right = synth.stereo_pair("s2", 96, 160)
    with Context(96, 160, device=0) as c:
        c.stereo_upload(left, right)
        c.stereo_submit(c.default_params(F))
        try:
            s = scene(5, 7)
            rc, out = CALLS[name](c, s, cap=ref["n"])
            overwrite(s)
            assert rc == EBVO_ERR_STATE
            assert out["n"] == -7 and untouched(out), "the refused call wrote an output"
        finally:
            c.stereo_wait()
        rc, got = CALLS[name](c, scene(5, 7), cap=ref["n"])
        assert rc == EBVO_OK
        assert_same(got, ref, f"{name} after the state error")


# ---- optional outputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,left_out", [(n, k) for n, keys in OPTIONAL.items() for k in keys])
def test_an_optional_argument_left_out(hctx, name, left_out):
    skip = frozenset([left_out])
    ref = fresh(name, 3, None, skip) if left_out in INPUTS else fresh(name, 3)
    rc, got = CALLS[name](hctx, scene(3), skip)
    assert rc == EBVO_OK
    assert_same(got, ref, f"{name} without {left_out}", but=skip)
    if left_out not in INPUTS:
        assert (got[left_out].view(np.uint8) == SENTINEL).all(), "an output that was not passed"
