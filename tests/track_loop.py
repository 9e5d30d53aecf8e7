"""What tests/test_gpu_track_slots.py shares: the two halves of tests/test_gpu_depth.py::current (upload + submit, wait + fetch),
the size calls through ctypes and the comparisons of whole records.  Every comparison is bit for bit."""
import ctypes
import functools

import numpy as np

from tests import oracle_cover as ocv
from tests.test_gpu_depth import INT_FIELDS as DEPTH_INTS
from tests.test_gpu_depth import frame
from tests.test_gpu_temporal_edges import F as F_RIG
from tests.util import assert_bit_equal, assert_edges_equal

POSE_INTS = ("status", "stop_reason", "rounds_run", "steps_kept", "n_kf", "fit_terms", "inliers", "n_assoc")
POSE_DOUBLES = ("cost_first", "cost_last", "rms_normal")
COUNTS = ("n_left", "n_right", "n_pairs", "n_matches")
FETCHED = ("row_ptr", "col_idx", "sims", "best", "keep")


@functools.lru_cache(maxsize=None)
def images(k):
    """frame k of tests/test_gpu_depth.py, made once: an asynchronous upload reads the arrays until the pair has been waited for"""
    return frame(k)


def submit(c, k, slot, upload="upload"):
    """the first half of current(): frame k into the slot and its chain enqueued; returns at once"""
    l, r = images(k)
    (c.stereo_upload_async if upload == "async" else c.stereo_upload)(l, r, slot=slot)
    c.stereo_submit(c.default_params(F_RIG), slot=slot)


def collect(c, slot):
    """the second half: (counts, the full fetch) of the slot's pair"""
    pair = c.stereo_wait(slot=slot)
    return pair, c.stereo_fetch(pair, slot=slot)


def same_pair(a, b, what):
    (ca, fa), (cb, fb) = a, b
    for k in COUNTS:
        assert getattr(ca, k) == getattr(cb, k), (what, k, getattr(ca, k), getattr(cb, k))
    assert_edges_equal(fa["left"], fb["left"], f"{what}: left edges")
    assert_edges_equal(fa["right"], fb["right"], f"{what}: right edges")
    for k in FETCHED:
        assert_bit_equal(fa[k], fb[k], f"{what}: {k}")


def same_final(a, b, what):
    """two results of stereo_finalize / stereo_finalize_wait"""
    (ca, fa), (cb, fb) = a, b
    assert ca == cb, (what, ca, cb)
    assert set(fa) == set(fb), (what, set(fa), set(fb))
    assert_edges_equal(fa["right"], fb["right"], f"{what}: right centre")
    for k in set(fa) - {"right"}:
        assert_bit_equal(fa[k], fb[k], f"{what}: {k}")


def align_size(c, slot):
    """(n_kf, n_left, n_right) of ebvo_temporal_align_size"""
    n = [ctypes.c_int32(-1) for _ in range(3)]
    c._check(c.lib.ebvo_temporal_align_size(c._ctx, slot, *(ctypes.byref(v) for v in n)), "ebvo_temporal_align_size")
    return tuple(v.value for v in n)


def cover_size(c, slot, **kw):
    """(n_kf, n0, cw, ch) of ebvo_temporal_cover_size"""
    p = c.cover_params(**kw)
    n = [ctypes.c_int32(-1) for _ in range(4)]
    c._check(c.lib.ebvo_temporal_cover_size(c._ctx, slot, ctypes.byref(p), *(ctypes.byref(v) for v in n)), "ebvo_temporal_cover_size")
    return tuple(v.value for v in n)


def same_pose_record(a, b, what):
    """two ebvo_aligned_pose records (without the association arrays, which the frame step does not return)"""
    for k in POSE_INTS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    for k in POSE_DOUBLES:
        assert_bit_equal(np.float64(a[k]), np.float64(b[k]), f"{what} {k}")
    for k in ("R", "t"):
        assert_bit_equal(a[k], b[k], f"{what} {k}")


def same_depth_record(a, b, what):
    for k in DEPTH_INTS + ("rms_before", "rms_after"):
        assert_bit_equal(np.asarray(a[k], dtype=np.float64), np.asarray(b[k], dtype=np.float64), f"{what} {k}")


def same_cover_record(a, b, what):
    for k in ocv.INT_FIELDS:
        assert a[k] == b[k], (what, k, a[k], b[k])
    assert_bit_equal(a["hist"], b["hist"], f"{what} hist")


def same_step(a, b, what):
    """two results of temporal_track_frame"""
    for k in ("tracked", "failed_stage", "decision", "reasons", "switched"):
        assert a[k] == b[k], (what, k, a[k], b[k])
    same_pose_record(a["pose"], b["pose"], f"{what}: pose")
    same_depth_record(a["depth"], b["depth"], f"{what}: depth")
    same_cover_record(a["cover"], b["cover"], f"{what}: cover")
    assert a["carried"] == b["carried"], (what, a["carried"], b["carried"])
    assert a["finalized"] == b["finalized"], (what, a["finalized"], b["finalized"])
    assert_bit_equal(a["R_seq"], b["R_seq"], f"{what}: R_seq")
    assert_bit_equal(a["t_seq"], b["t_seq"], f"{what}: t_seq")


def same_keyframe_pose(a, b, what):
    assert_bit_equal(a[0], b[0], f"{what}: Rk")
    assert_bit_equal(a[1], b[1], f"{what}: tk")
