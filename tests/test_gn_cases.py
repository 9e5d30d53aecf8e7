"""The inputs of tests/test_gpu_gn_edges.py meet the conditions that file relies on -- recomputed on the oracle alone (no
device): the step images fill both 11-bit gradient fields of the packed records in every sign combination, the half-flat pair
stops pairs on H < 1e-8 at the first iteration and after it, the chosen rows_below values sit on the active-pair profile where
the hand-over cases need them, the size and border cases are what their names say -- and the oracle agrees bit for bit with
the line-by-line Python reading of tests/test_oracle_gn.py at these gradients, clamped patches and late stops included."""
import numpy as np

from tests import gn_cases as gc
from tests import oracle as orc
from tests.test_oracle_gn import _gn_python


def test_steps_pair_fills_the_packed_fields():
    h, w = gc.STEPS_SHAPE
    for img in gc.steps_pair(h, w):
        assert set(np.unique(img)) == {0, 255}
        fx, fy = gc.packed_fields(img)
        for f in (fx, fy):                                    # the top magnitude bit and the sign extension below -512
            assert f.max() == 1020 and f.min() == -1020
        big = (np.abs(fx) >= 512) & (np.abs(fy) >= 512)
        for sx in (1, -1):
            for sy in (1, -1):
                assert (big & (np.sign(fx) == sx) & (np.sign(fy) == sy)).sum() >= 100, (sx, sy)
        assert (np.abs(fy[:, [0, -1]]) >= 512).any() and (np.abs(fx[[0, -1], :]) >= 512).any()
        # reflect-101: the two columns a border column's gx subtracts are the same column, likewise gy in the border rows
        assert not fx[:, [0, -1]].any() and not fy[[0, -1], :].any()
    l, r = gc.steps_pair(h, w)
    assert (r[:, :-gc.DISPARITY] == l[:, gc.DISPARITY:]).all()


def test_the_generators_stay_below_the_top_bit():
    """what every other refinement test samples: s2 and s1 never set the top magnitude bit of either field"""
    from edge_based_visual_odometry_amd import synth
    for img in (synth.s2_image(96, 160), synth.s1_image(96, 160)):
        fx, fy = gc.packed_fields(img)
        assert max(np.abs(fx).max(), np.abs(fy).max()) < 512 and img.min() > 0 and img.max() < 255


def test_half_flat_pair_stops_late():
    c, ref = gc.half_flat_case(), gc.named_ref("half_flat")
    assert (c["r"][:, 48:] == 128).all() and len(c["cand"]) == 2 * len(c["L"]) > 1500
    v, it = ref["validity"], ref["iters"]
    assert ((v == 2) & (it >= 1)).sum() >= 20 and ((v == 2) & (it == 0)).sum() >= 5
    assert set(np.unique(v)) == {0, 1, 2}
    assert len(set(it[(v == 2)])) >= 8                       # ... at many different iterations
    assert np.isnan(ref["score"][v == 2]).all() and not np.isnan(ref["score"][v != 2]).any()
    assert np.abs(ref["alpha"]).max() > 200                   # patches sampled far outside the image, clamped


def test_profile_counts_the_active_pairs():
    for name in ("half_flat", "steps", "s2"):
        ref = gc.named_ref(name)
        prof = gc.profile(ref, 20)
        assert prof[0] == len(ref["iters"]) and (np.diff(prof) <= 0).all() and prof[-1] > 0
        # the pairs that leave between two iterations are those whose verdict the earlier one wrote
        v2 = ref["validity"] == 2
        for it in range(19):
            assert prof[it] - prof[it + 1] == int(((ref["iters"] == it) & v2).sum() + ((ref["iters"] == it + 1) & ~v2).sum())
    # tol = 0 on the step pair: no pair leaves before the last iteration, so a rows_below of n_pairs - 1 keeps every
    # iteration in the thread layout; on the half-flat pair only the stops on H < 1e-8 leave
    ref = gc.named_ref("steps", tol=0.0)
    assert (gc.profile(ref, 20) == len(ref["iters"])).all() and (ref["iters"] == 20).all()
    ref = gc.named_ref("half_flat", tol=0.0)
    prof = gc.profile(ref, 20)
    assert prof[0] - prof[-1] == ((ref["validity"] == 2) & (ref["iters"] < 19)).sum() > 20
    # tol = inf: the first iteration finishes every pair
    assert (gc.profile(gc.named_ref("half_flat", tol=np.inf), 20)[1:] == 0).all()


def test_thresholds_sit_on_the_profile():
    prof = gc.profile(gc.named_ref("half_flat"), 20)
    thr, j = gc.thresholds(prof)
    n = len(gc.half_flat_case()["cand"])
    assert thr["all"] == n and thr["all-1"] == n - 1                       # n_pairs > rows_below: false, then true
    assert 2 <= j < 19 and prof[j] < prof[j - 1] and thr["equal"] == prof[j]  # the list before it is over the threshold
    assert thr["equal-1"] == prof[j] - 1 >= 1 and prof[j] > thr["equal-1"]    # iteration j itself is over this one
    assert prof[-1] > thr["one"] == 1                                      # never in the row layout before the last list
    assert 8 <= j <= 12 and prof[j + 1] > 0                                # several iterations in either layout
    assert len(set(thr.values())) == 5
    # with one workgroup (developer key 9 = 1) the 32 groups of the persistent launch walk many pairs each
    assert thr["all"] / 32 > 50


def test_chain_refinement_thresholds_differ():
    """the refinement inside the default pair's finalize chain: its inputs are the chain oracle's, and the two rows_below
    values of the GPU file hand over at different iterations"""
    from tests import finalize_cases as fc
    case, ref = gc.chain_refinement()
    ch = fc.chain("default")
    assert len(case["cand"]) == ch["counts"]["n_bnb"] and (np.diff(case["rp"]) == ch["stage_rows"]["REFINE"]).all()
    prof = gc.profile(ref, 20)
    (one, mid), j = gc.chain_thresholds()
    assert one == 1 and mid == prof[j] < prof[j - 1] and 8 <= j <= 12
    # key 5 = mid: iterations 0 .. j - 1 in the thread layout, j .. 19 in the row layout; key 5 = 1: all 20 in the thread layout
    assert prof[0] > mid > prof[-1] > 1 and prof[j + 1] > 0
    assert prof[0] > 3 * 256 * 4                       # more than one grid-stride turn per block under grid caps 1 and 3


def test_size_cases_are_what_they_are_named():
    c = gc.s2_case()
    assert len(c["cand"]) > max(gc.PAIR_COUNTS) and len(c["L"]) > max(gc.LEFT_COUNTS)
    for n in gc.PAIR_COUNTS:
        s = gc.sub_case(c, n_pairs=n)
        assert s["rp"][-1] == n == len(s["cand"]) and len(s["rp"]) == len(c["L"]) + 1 and (np.diff(s["rp"]) >= 0).all()
    for nL in gc.LEFT_COUNTS:
        s = gc.sub_case(c, nL=nL)
        assert len(s["L"]) == len(s["lines"]) == nL == len(s["rp"]) - 1 and s["rp"][-1] == len(s["cand"]) > 0, nL
    assert list(gc.sub_case(c, nL=1)["rp"]) == [0, 2]                      # a one-row CSR that holds pairs
    rows = gc.row_shape_cases()
    for s in rows.values():
        assert len(s["rp"]) == len(s["L"]) + 1 and s["rp"][0] == 0 and s["rp"][-1] == len(s["cand"]) == 600
        assert (np.diff(s["rp"]) >= 0).all()
    e = gc.EMPTY_ROWS
    assert not rows["first-rows-empty"]["rp"][:e + 1].any() and rows["first-rows-empty"]["rp"][e + 3] > 0
    assert (rows["last-rows-empty"]["rp"][-e - 1:] == 600).all() and rows["last-rows-empty"]["rp"][-e - 2] < 600
    assert (np.diff(rows["one-row"]["rp"]) > 0).sum() == 1
    assert gc.SMALL_SHAPES[0] == (32, 32) and {w % 64 for _, w in gc.SMALL_SHAPES[1:]} == {1, 63}
    for h, w in gc.SMALL_SHAPES:
        img = gc.small_case(h, w)["l"]
        view = gc.strided(img)
        assert view.strides[0] > w and (view == img).all() and not view.flags["C_CONTIGUOUS"]
    assert {1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 1025} == set(gc.PAIR_COUNTS) and len(gc.temporal_s2_case()["kf"]) == 1025


def test_border_points_clamp_at_every_border_and_corner():
    h, w = gc.STEPS_SHAPE
    pts = gc.border_points(h, w)
    side = lambda v, n: -1 if v < 0 else (1 if v > n - 1 else 0)          # the centre itself is outside on that axis
    assert {(side(x, w), side(y, h)) for x, y in pts[:8]} =={(sx, sy) for sx in (-1, 0, 1) for sy in (-1, 0, 1)} - {(0, 0)}
    far = pts[8:]
    assert np.isfinite(far).all() and {1e6, -1e6, 1e15, -1e15} <= set(far.ravel())
    # the stereo rows and the temporal items that carry them
    c = gc.with_border_candidates(gc.steps_case())
    assert (c["cand"][-len(pts):] == pts).all() and c["rp"][-1] == len(c["cand"]) and len(c["rp"]) == len(c["L"]) + 1
    t = gc.with_border_starts(gc.temporal_steps_case())
    n = len(pts)
    assert (np.abs((t["kf"]["x"][-n:] - t["init"][-n:, 0]) - pts[:, 0]) <= np.abs(pts[:, 0]) * 2e-16 + 1e-12).all()
    # the refinement's verdicts there are not all of one kind
    assert len(set(gc.stereo_ref(c)["validity"][-n:])) >= 2


def test_steps_refinement_at_both_huber_deltas():
    v3, v40 = gc.named_ref("steps")["validity"], gc.named_ref("steps", huber_delta=40.0)["validity"]
    assert (v3 == 0).sum() > 50 and (v3 == 1).sum() > 50 and (v40 == 1).mean() > 0.95 and (v3 != v40).any()
    t = gc.named_ref("temporal_steps")
    assert (t["validity"] == 0).sum() > 50 and (t["validity"] == 1).sum() > 50


def _python_agrees(case, picks, kw=None):
    kw = kw or {}
    rows = np.repeat(np.arange(len(case["L"])), np.diff(case["rp"]))
    out = orc.gn_refine_stereo(case["l"], case["r"], case["L"], case["lines"], case["rp"], case["cand"], math_mode=orc.LIBM,
                               **{**gc.GN_DEFAULT, **kw})
    IL, IR = case["l"].astype(np.float32), case["r"].astype(np.float32)
    GX, GY = orc.sobel_gradients(case["r"])
    for k in picks:
        le, ln = case["L"][rows[k]], case["lines"][rows[k]]
        a, sc, cf, va, it, xy = _gn_python(IL, IR, GX, GY, le, ln, case["cand"][k, 0], case["cand"][k, 1],
                                           huber=kw.get("huber_delta", 3.0))
        assert (out["validity"][k], out["iters"][k]) == (va, it), k
        same = lambda x, y: np.float64(x).tobytes() == np.float64(y).tobytes()     # the bytes: -0.0 is not +0.0
        assert same(out["alpha"][k], a) and same(out["refined_xy"][k, 0], xy[0]) and same(out["refined_xy"][k, 1], xy[1]), k
        if va != 2:
            assert same(out["score"][k], sc) and same(out["confidence"][k], cf), k
        else:
            assert np.isnan(out["score"][k]) and np.isnan(out["confidence"][k]), k
    return out


def test_oracle_equals_python_reading_on_steps():
    """~40 pairs of the step image, a third of them clamped at a border or far outside, at both Huber deltas"""
    c = gc.with_border_candidates(gc.steps_case())
    n_far = len(gc.border_points(*gc.STEPS_SHAPE))
    rng = np.random.default_rng(7)
    picks = np.concatenate([rng.choice(len(c["cand"]) - n_far, 16, replace=False), np.arange(len(c["cand"]) - n_far, len(c["cand"]))])
    assert len(picks) == 40
    out = _python_agrees(c, picks)
    assert len(set(out["validity"][picks])) == 3
    _python_agrees(c, picks[::3], dict(huber_delta=40.0))


def test_oracle_equals_python_reading_on_half_flat():
    """~40 pairs of the half-flat pair, half of them stopping on H < 1e-8 after the first iteration"""
    c, ref = gc.half_flat_case(), gc.named_ref("half_flat")
    late = np.flatnonzero((ref["validity"] == 2) & (ref["iters"] >= 1))
    rng = np.random.default_rng(8)
    picks = np.concatenate([late[:: max(1, len(late) // 20)][:20], np.flatnonzero((ref["validity"] == 2) & (ref["iters"] == 0))[:4],
                            rng.choice(len(c["cand"]), 16, replace=False)])
    out = _python_agrees(c, picks)
    assert ((out["validity"][picks] == 2) & (out["iters"][picks] >= 1)).sum() >= 15
