"""The inputs of the Gauss-Newton refinement edge tests (tests/test_gpu_gn_edges.py, tests/test_gn_cases.py): 0/255 step
images that fill the two 11-bit gradient fields of gn_pack_kernel's records, a half-flat right image on which pairs stop on
H < 1e-8 after their first iteration, the active-pair profile of a refinement and the rows_below values that put the stereo
hand-over on it, and the size, border and parameter cases.  Everything here is numpy and the CPU oracle (tests/oracle.py);
nothing comes from the device.  tests/test_gn_cases.py re-derives every condition the GPU file relies on."""
import functools

import numpy as np

from edge_based_visual_odometry_amd import synth
from tests import oracle as orc

F = synth.fundamental_for("kitti")     # rectified rig: horizontal epipolar lines
DISPARITY = 12
GN_DEFAULT = dict(max_iter=20, tol=1e-3, huber_delta=3.0)
STEPS_SHAPE = HALF_FLAT_SHAPE = (64, 96)
S2_SHAPE = (96, 160)


# --- images -------------------------------------------------------------------------------------------------------------
def steps_image(h, w, shift=0, y0=0):
    """0 / 255 only: a 9 x 7 chequerboard (axis-aligned steps) XOR a diagonal family XOR an anti-diagonal family, sampled at
    (x + shift, y + y0).  Axis-aligned steps alone give |8 g| = 1020 in one field at a time, the diagonal family both fields
    with equal signs, the anti-diagonal one with opposite signs."""
    y = np.arange(h, dtype=np.int64)[:, None] + y0
    x = np.arange(w, dtype=np.int64)[None, :] + shift
    v = ((x // 9 + y // 7) % 2) ^ ((x + y) % 23 < 11) ^ ((x - y) % 19 < 9)
    return (v * 255).astype(np.uint8)


def steps_pair(h, w):
    """the right image is the left scene DISPARITY px to the left (x_R = x_L - d, as synth.stereo_pair)"""
    return steps_image(h, w), steps_image(h, w, shift=DISPARITY)


def half_flat_pair(h, w):
    """synth.stereo_pair("s2", ...) with the right image flat (128) from column w / 2 on: a patch that wanders into the flat
    half meets zero gradients and stops on H < 1e-8 at whichever iteration takes it there"""
    l, r = synth.stereo_pair("s2", h, w)
    r = r.copy()
    r[:, w // 2:] = 128
    return l, r


def packed_fields(img):
    """(8 gx, 8 gy) of the oracle's Sobel planes as integers: what gn_pack_kernel stores in its two 11-bit fields"""
    gx, gy = orc.sobel_gradients(img)
    fx, fy = gx.astype(np.float64) * 8, gy.astype(np.float64) * 8
    assert (fx == np.rint(fx)).all() and (fy == np.rint(fy)).all()
    return fx.astype(np.int64), fy.astype(np.int64)


def strided(img, pad=13):
    """the same pixels as a row-strided view of a wider array (the filler is not the image's border value)"""
    wide = np.full((img.shape[0], img.shape[1] + pad), 201, dtype=np.uint8)
    wide[:, :img.shape[1]] = img
    view = wide[:, :img.shape[1]]
    assert view.strides == (img.shape[1] + pad, 1)
    return view


# --- stereo cases: dict(l, r, L, lines, rp, cand) -------------------------------------------------------------------------
def _case(l, r, L, rp, cand):
    return dict(l=l, r=r, L=L, lines=orc.epipolar_lines(F, L), rp=np.asarray(rp, dtype=np.int32), cand=np.asarray(cand, dtype=np.float64))


def _rows(per):
    return np.concatenate([[0], np.cumsum(per)]).astype(np.int32), np.repeat(np.arange(len(per)), per)


@functools.lru_cache(maxsize=None)
def half_flat_case():
    """every left TOED edge with two candidates on its own scanline, at x = w / 2 + U(-14, 6): around the flat half's rim"""
    h, w = HALF_FLAT_SHAPE
    l, r = half_flat_pair(h, w)
    L = orc.toed(l)["edges"]
    rng = np.random.default_rng(21)
    rp, rows = _rows(np.full(len(L), 2))
    cand = np.stack([w / 2 + rng.uniform(-14, 6, len(rows)), L["y"][rows]], 1)
    return _case(l, r, L, rp, cand)


@functools.lru_cache(maxsize=None)
def steps_case():
    """left TOED edges of the step image, 0 .. 2 candidates each at x - 12 +- 2 on the scanline"""
    l, r = steps_pair(*STEPS_SHAPE)
    L = orc.toed(l)["edges"]
    rng = np.random.default_rng(22)
    rp, rows = _rows(rng.integers(0, 3, len(L)))
    cand = np.stack([L["x"][rows] - DISPARITY + rng.uniform(-2, 2, len(rows)), L["y"][rows]], 1)
    return _case(l, r, L, rp, cand)


@functools.lru_cache(maxsize=None)
def s2_case():
    """s2 at 96 x 160, one candidate list whose prefixes are the size cases: 0 .. 3 candidates per edge near the true mate
    (the first edge holds two, so that the one-edge case is a one-row CSR with pairs in it and not an empty call)"""
    l, r = synth.stereo_pair("s2", *S2_SHAPE)
    L = orc.toed(l)["edges"]
    rng = np.random.default_rng(23)
    per = rng.integers(0, 4, len(L))
    per[0] = 2
    rp, rows = _rows(per)
    cand = np.stack([L["x"][rows] - DISPARITY + rng.uniform(-2, 2, len(rows)), L["y"][rows] + rng.uniform(-1, 1, len(rows))], 1)
    return _case(l, r, L, rp, cand)


def sub_case(case, n_pairs=None, nL=None):
    """the first n_pairs pairs (rows after the last one stay, empty) or the first nL left edges of a case"""
    c = dict(case)
    if nL is not None:
        c["L"], c["lines"], c["rp"] = case["L"][:nL], case["lines"][:nL], case["rp"][:nL + 1]
        c["cand"] = case["cand"][:c["rp"][-1]]
    if n_pairs is not None:
        c["rp"] = np.minimum(c["rp"], n_pairs).astype(np.int32)
        c["cand"] = c["cand"][:n_pairs]
    return c


PAIR_COUNTS = (1, 7, 8, 9, 31, 32, 33, 255, 256, 257, 1025)   # around 8 lanes, 32 groups and 256 threads per block, > 1 block
LEFT_COUNTS = (1, 31, 32, 33, 257)                             # around gn_left_kernel's 32 edges per block
EMPTY_ROWS = 40


def row_shape_cases():
    """name -> case on s2 96 x 160, 600 pairs: the first / the last EMPTY_ROWS rows empty, one row holding every pair"""
    base = sub_case(s2_case(), nL=400)
    n = 600
    cand = s2_case()["cand"][:n]
    nL = len(base["L"])

    def with_rp(rp):
        return dict(base, rp=np.asarray(rp, dtype=np.int32), cand=cand)

    inner = np.minimum(base["rp"][:nL - EMPTY_ROWS + 1], n)
    inner[-1] = n
    first = np.concatenate([np.zeros(EMPTY_ROWS, np.int64), inner])
    last = np.concatenate([inner, np.full(EMPTY_ROWS, n)])
    one = np.concatenate([np.zeros(200, np.int64), np.full(nL - 199, n)])
    return {"first-rows-empty": with_rp(first), "last-rows-empty": with_rp(last), "one-row": with_rp(one)}


SMALL_SHAPES = ((32, 32), (33, 65), (36, 63))    # the smallest accepted image, one and one short of gn_pack_kernel's 64 columns


@functools.lru_cache(maxsize=None)
def small_case(h, w):
    """a pair too small for TOED to leave many edges: 150 left points anywhere in the image at any orientation, two
    candidates each near x - 4 (the patches of most reach over a border)"""
    l, r = synth.stereo_pair("s2", h, w, disparity=4)
    rng = np.random.default_rng(100 * h + w)
    L = np.zeros(150, dtype=orc.EDGE_DTYPE)
    L["x"], L["y"], L["theta"] = rng.uniform(0, w - 1, 150), rng.uniform(0, h - 1, 150), rng.uniform(-np.pi, np.pi, 150)
    L["index"] = np.arange(150)
    rp, rows = _rows(np.full(150, 2))
    cand = np.stack([L["x"][rows] - 4 + rng.uniform(-2, 2, 300), L["y"][rows] + rng.uniform(-0.5, 0.5, 300)], 1)
    return _case(l, r, L, rp, cand)


def border_points(h, w):
    """centres whose 7 x 7 patches (4.5 px to either side of the centre along the normal) are clamped at each of the four
    borders and the four corners, and finite centres far outside: +-1e6 and +-1e15 on either axis and on both.  A stereo
    candidate that far out samples one clamped pixel row / column or corner, a constant patch: it stops on H < 1e-8 in
    iteration 0 (validity 2, alpha 0, the candidate returned), so those rows check the clamp of huge coordinates and no
    more; the temporal starts there go on iterating (validity 0, |disp| ~ 1e15) and check the arithmetic too."""
    xs, ys = (-2.5, w / 2 + 0.25, w + 1.5), (-1.5, h / 2 + 0.75, h + 2.5)
    near = [(x, y) for x in xs for y in ys if (x, y) != (xs[1], ys[1])]
    far = [(sx * m, sy * m) for m in (1e6, 1e15) for sx, sy in ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, 1), (1, -1), (-1, -1))]
    far = [(x if x else w / 3, y if y else h / 3) for x, y in far]
    return np.array(near + far, dtype=np.float64)


def with_border_candidates(case):
    """the case plus one row per border point: the left edges are the case's first ones, again"""
    pts = border_points(*case["l"].shape)
    n = len(pts)
    L = np.concatenate([case["L"], case["L"][:n]])
    rp = np.concatenate([case["rp"], case["rp"][-1] + 1 + np.arange(n)]).astype(np.int32)
    return _case(case["l"], case["r"], L, rp, np.concatenate([case["cand"], pts]))


# --- temporal cases: dict(kf_img, cf_img, kf, cf, init) -------------------------------------------------------------------
def _temporal(kf_img, cf_img, kf, seed, n=None, sx=3, sy=2):
    rng = np.random.default_rng(seed)
    if n is not None:
        kf = kf[rng.choice(len(kf), n, replace=True)]
    cf = kf.copy()
    cf["x"] += sx
    cf["y"] += sy
    wrong = rng.random(len(kf)) < 0.3                               # 30 %: another edge's orientation and place
    cf["theta"][wrong] = rng.uniform(-np.pi, np.pi, int(wrong.sum()))
    cf["x"][wrong] += rng.uniform(-6, 6, int(wrong.sum()))
    init = np.stack([kf["x"] - cf["x"], kf["y"] - cf["y"]], 1) + rng.uniform(-1.5, 1.5, (len(kf), 2))
    return dict(kf_img=kf_img, cf_img=cf_img, kf=kf, cf=cf, init=init)


def _moved(gen, h, w, sx=3, sy=2):
    """keyframe image and a current frame whose content moved by (+sx, +sy) px"""
    return gen(h, w, 8, 8), gen(h, w, 8 - sx, 8 - sy)


@functools.lru_cache(maxsize=None)
def temporal_s2_case(n=1025):
    big = synth.s2_image(S2_SHAPE[0] + 16, S2_SHAPE[1] + 16, scene=7, noise_seed=1)
    kf_img, cf_img = _moved(lambda h, w, x0, y0: np.ascontiguousarray(big[y0:y0 + h, x0:x0 + w]), *S2_SHAPE)
    return _temporal(kf_img, cf_img, orc.toed(kf_img)["edges"], 31, n)


@functools.lru_cache(maxsize=None)
def temporal_steps_case():
    kf_img, cf_img = _moved(lambda h, w, x0, y0: steps_image(h, w, x0, y0), *STEPS_SHAPE)
    return _temporal(kf_img, cf_img, orc.toed(kf_img)["edges"], 32)


@functools.lru_cache(maxsize=None)
def temporal_half_flat_case():
    """the half-flat pair read as (keyframe, current frame): the current-frame points sit around the flat half's rim"""
    c = half_flat_case()
    rows = np.repeat(np.arange(len(c["L"])), np.diff(c["rp"]))
    kf = c["L"][rows]
    cf = kf.copy()
    cf["x"], cf["y"] = c["cand"][:, 0], c["cand"][:, 1]
    return dict(kf_img=c["l"], cf_img=c["r"], kf=kf, cf=cf, init=np.stack([kf["x"] - cf["x"], kf["y"] - cf["y"]], 1))


@functools.lru_cache(maxsize=None)
def temporal_small_case(h, w):
    c = small_case(h, w)
    return _temporal(c["l"], c["r"], c["L"], 33 + h, sx=-4, sy=0)


def temporal_sub(case, n):
    return dict(case, kf=case["kf"][:n], cf=case["cf"][:n], init=case["init"][:n])


def with_border_starts(case):
    """the case plus one item per border point: the start displacement puts the current-frame patch centre (kf - disp, the
    reference's :786) on the point"""
    pts = border_points(*case["kf_img"].shape)
    n = len(pts)
    kf, cf = case["kf"][:n], case["cf"][:n]
    init = np.stack([kf["x"] - pts[:, 0], kf["y"] - pts[:, 1]], 1)
    return dict(case, kf=np.concatenate([case["kf"], kf]), cf=np.concatenate([case["cf"], cf]), init=np.concatenate([case["init"], init]))


# --- references (computed once, never written to) ------------------------------------------------------------------------
def _frozen(kw):
    return tuple(sorted({**GN_DEFAULT, **kw}.items()))


def _readonly(out):
    for a in out.values():
        a.setflags(write=False)
    return out


def stereo_ref(case, **kw):
    return orc.gn_refine_stereo(case["l"], case["r"], case["L"], case["lines"], case["rp"], case["cand"], **{**GN_DEFAULT, **kw})


def temporal_ref(case, **kw):
    return orc.gn_refine_temporal(case["kf_img"], case["cf_img"], case["kf"], case["cf"], case["init"], **{**GN_DEFAULT, **kw})


@functools.lru_cache(maxsize=None)
def _named_ref(name, frozen):
    kw = dict(frozen)
    if name.startswith("temporal_"):
        return _readonly(temporal_ref(globals()[name + "_case"](), **kw))
    return _readonly(stereo_ref(globals()[name + "_case"](), **kw))


def named_ref(name, **kw):
    """the oracle's outputs of half_flat / steps / s2 / temporal_s2 / temporal_steps / temporal_half_flat under the
    parameters (defaults: the reference's constants), computed once"""
    return _named_ref(name, _frozen(kw))


# --- the active-pair profile and the hand-over thresholds ----------------------------------------------------------------
def profile(ref, max_iter):
    """pairs active on entering iteration it = 0 .. max_iter - 1, from the oracle's outputs alone: a pair that stops on
    H < 1e-8 (validity 2) in iteration `iters` was active in it, any other pair's last iteration is iters - 1.  This is what
    the device keeps in counts[it]."""
    last = np.where(ref["validity"] == 2, ref["iters"], ref["iters"] - 1)
    return np.array([int((last >= it).sum()) for it in range(max_iter)], dtype=np.int64)


def thresholds(prof):
    """the rows_below values (developer key 5) that put the stereo hand-over on the profile, and the iteration j they use:
       all       prof[0]      n_pairs > rows_below is false: the persistent launch alone
       all-1     prof[0] - 1  the thread layout runs iteration 0
       equal     prof[j]      a strict drop at j: iteration j is the first in the row layout, on n_active == rows_below
       equal-1   prof[j] - 1  iteration j still runs in the thread layout
       one       1
    j is the strict drop nearest to the middle of the iteration range: several iterations run in either layout."""
    drops = [j for j in range(2, len(prof) - 1) if 1 < prof[j] < prof[j - 1]]
    j = min(drops, key=lambda i: (abs(2 * i - len(prof)), i))
    return {"all": int(prof[0]), "all-1": int(prof[0]) - 1, "equal": int(prof[j]), "equal-1": int(prof[j]) - 1, "one": 1}, j


# --- the refinement inside the finalize chain ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_refinement(name="default"):
    """(case, oracle outputs) of the refinement that the finalize chain of tests/finalize_cases.py's pair runs with default
    parameters: the kept matches after the Best-Nearly-Best test, shifted to their epipolar lines -- the steps of
    oracle_chain.stereo_edge_pairs up to its call of gn_refine_stereo, on the oracle's first stage"""
    from tests import finalize_cases as fc
    from tests import oracle_chain as oc
    l, r = fc.images(name)
    s = fc.stage1(name)
    L, R, lines = fc.edges(name)
    k = s["keep"].astype(bool)
    cand, score, rp = R[s["col_idx"][k]].copy(), s["best"][k], oc.filter_rows(s["row_ptr"], k)
    cand["index"] = 0
    cnt, order = orc.bnb_test(rp, score, 0.9, True)
    idx, rp = oc.csr_select(rp, cnt, order)
    cand = orc.epipolar_shift(cand[idx], lines, rp)
    case = dict(l=l, r=r, L=L, lines=lines, rp=rp, cand=np.stack([cand["x"], cand["y"]], 1))
    return case, _readonly(stereo_ref(case))


def chain_thresholds(name="default"):
    """rows_below values for the chain's refinement: 1, and the active count on entering a mid iteration (a strict drop:
    the hand-over falls on the equality there)"""
    thr, j = thresholds(profile(chain_refinement(name)[1], GN_DEFAULT["max_iter"]))
    return (1, thr["equal"]), j
