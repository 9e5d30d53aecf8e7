"""cv::undistort on the device (ebvo_undistort, and inside the resident pipeline via ebvo_stereo_set_undistort) against the
oracle's restatement: byte-exact.  With undistortion on, TOED and the refinement run on the undistorted images while
both NCC passes sample the RAW ones, as the reference does (src/Pipeline.cpp:78-99 vs src/Stereo_Matches.cpp:562-563)."""
import numpy as np
import pytest

from edge_based_visual_odometry_amd import synth
from tests import oracle as orc
from tests import oracle_chain
from tests.util import assert_bit_equal, assert_edges_equal

pytestmark = pytest.mark.gpu

CE = synth.CALIB["euroc"]


@pytest.mark.parametrize("shape", [(480, 752), (120, 200), (97, 131)])
@pytest.mark.parametrize("cam", ["left", "right"])
def test_undistort_equals_oracle(ctx, shape, cam):
    img = synth.s2_image(*shape, noise_seed=3)
    K, d = (CE["K"], CE["dist"]) if cam == "left" else (CE["K_right"], CE["dist_right"])
    if shape != (480, 752):                         # keep the principal point inside the smaller test images
        K = (K[0] * shape[1] / 752, K[1] * shape[0] / 480, K[2] * shape[1] / 752, K[3] * shape[0] / 480)
    got = ctx.undistort(img, K, d)
    ref = orc.undistort(img, K, d)
    assert (got == ref).all(), f"{int((got != ref).sum())} pixels differ"
    assert (got != img).mean() > 0.3
    assert (ctx.undistort(img, K, [0, 0, 0, 0]) == img).all()      # zero distortion: identity
    got5 = ctx.undistort(img, K, list(d) + [0.01])                  # k3
    assert (got5 == orc.undistort(img, K, list(d) + [0.01])).all()
    wide = np.zeros((shape[0], shape[1] + 13), dtype=np.uint8)      # strided input
    wide[:, :shape[1]] = img
    assert (ctx.undistort(wide[:, :shape[1]], K, d) == ref).all()


def test_resident_pipeline_with_undistortion(ctx):
    h, w = 240, 376
    K = (CE["K"][0] / 2, CE["K"][1] / 2, CE["K"][2] / 2, CE["K"][3] / 2)
    Kr = (CE["K_right"][0] / 2, CE["K_right"][1] / 2, CE["K_right"][2] / 2, CE["K_right"][3] / 2)
    F = synth.fundamental_21(K, Kr, CE["R21"], CE["T21"])
    l, r = synth.stereo_pair("s2", h, w, disparity=9)
    lu, ru = orc.undistort(l, K, CE["dist"]), orc.undistort(r, Kr, CE["dist_right"])
    kl = [K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1]
    kr = [Kr[0], 0, Kr[2], 0, Kr[1], Kr[3], 0, 0, 1]
    calib = (kl, kr, CE["R21"], CE["T21"])
    ctx.set_undistort(K, CE["dist"], Kr, CE["dist_right"])
    try:
        ctx.stereo_upload(l, r)
        c = ctx.stereo_run(ctx.default_params(F))
        out = ctx.stereo_fetch(c, patches=True)
        counts, fin = ctx.stereo_finalize(calib)
    finally:
        ctx.set_undistort()
    # stage by stage on the oracle: TOED on the undistorted images, candidates, NCC on the RAW images
    L, R = orc.toed(lu)["edges"], orc.toed(ru)["edges"]
    assert_edges_equal(out["left"], L, "left edges (undistorted image)")
    assert_edges_equal(out["right"], R, "right edges (undistorted image)")
    lines = orc.epipolar_lines(F, L)
    rp, ci = orc.epi_candidates(L, R, lines)
    assert_bit_equal(out["row_ptr"], rp, "row_ptr")
    assert_bit_equal(out["col_idx"], ci, "col_idx")
    sims, best, keep, lp = orc.ncc_pairs(l, r, L, R[ci], rp)
    assert_bit_equal(out["sims"], sims, "sims (raw images)")
    assert_bit_equal(out["keep"], keep, "keep")
    assert_bit_equal(out["left_patches"], lp, "left patches (raw image)")
    sims_u, _, _, _ = orc.ncc_pairs(lu, ru, L, R[ci], rp)
    assert not np.array_equal(sims_u, sims)                          # the distinction is observable in this fixture
    ref = oracle_chain.stereo_edge_pairs(l, r, F, calib, left_img_undist=lu, right_img_undist=ru)
    assert counts == ref["counts"] and counts["n_final"] > 100
    assert_bit_equal(fin["left_index"], ref["left_index"], "left_index")
    assert_edges_equal(fin["right"], ref["right"], "right centre")
    assert_bit_equal(fin["score"], ref["score"], "score")
    assert_bit_equal(fin["rows"], ref["rows"], "rows")
    # switched off again: the same raw pair gives the plain result
    ctx.stereo_upload(l, r)
    c2 = ctx.stereo_run(ctx.default_params(F))
    assert_edges_equal(ctx.stereo_fetch(c2)["left"], orc.toed(l)["edges"])


# ---- the branches no EuRoC-like model reaches: borders, the (short) wrap, saturation, stripes of 1 .. 3 rows --------------------
# (tests/undistort_cases.py; tests/test_undistort_cases.py shows on the CPU that every case reaches its branch and that a second
# reading of the algorithm agrees with the oracle there)
import ctypes as C

from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG
from edge_based_visual_odometry_amd.api import Context
from tests import undistort_cases as uc

F_KITTI = synth.fundamental_for("kitti")


@pytest.fixture(scope="module")
def wide_ctx():
    """the stripe cases are wider than the session context"""
    c = Context(*uc.WIDE_CONTEXT, device=0)
    yield c
    c.close()


def _oracle(name):
    _, K, dist = uc.CASES[name]
    return orc.undistort(uc.image(name), K, dist)


def _check_case(c, name):
    (h, w), K, dist = uc.CASES[name]
    img, ref = uc.image(name), _oracle(name)
    got = c.undistort(img, K, dist)
    assert (got == ref).all(), f"{name}: {int((got != ref).sum())} pixels differ, first at {np.argwhere(got != ref)[:4].tolist()}"
    wide = np.full((h, w + 13), 201, dtype=np.uint8)             # strided input: the padding must never be sampled
    wide[:, :w] = img
    got = c.undistort(wide[:, :w], K, dist)
    assert (got == ref).all(), f"{name} (strided): {int((got != ref).sum())} pixels differ"


@pytest.mark.parametrize("name", [n for n in uc.CASES if n not in uc.WIDE])
def test_border_wrap_and_saturation_cases_equal_oracle(ctx, name):
    _check_case(ctx, name)


@pytest.mark.parametrize("name", uc.WIDE)
def test_stripe_cases_equal_oracle(wide_ctx, name):
    _check_case(wide_ctx, name)


def _raw_undistort(c, img, h, w, K, dist, out, out_stride, n_dist=None):
    K = np.ascontiguousarray(K, dtype=np.float64)
    dist = np.ascontiguousarray(dist, dtype=np.float64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    return c.lib.ebvo_undistort(c._ctx, p(img), h, w, img.strides[0], p(K), p(dist), len(dist) if n_dist is None else n_dist,
                                p(out), out_stride)


def test_padded_output_rows_and_refusals(ctx):
    """ebvo_undistort with out_stride != w (the 2-D copy back, which api.undistort never asks for), and the argument checks"""
    name = "pincushion"
    (h, w), K, dist = uc.CASES[name]
    img = np.ascontiguousarray(uc.image(name))
    out = np.full((h, w + 7), 0xA5, dtype=np.uint8)
    assert _raw_undistort(ctx, img, h, w, K, dist, out, w + 7) == 0
    assert (out[:, :w] == _oracle(name)).all()
    assert (out[:, w:] == 0xA5).all()                                # the padding bytes are untouched
    before = out.copy()
    six = list(dist) + [0.0, 0.0]
    assert _raw_undistort(ctx, img, h, w, K, six, out, w + 7, n_dist=6) == EBVO_ERR_ARG
    assert _raw_undistort(ctx, img, h, w, K, dist, out, w - 1) == EBVO_ERR_ARG
    assert _raw_undistort(ctx, img, 31, w, K, dist, out, w + 7) == EBVO_ERR_ARG
    assert (out == before).all()                                     # a refused call writes nothing


def test_resident_pipeline_samples_over_the_border(ctx):
    """set_undistort with two models that leave the image (left: pincushion, right: corner_pp): the detector then runs on images
    with black regions, whose rims are edges themselves"""
    h, w = 97, 131
    _, K, d = uc.CASES["pincushion"]
    _, Kr, dr = uc.CASES["corner_pp"]
    l, r = synth.stereo_pair("s2", h, w)
    lu, ru = orc.undistort(l, K, d), orc.undistort(r, Kr, dr)
    ctx.set_undistort(K, d, Kr, dr)
    try:
        ctx.stereo_upload(l, r)
        c = ctx.stereo_run(ctx.default_params(F_KITTI))
        out = ctx.stereo_fetch(c)
    finally:
        ctx.set_undistort()
    L, R = orc.toed(lu)["edges"], orc.toed(ru)["edges"]
    assert_edges_equal(out["left"], L, "left edges (undistorted image)")
    assert_edges_equal(out["right"], R, "right edges (undistorted image)")
    rp, ci = orc.epi_candidates(L, R, orc.epipolar_lines(F_KITTI, L))
    assert len(ci) > 1000
    assert_bit_equal(out["row_ptr"], rp, "row_ptr")
    assert_bit_equal(out["col_idx"], ci, "col_idx")
    sims, _, keep, _ = orc.ncc_pairs(l, r, L, R[ci], rp)
    assert_bit_equal(out["sims"], sims, "sims (raw images)")
    assert_bit_equal(out["keep"], keep, "keep")
    assert not np.array_equal(orc.ncc_pairs(lu, ru, L, R[ci], rp)[0], sims)
    # the border is really in play: left edges next to the region that no source pixel reaches
    from tests import undistort_reading as ur
    black = ur.undistort(l, K, d)[1]["none_mask"]
    assert black.sum() >= 1000 and (lu[black] == 0).all()
    x, y = np.rint(L["x"]).astype(int), np.rint(L["y"]).astype(int)
    near = [black[max(0, b - 3):b + 4, max(0, a - 3):a + 4].any() for a, b in zip(x, y)]
    assert sum(near) >= 1
