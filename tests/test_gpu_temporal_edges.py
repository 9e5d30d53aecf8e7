"""The temporal chain (ebvo_temporal_set_keyframe / _match[_submit / _wait] / _fetch / _fetch_final / _estimate_pose) across
launch grids, counts on the kernels' work units, empty middles, frame sizes and slots -- every candidate quad, both NCC
maxima, the keep flags and every final quad against oracle_chain.temporal_reference, bit for bit; the pose against
tests/oracle_pose.py.  No device output is ever passed to the oracle: the reference is computed from the ORACLE's stereo
mates (tests/temporal_cases.py), and the device's mates -- its stereo chain, which the other GPU files pin -- are asserted
equal to those before every match.  The temporal stages do not depend on the detector mode, so the oracle side is computed
once per process and both modes are compared with it.

Launches of temporal_stage0_enqueue, in order, and the developer key (ebvo_debug_set) that moves each grid:
  mate_cells_kernel              22      cell_scan_kernel               one block by construction
  cell_scatter_kernel            22      cell_sort_kernel               22
  temporal_candidates<count>     22      scan_apply (+ scan_reduce)     one block per 4096-entry tile: no cap to move
  temporal_candidates<fill>      22      expand_rows_kernel             22
  sincos_batch + patches (x2)    22      ncc_quads_indexed_kernel       22
  count_flags_kernel             22
and of temporal_chain:
  rows_from_flags, row_index, gather (every compaction), bnb (x2), quad_refine_inputs (x2), quad_apply_refine, cluster,
  quad_cluster_post: 22 (the glue's own cap, 2048 blocks of 256, lies above every count here; key 18 divides grids of the
  stereo chain only and reaches none of these)
  sift_blur_rows / _cols, gn_pack: one thread per pixel, no loop    sift_desc, sift_gather, sift_dist, and_flags: 22
  gn2_init, gn2_rows_persistent | gn2_iter_rows | gn2_iter: 22 for the grid, keys 4 / 7 for the layout (keys 5, 8, 9 belong
  to the stereo refinement and do not reach the temporal one)
  count_flags: 22

Counts of the committed cases (tests/test_temporal_cases.py recomputes them without a GPU): see temporal_cases.UNIT_CASES
and temporal_cases.EXPECTED.  No image of the search had fewer than the smallest n_kf / n_cf listed there.

The two refusals (a keyframe of another size with stages = 1; ebvo_temporal_set_keyframe while any slot has a match in
flight) are exercised as refusals only: what the library did before them is not run."""
import contextlib

import numpy as np
import pytest

from edge_based_visual_odometry_amd import synth
from edge_based_visual_odometry_amd._lib import EBVO_ERR_ARG, EBVO_ERR_STATE, EbvoError
from edge_based_visual_odometry_amd.api import Context
from tests import oracle_chain
from tests import oracle_pose as op
from tests import temporal_cases as tc
from tests import test_gpu_fullsize_temporal as fs
from tests.test_gpu_pose import assert_same
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu

F, CALIB = tc.rig()
ORACLE_NAME = dict(cell_size="cell", grid_radius="radius", orient_thr_deg="orient_thr_deg", ncc_thr="ncc_thr",
                   sift_thr="sift_thr", bnb_ncc="bnb_ncc", bnb_sift="bnb_sift")
STAGE0 = ("row_ptr", "col_idx", "sim_left", "sim_right", "keep")
FINAL = ("row_ptr", "cf_index", "ncc_left", "sift_left", "score_left", "score_right", "valid")


def new_context(mode, slots=3):
    c = Context(*synth.SHAPES["euroc"], device=0, toed_mode=mode)
    c.set_slots(slots)
    return c


@pytest.fixture(scope="module", params=["strict", "hybrid"])
def tctx(request):
    """A context of these tests' own (key 22 can never reach the session context), sized for the full EuRoC frame"""
    c = new_context(request.param)
    yield c
    c.close()


@contextlib.contextmanager
def keys(c, settings):
    try:
        for k, v in settings.items():
            c.debug_set(k, v)
        yield
    finally:
        for k in settings:
            c.debug_set(k, 0)


def load(c, name, slot=0):
    """the named frame through the stereo chain of `slot`; its mates are the oracle's"""
    l, r = tc.images(name)
    c.stereo_upload(l, r, slot=slot)
    c.stereo_submit(c.default_params(F), slot=slot)
    cnt = c.stereo_wait(slot=slot)
    left = c.stereo_fetch(cnt, slot=slot)["left"]
    _, fin = c.stereo_finalize(CALIB, slot=slot)
    oL, oR = tc.oracle_mates(name)
    for got, ref, what in ((left[fin["left_index"]], oL, "left"), (fin["right"], oR, "right")):
        assert len(got) == len(ref), (name, what, len(got), len(ref))
        for f in ("x", "y", "theta"):
            assert_bit_equal(got[f].copy(), ref[f].copy(), f"{name}: {what} mate {f}")


def reference_of(kf, cf, kw):
    okw = {ORACLE_NAME[k]: v for k, v in kw.items() if k != "stages"}
    return tc.reference(kf, cf, None, bool(kw.get("stages", 0)), **okw)


def assert_matches_oracle(counts, q, kf, cf, kw, what=""):
    ref = reference_of(kf, cf, kw)
    bad = oracle_chain.temporal_problems(counts, q, ref)
    assert bad == [], (what, kf, cf, kw, bad)
    return ref


def match(c, kf, cf, slot=0, what="", **kw):
    counts, q = c.temporal_match(slot=slot, **kw)
    ref = assert_matches_oracle(counts, q, kf, cf, kw, what)
    return counts, q, ref


def same_results(a, b, what):
    for k in STAGE0:
        assert_bit_equal(a[k], b[k], f"{what}: {k}")
    if "final" in a or "final" in b:
        for k in FINAL:
            assert_bit_equal(a["final"][k], b["final"][k], f"{what}: final.{k}")
        for k in ("left", "right"):
            assert oracle_chain._same_edges(a["final"][k], b["final"][k]), f"{what}: final.{k}"


# --- A. launch grids ----------------------------------------------------------------------------------------------------
GRIDS = [{22: 1}, {22: 3}, {22: 64}, {22: 0}]
GRIDS_CHAIN = GRIDS + [{22: 1, 4: 1}, {22: 3, 7: 1}, {22: 64, 4: 1, 7: 1}]   # with the refinement's other launch layouts


@pytest.mark.parametrize("stages", [0, 1])
def test_grid_cap_changes_no_bit(tctx, stages):
    load(tctx, "kf")
    tctx.temporal_set_keyframe()
    load(tctx, "cf2")
    seen = None
    for settings in (GRIDS_CHAIN if stages else GRIDS):
        with keys(tctx, settings):
            counts, q, ref = match(tctx, "kf", "cf2", what=str(settings), stages=stages)
        seen = counts
    assert seen["n_kf"] > 4000 and seen["n_candidates"] > 10 * seen["n_kf"] and (not stages or seen["n_final"] > 1000)


def test_refused_grid_cap_changes_nothing(tctx):
    load(tctx, "kf")
    tctx.temporal_set_keyframe()
    load(tctx, "cf2")
    with keys(tctx, {22: 3}):
        for bad in (65537, 1 << 30, -1):
            with pytest.raises(EbvoError) as ei:
                tctx.debug_set(22, bad)
            assert ei.value.status == EBVO_ERR_ARG, bad
        match(tctx, "kf", "cf2", what="after refused values", stages=1)
    tctx.debug_set(22, 65536)
    match(tctx, "kf", "cf2", what="largest accepted value", stages=1)
    tctx.debug_set(22, 0)


_FULL = {}   # the full-size oracle run, made once per process: (mates, reference)


def test_grid_cap_at_full_size(tctx):
    """EuRoC 752x480 with undistortion (tests/test_gpu_fullsize_temporal.py's case): one block per launch against the
    default-grid run, which is checked against the oracle once."""
    cfg, k, undist = fs.CASES["euroc-752x480-undistort"]
    h, w = synth.SHAPES[cfg]
    cal = synth.CALIB[cfg]
    calib = fs.calib_of(cfg)
    params = tctx.default_params(synth.fundamental_for(cfg))
    tctx.set_undistort(cal["K"], cal["dist"], cal["K_right"], cal["dist_right"])
    try:
        f0, fk = fs.sequence_frame(cfg, 0), fs.sequence_frame(cfg, k)
        kfL, kfR = fs.mates_of(tctx, f0, params, calib)
        tctx.temporal_set_keyframe()
        cfL, cfR = fs.mates_of(tctx, fk, params, calib)
        counts0, q0 = tctx.temporal_match(stages=1)
        with keys(tctx, {22: 1}):
            counts1, q1 = tctx.temporal_match(stages=1)
    finally:
        tctx.set_undistort()
    mates = (kfL, kfR, cfL, cfR)
    if not _FULL:
        _FULL["mates"] = mates
        _FULL["ref"] = oracle_chain.temporal_reference(*mates, fs.image_triple(f0, cal, undist), fs.image_triple(fk, cal, undist), w, h)
    assert all(oracle_chain._same_edges(a, b) for a, b in zip(mates, _FULL["mates"]))   # the modes give the same mates
    assert oracle_chain.temporal_problems(counts0, q0, _FULL["ref"]) == []
    assert counts1 == counts0 and counts0["n_kf"] > 10000 and counts0["n_candidates"] > 131072
    same_results(q1, q0, "key 22 = 1 at full size")


# --- B. counts on the work units ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(tc.UNIT_CASES))
def test_counts_on_work_units(tctx, case):
    kf, cf, cell, stages = tc.UNIT_CASES[case]
    exp = tc.EXPECTED[case]
    load(tctx, kf)
    tctx.temporal_set_keyframe()
    load(tctx, cf)
    counts, q, ref = match(tctx, kf, cf, what=case, cell_size=cell, stages=stages)
    assert (counts["n_kf"], counts["n_cf"]) == (exp["n_kf"], exp["n_cf"])
    with keys(tctx, {22: 1}):
        match(tctx, kf, cf, what=case + ", one block", cell_size=cell, stages=stages)


# --- C. empty middles ---------------------------------------------------------------------------------------------------
def _empty_cases():
    levels, below, _ = tc.sift_levels("kf", "cf2")
    return {
        "nothing-kept": (dict(ncc_thr=2.0), lambda c: c["n_candidates"] > 0 and c["n_kept"] == 0),
        "nothing-passes-sift": (dict(sift_thr=float(levels[0])), lambda c: c["n_kept"] > 0 and c["n_sift"] == 0),
        "no-candidates": (dict(orient_thr_deg=0.0), lambda c: c["n_kf"] > 0 and c["n_cf"] > 0 and c["n_candidates"] == 0),
    }


@pytest.mark.parametrize("case", ["nothing-kept", "nothing-passes-sift", "no-candidates"])
def test_empty_middle(tctx, case):
    kw, intended = _empty_cases()[case]
    load(tctx, "kf")
    tctx.temporal_set_keyframe()
    load(tctx, "cf2")
    match(tctx, "kf", "cf2", what="before", stages=1)                # a full final list sits in the slot's buffers
    counts, q, ref = match(tctx, "kf", "cf2", what=case, stages=1, **kw)
    assert intended(ref["counts"]) and ref["counts"]["n_final"] == 0   # the oracle says this is the intended exit
    fin = q["final"]
    assert_bit_equal(fin["row_ptr"], np.zeros(counts["n_kf"] + 1, dtype=np.int32), "final row_ptr")
    assert all(len(fin[k]) == 0 for k in FINAL[1:] + ("left", "right"))
    got = tctx.temporal_estimate_pose(CALIB)                         # (sizes its mask by ebvo_temporal_final_size: 0)
    assert got["status"] == 1 and not got["found"] and got["n_quads"] == 0 and got["draws"] == 0
    assert (got["R"] == np.eye(3)).all() and (got["t"] == 0).all() and len(got["inlier"]) == 0
    match(tctx, "kf", "cf2", what="right after " + case, stages=1)   # no stale state


@pytest.mark.parametrize("n", [1, 2])
def test_final_list_of_one_and_two_quads(tctx, n):
    levels, below, _ = tc.sift_levels("kf", "cf2")
    assert below[n] == n and levels[n] > 0                            # sift_thr ON a realized distance: exactly n quads below it
    load(tctx, "kf")
    tctx.temporal_set_keyframe()
    load(tctx, "cf2")
    counts, q, ref = match(tctx, "kf", "cf2", stages=1, sift_thr=float(levels[n]))
    assert counts["n_sift"] == n == counts["n_final"]
    kfL, kfR = tc.oracle_mates("kf")
    rf = ref["final"]
    for kw in (dict(), dict(top_rank_fraction=1.0)):
        got = tctx.temporal_estimate_pose(CALIB, **kw)
        assert_same(got, op.estimate_pose(kfL, kfR, rf["row_ptr"], rf["left"], rf["right"], CALIB[0], CALIB[2], CALIB[3], **kw),
                    geom=False)
        assert got["n_quads"] == n == len(got["inlier"])


# --- D. frame sizes -----------------------------------------------------------------------------------------------------
def _fetch(c, counts, stages, slot=0):
    from tests.test_gpu_pose import _fetch_counts
    return c._temporal_results(slot, _fetch_counts(counts), stages, True)[1]


@pytest.mark.parametrize("kf,cf,same", [("kf", "small2", "cf2"), ("small0", "cf2", "small2")])
def test_keyframe_and_frame_of_different_sizes(tctx, kf, cf, same):
    load(tctx, kf)
    tctx.temporal_set_keyframe()
    load(tctx, same)
    counts_s, q_s, _ = match(tctx, kf, same, what="same size", stages=1)
    before = _fetch(tctx, counts_s, 1)
    # stages = 1 across sizes: refused, and the slot's quads of the frame before stay where they were ... but the slot now
    # holds another pair, so the refusal is shown on the slot the earlier quads live in: slot 1 takes the other size
    load(tctx, cf, slot=1)
    with pytest.raises(EbvoError) as ei:
        tctx.temporal_match(slot=1, stages=1)
    assert ei.value.status == EBVO_ERR_STATE and "size" in str(ei.value)
    same_results(_fetch(tctx, counts_s, 1), before, "slot 0 after the refusal in slot 1")
    # stages = 0 across sizes, on the CURRENT frame's grid
    counts, q, ref = match(tctx, kf, cf, slot=1, what="across sizes", stages=0)
    assert counts["n_candidates"] > counts["n_kf"] // 8 > 0
    if kf == "kf":
        out, clipped = tc.rows_outside_grid(kf, cf)                  # keyframe mates whose query cell is outside the grid
        assert len(out) > 1000 and len(clipped) > 1000
        rows = np.diff(q["row_ptr"])
        assert_bit_equal(rows[out], np.diff(ref["row_ptr"])[out], "rows of mates outside the current grid")
        assert rows[out].sum() > 0 and rows[clipped].sum() == 0      # some still reach the grid's edge; a clipped walk finds none
    # the refusal on a slot that holds quads: they stay fetchable, bit for bit
    kept = _fetch(tctx, counts, 0, slot=1)
    with pytest.raises(EbvoError) as ei:
        tctx.temporal_match(slot=1, stages=1)
    assert ei.value.status == EBVO_ERR_STATE
    same_results(_fetch(tctx, counts, 0, slot=1), kept, "slot 1 after its own refusal")
    # a same-size frame through the whole chain, in the slot that was just refused
    load(tctx, same, slot=1)
    match(tctx, kf, same, slot=1, what="same size after the refusals", stages=1)


def test_keyframe_store_grows_and_shrinks(tctx):
    """a context of its own: the first keyframe is the smallest, so every later one re-allocates (mates, then images too);
    the last one is small again under buffers sized for the largest"""
    c = new_context(tctx.toed_mode, slots=1)
    try:
        for kf, cf in (("k3", "small2"), ("small0", "small2"), ("kf", "cf2"), ("k3", "small2"), ("kf", "cf3")):
            load(c, kf)
            c.temporal_set_keyframe()
            load(c, cf)
            match(c, kf, cf, what=f"keyframe {kf}", stages=1)
    finally:
        c.close()


# --- E. slots -----------------------------------------------------------------------------------------------------------
def test_keyframe_from_another_slot_and_replacement_in_flight(tctx):
    load(tctx, "kf", slot=2)
    tctx.temporal_set_keyframe(slot=2)                               # keyframe A from slot 2 of 3
    load(tctx, "cf2", slot=2)                                        # the slot it came from, after re-upload
    load(tctx, "cf3", slot=1)
    match(tctx, "kf", "cf2", slot=2, stages=1)
    match(tctx, "kf", "cf3", slot=1, stages=1)
    # two slots in flight against A, fetched after both waits
    tctx.temporal_match_submit(slot=1, stages=1)
    tctx.temporal_match_submit(slot=2, stages=1)
    r2 = tctx.temporal_match_wait(slot=2)
    r1 = tctx.temporal_match_wait(slot=1)
    assert_matches_oracle(*r1, "kf", "cf3", dict(stages=1), "slot 1 against A")
    assert_matches_oracle(*r2, "kf", "cf2", dict(stages=1), "slot 2 against A")
    # keyframe B from slot 0; both slots again
    load(tctx, "cf2", slot=0)
    tctx.temporal_set_keyframe(slot=0)
    same_results(_fetch(tctx, r1[0], 1, slot=1), r1[1], "slot 1's quads against A after the keyframe changed")
    match(tctx, "cf2", "cf3", slot=1, stages=1)
    match(tctx, "cf2", "cf2", slot=2, stages=1)
    # no replacement under a match in flight
    load(tctx, "kf", slot=0)
    tctx.temporal_match_submit(slot=1, stages=1)
    with pytest.raises(EbvoError) as ei:
        tctx.temporal_set_keyframe(slot=0)
    assert ei.value.status == EBVO_ERR_STATE and "in flight" in str(ei.value)
    got = tctx.temporal_match_wait(slot=1)
    assert_matches_oracle(*got, "cf2", "cf3", dict(stages=1), "against the OLD keyframe")
    assert tctx.temporal_estimate_pose(CALIB, slot=1)["n_quads"] == got[0]["n_final"]
    tctx.temporal_set_keyframe(slot=0)                               # nothing in flight: the replacement succeeds
    with pytest.raises(EbvoError) as ei:                             # quads of the old keyframe give no pose
        tctx.temporal_estimate_pose(CALIB, slot=1)
    assert ei.value.status == EBVO_ERR_STATE
    match(tctx, "kf", "cf3", slot=1, stages=1)
