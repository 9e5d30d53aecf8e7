"""The candidate walk marks the staged chunks of a left edge either against the edge's region box (both the epipolar and the
disparity stage enabled, line nearly parallel to an axis) or against the line itself; the CSR must be the brute force's
either way.  The synthetic cases of tests/candidate_box_cases.py (what they contain is asserted without a device in
test_candidate_box_cases.py) go through ebvo_epi_candidates -- count, scan, fill -- under every stage mask, and row_ptr
and col_idx must equal the oracle's element for element; one resident pair with the non-rectified EuRoC calibration must
give the host-buffer call's CSR."""
import functools

import numpy as np
import pytest

from edge_based_visual_odometry_amd import synth
from tests import candidate_box_cases as cbc
from tests import oracle as orc
from tests.util import assert_bit_equal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mask", cbc.MASKS)
@pytest.mark.parametrize("name", list(cbc.PARAMS))
def test_csr_of_the_synthetic_cases_is_the_oracles(ctx, name, mask):
    c = cbc.case(name)
    ref_rp, ref_ci = cbc.reference(name, mask)
    rp, ci = ctx.epi_candidates(c["L"], c["R"], c["lines"], stage_mask=mask, **c["params"])
    assert_bit_equal(rp, ref_rp, f"{name}, mask {mask}: row_ptr")
    assert_bit_equal(ci, ref_ci, f"{name}, mask {mask}: col_idx")


@pytest.mark.parametrize("name", list(cbc.PARAMS))
def test_csr_does_not_depend_on_the_left_edges_neighbours(ctx, name):
    """the same left edges in reverse order meet other edges in their wave and tile: every row must stay what it was"""
    c = cbc.case(name)
    ref_rp, ref_ci = cbc.reference(name, 7)
    rp, ci = ctx.epi_candidates(c["L"][::-1].copy(), c["R"], c["lines"][::-1].copy(), stage_mask=7, **c["params"])
    n = len(c["L"])
    assert_bit_equal(np.diff(rp), np.diff(ref_rp)[::-1].copy(), f"{name}: row lengths")
    for i in (0, 1, 2, 5, 63, 64, 65, n - 1):
        assert_bit_equal(ci[rp[n - 1 - i]:rp[n - i]], ref_ci[ref_rp[i]:ref_rp[i + 1]], f"{name}: row {i}")


H, W = 120, 160
F_EUROC = synth.fundamental_for("euroc")


@functools.lru_cache(maxsize=None)
def _euroc_ref():
    l, r = synth.stereo_pair("s2", H, W)
    L, R = orc.toed(l)["edges"], orc.toed(r)["edges"]
    return l, r, L, R, orc.epi_candidates(L, R, orc.epipolar_lines(F_EUROC, L))


def test_resident_pair_with_a_tilted_calibration(ctx):
    l, r, L, R, (ref_rp, ref_ci) = _euroc_ref()
    assert len(L) > 2 * cbc.TILE and ref_rp[-1] > 0
    ctx.stereo_upload(l, r)
    p = ctx.default_params(F_EUROC)
    ctx.stereo_submit(p, 0)
    c = ctx.stereo_wait(0)
    out = ctx.stereo_fetch(c, slot=0)
    assert_bit_equal(out["row_ptr"], ref_rp, "resident: row_ptr against the oracle")
    assert_bit_equal(out["col_idx"], ref_ci, "resident: col_idx against the oracle")
    assert c.n_pairs == len(ref_ci)
    lines = ctx.epipolar_lines(F_EUROC, out["left"])
    rp, ci = ctx.epi_candidates(out["left"], out["right"], lines)      # replaces the host slot's pair: last
    assert_bit_equal(out["row_ptr"], rp, "resident: row_ptr against ebvo_epi_candidates")
    assert_bit_equal(out["col_idx"], ci, "resident: col_idx against ebvo_epi_candidates")
