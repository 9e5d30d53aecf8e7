"""Device-free companion of test_gpu_candidate_boxes.py: the cases of tests/candidate_box_cases.py are what they claim, and
the two chunk marks of the candidate walk, recomputed in numpy, are conservative on them -- every chunk that holds a pair
of the oracle's CSR is marked, by the region-box test for the flat edges and by the line test for the others."""
import numpy as np
import pytest

from tests import candidate_box_cases as cbc


def _marks(c, mask):
    boxes = cbc.chunk_boxes(c["R"])
    regions = cbc.region_boxes(c["L"], c["lines"], c["params"], mask)
    flat = cbc.flat_flags(c["lines"], c["params"], mask)
    fast = cbc.fast_marks(boxes, regions)
    line = cbc.line_marks(boxes, c["L"], c["lines"], c["params"], mask)
    return boxes, regions, flat, fast, line


@pytest.mark.parametrize("name", list(cbc.PARAMS))
def test_sizes_tiles_groups_and_batches(name):
    c = cbc.case(name)
    nL, nR = len(c["L"]), len(c["R"])
    assert nL == 130 and (nL + cbc.TILE - 1) // cbc.TILE == 3 and nL % cbc.TILE != 0
    nch = (nR + cbc.CHUNK - 1) // cbc.CHUNK
    assert 1000 <= nR <= 1300 and (nch + cbc.GROUP - 1) // cbc.GROUP == 3, (nR, nch)
    boxes, regions, *_ = _marks(c, 7)
    assert cbc.chunks_of_tile_union(boxes, regions, 0) > 64          # two staging batches
    assert set(c["kinds"][:8]) == set(cbc.KINDS) and c["kinds"][8:16] == c["kinds"][:8]   # all kinds in every wave
    assert {w for _, w, _ in c["special"]} == {"disparity", "band", "region"}


@pytest.mark.parametrize("name", list(cbc.PARAMS))
def test_flat_flags_are_what_the_kinds_say(name):
    c = cbc.case(name)
    flat = cbc.flat_flags(c["lines"], c["params"], 3)
    want = {"a=0": True, "below flat": True, "above flat": False, "45 deg": False, "b=0": True, "NaN": False,
            "a=b=0": False, "steep below flat": True}
    for k, kind in enumerate(c["kinds"]):
        assert flat[k] == want[kind], (k, kind)
    for mask in (1, 2, 4, 5, 6):                                      # without both stages nothing takes the fast mark
        assert not cbc.flat_flags(c["lines"], c["params"], mask).any()
    assert np.array_equal(cbc.flat_flags(c["lines"], c["params"], 7), flat)


@pytest.mark.parametrize("mask", cbc.MASKS)
@pytest.mark.parametrize("name", list(cbc.PARAMS))
def test_both_marks_keep_every_chunk_with_a_passing_pair(name, mask):
    c = cbc.case(name)
    rp, ci = cbc.reference(name, mask)
    assert rp[-1] == len(ci) > 0
    boxes, regions, flat, fast, line = _marks(c, mask)
    holds = np.zeros_like(fast)
    rows = np.repeat(np.arange(len(c["L"])), np.diff(rp))
    holds[rows, ci // cbc.CHUNK] = True
    # every passing pair lies inside its left edge's region box -- flat or not: the argument does not need the flag
    assert not (holds & ~fast).any(), np.argwhere(holds & ~fast)[:5]
    assert not (holds & ~line).any(), np.argwhere(holds & ~line)[:5]
    if (mask & 3) == 3:
        assert flat.any() and (~flat).any()                           # both paths populated
        assert holds[flat].any() and holds[~flat].any()               # ... by edges that have candidates
        # the filters filter: a flat edge's region box rejects chunks, and marks few that the line test does not
        assert (~fast[flat]).any() and (~line[~flat]).any()
        rect = np.array([k == "a=0" for k in c["kinds"]])
        # a = 0: the region box is the band ∩ square plus BOX_SLACK (1e-6 px); the only chunks it marks beyond the line
        # test are those that touch that margin -- the points this case puts on the region box's boundary
        assert not (line[rect] & ~fast[rect]).any()
        assert (fast[rect] & ~line[rect]).sum() <= 0.05 * line[rect].sum()


@pytest.mark.parametrize("name", list(cbc.PARAMS))
def test_boundary_points_are_on_their_boundaries(name):
    c = cbc.case(name)
    p, L, R = c["params"], c["L"], c["R"]
    seen = {"disparity": set(), "band": set()}
    for li, what, j in c["special"]:
        if what == "disparity":
            assert R["y"][j] == L["y"][li]
            seen[what].add(np.sign((L["x"][li] - R["x"][j]) - p["max_disp"]))
        elif what == "band":
            a, b, cc = c["lines"][li]
            d = abs(a * R["x"][j] + b * R["y"][j] + cc) / np.sqrt(a * a + b * b)
            assert abs(d - p["epi_thr"]) < 1e-12
            seen[what].add(np.sign(d - p["epi_thr"]))
    assert seen["disparity"] == {-1.0, 0.0, 1.0}                       # exactly max_disp and one ulp either side
    assert {-1.0, 1.0} <= seen["band"]
    # ... and they decide pairs: the exact-disparity point of an a = 0 edge is a candidate under the disparity stage alone
    rp, ci = cbc.reference(name, 2)
    li, _, j = next(s for s in c["special"] if s[1] == "disparity" and L["x"][s[0]] - R["x"][s[2]] == p["max_disp"])
    assert j in ci[rp[li]:rp[li + 1]]
    li, _, j = next(s for s in c["special"] if s[1] == "disparity" and L["x"][s[0]] - R["x"][s[2]] > p["max_disp"])
    assert j not in ci[rp[li]:rp[li + 1]]


def test_some_rows_pass_the_staging_area():
    n = {name: np.diff(cbc.reference(name, 7)[0]) for name in cbc.PARAMS}
    for name in cbc.PARAMS:                                             # long, short and empty rows together
        flat = cbc.flat_flags(cbc.case(name)["lines"], cbc.PARAMS[name], 7)
        assert (n[name][flat] > cbc.STAGE).any(), name
        assert ((n[name] > 0) & (n[name] <= cbc.STAGE)).any() and (n[name] == 0).any(), name
    flat = cbc.flat_flags(cbc.case("wide")["lines"], cbc.PARAMS["wide"], 7)
    assert (n["wide"][~flat] > cbc.STAGE).any()                         # the line test's edges have long rows as well
