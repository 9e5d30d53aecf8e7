"""The word-wise candidate and neighbour lists of the hybrid detector (toed_compact_phase_kernel, toed_need_compact_kernel:
one wave per grid row, eight flag bytes or one bitmap word per lane) at the smallest shapes where their indexing can go wrong.

A wrong rank, a missing list entry or a wrong list length shows as a differing edge list, so the check is the detector's
edges -- x, y, theta bits, index -- against tests/oracle.py, for one image and for a batch of two.

ebvo_ctx_create accepts no side below 32, so the shapes asked for below that are replaced by the smallest accepted ones with
the same residues: heights 32 and 33 for 24 and 25 (both parities of the last grid rows, which publish the neighbour lists'
lengths), and widths 35 and 34 for 15 and 18 (2W - 20 = 50 and 48: a partial last lane, 50 = 10 mod 8, and a whole number of
lanes).  The other widths are the asked ones: 2W - 20 = 510, 512, 514 and 1024, 1026 (the end of the first and of the second
512-column turn), and ceil(2W / 32) = 2, 3 and 63, 64, 65 (the neighbour bitmap's first turn partly filled, full, and a second
turn of a single word)."""
import numpy as np
import pytest

from edge_based_visual_odometry_amd import synth
from edge_based_visual_odometry_amd.api import Context
from tests import oracle as orc
from tests.util import assert_edges_equal

pytestmark = pytest.mark.gpu

HEIGHTS = [32, 33]
WIDTHS = [35, 34, 265, 266, 267, 522, 523, 32, 33, 1008, 1024, 1025]


def _images(h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return {
        "s2": synth.s2_image(h, w, 11, 4, 2),
        "blank": np.full((h, w), 93, np.uint8),                               # no candidate: every list empty
        "vstep": np.where(xx < w // 2 + 1, 40, 200).astype(np.uint8),         # runs of set bits in ONE word, one column parity
        "hstep": np.where(yy < h // 2, 40, 200).astype(np.uint8),             # whole rows of set bits, one row parity
    }


_REF = {}


def _ref(name, img):
    key = (name,) + img.shape
    if key not in _REF:
        _REF[key] = orc.toed(img, math_mode=orc.PORTABLE)
    return _REF[key]


@pytest.mark.parametrize("w", WIDTHS)
def test_hybrid_edges_at_lane_and_turn_boundaries(w):
    for h in HEIGHTS:
        imgs = _images(h, w)
        with Context(h, w, toed_mode="hybrid") as c:
            for name, img in imgs.items():
                ref = _ref(name, img)
                got = c.toed(img)
                st = c.toed_stats()["left"]
                print(f"h={h} w={w} {name}: kept={len(got.edges)} total={got.n_total} stats={st} fallbacks={c.toed_fallbacks}")
                assert got.n_total == ref["n_total"], (h, w, name)
                assert_edges_equal(got.edges, ref["edges"], f"{h}x{w} {name}")
                if name == "blank":
                    assert st["n_candidates"] == 0 and st["n_neighbour_points"] == 0 and len(got.edges) == 0
                else:
                    assert len(got.edges) > 0 and st["n_candidates"] >= got.n_total
            assert c.toed_fallbacks == 0  # all of the above went through the lists, not through the strict path
            # a batch of two: the images of a launch have their own rows, counters and lists
            for a, b in (("s2", "vstep"), ("hstep", "blank")):
                ea, eb, nt = c.toed_pair(imgs[a], imgs[b])
                assert_edges_equal(ea, _ref(a, imgs[a])["edges"], f"{h}x{w} pair {a}")
                assert_edges_equal(eb, _ref(b, imgs[b])["edges"], f"{h}x{w} pair {b}")
                assert nt == (_ref(a, imgs[a])["n_total"], _ref(b, imgs[b])["n_total"])
            assert c.toed_fallbacks == 0


# The overflow needs more flagged grid points than max_h * max_w, out of the (2h - 20)(2w - 20) interior ones.  At the widths
# 32 .. 35 the interior is too small a share of the grid for any checkerboard to get there: squares of 4, 6 and 8 pixels, in
# two alignments, at heights 32 .. 97 flag at most 0.78 of the capacity (measured).  So the overflow runs at the other eight widths -- 267 and 266 have the lane residues of 35 and 34 (2W - 20 = 2
# and 0 mod 8), 1008 leaves the bitmap's first turn partly filled as 32 and 33 do -- and at heights 64 and 65, the smallest pair
# of both parities at which squares of 4 pixels overflow at every one of them (at 48 and 49 they do not).
OVERFLOW_WIDTHS = [w for w in WIDTHS if w > 35]
OVERFLOW_HEIGHTS = [64, 65]


@pytest.mark.parametrize("w", OVERFLOW_WIDTHS)
def test_hybrid_overflowing_checkerboard_publishes_empty_lists(w):
    """A fine checkerboard is an image of ties: the screen flags more grid points than the candidate arrays hold (cap =
    max_h * max_w).  The lists must be published empty and counts[4] must keep the real total: the library reads both from
    the device, repeats the image on the strict path when counts[4] exceeds the capacity (toed_fallbacks counts that), and
    the edges are then the oracle's.  A list published with a length, or a total cut to the capacity, would leave the
    fallback out and edges missing."""
    for h in OVERFLOW_HEIGHTS:
        yy, xx = np.mgrid[0:h, 0:w]
        img = (((xx // 4 + yy // 4) % 2) * 200 + 20).astype(np.uint8)
        other = synth.s2_image(h, w, 11, 4, 2)
        ref = _ref("checker4", img)
        with Context(h, w, toed_mode="hybrid") as c:
            got = c.toed(img, cap=2 * h * w)
            print(f"h={h} w={w} checker4: kept={len(got.edges)} total={got.n_total} fallbacks={c.toed_fallbacks}")
            assert c.toed_fallbacks == 1, (h, w)
            assert got.n_total == ref["n_total"]
            assert_edges_equal(got.edges, ref["edges"], f"{h}x{w} checker4")
            ea, eb, nt = c.toed_pair(img, other)  # one image of the batch overflows, the other does not
            assert_edges_equal(ea, ref["edges"], f"{h}x{w} pair checker4")
            assert_edges_equal(eb, _ref("s2", other)["edges"], f"{h}x{w} pair s2")
            assert c.toed_fallbacks >= 2
