"""tests/sift_reading.py (a second, numpy-float32 reading of the SIFT base level, calcSIFTDescriptor and the min-of-four
distance) agrees with the C restatement bit for bit on every case of tests/sift_cases.py, and every case still meets the
condition it was chosen for: saturated entries, all-zero descriptors, windows off the image, negative first bins and votes
in front of the histogram.  CPU only."""
import numpy as np
import pytest

from edge_based_visual_odometry_amd import synth
from tests import oracle as orc
from tests import sift_cases as sc
from tests import sift_reading as sr
from tests.util import assert_bit_equal


@pytest.mark.parametrize("name", sc.NAMES)
def test_reading_equals_oracle_and_case_meets_its_condition(name):
    d, counters = sc.reading(name)
    assert_bit_equal(d, sc.oracle_descriptors(name), "descriptors")
    print(name, len(sc.case(name)[1]), counters)
    assert sc.condition(name), counters


@pytest.mark.parametrize("name", sc.NAMES)
def test_base_level_reading_equals_oracle(name):
    img, _ = sc.case(name)
    assert_bit_equal(sr.base_level(img), orc.sift_base(img), "base level")


def test_kernel_reading_is_the_oracles():
    import ctypes as C
    k = np.zeros(13, dtype=np.float32)
    orc.lib().orc_sift_kernel13(k.ctypes.data_as(C.c_void_p))
    assert_bit_equal(sr.kernel13(), k, "13 taps")
    assert abs(float(k.astype(np.float64).sum()) - 1) < 1e-6 and (k == k[::-1]).all()


def test_suite_images_never_saturated_before():
    """What this case list is for: on the generator's textured images no entry comes near 255"""
    img = synth.s2_image(96, 160)
    d, c = sr.descriptors(img, orc.toed(img)["edges"])
    assert c["saturated"] == c["equal_255"] == c["all_zero"] == 0 and d.max() < 255


@pytest.mark.parametrize("n_pairs", [1, 15, 16, 17, 300])
def test_distance_reading_equals_oracle_on_the_integer_lists(n_pairs):
    left, cand, row_ptr, sp = sc.distance_case(n_pairs)
    d = sr.min_distances(left, cand, row_ptr)
    assert_bit_equal(d, orc.sift_min_distances(left, cand, row_ptr), "min distances")
    check_specials(d, left, cand, row_ptr, sp, n_pairs)


def check_specials(d, left, cand, row_ptr, sp, n_pairs):
    """the constructed pairs have the distances they were built for, and the CSR its empty rows"""
    lens = np.diff(row_ptr)
    assert lens[0] == 0 and lens[-1] == 0 and int(row_ptr[-1]) == n_pairs == len(cand)
    if n_pairs >= 2:
        used = np.flatnonzero(lens)
        assert (lens[used[0]:used[-1]] == 0).any()
    assert d[sp["zero_vs_255"]].tolist() == [np.sqrt(128.0 * 255 * 255)]
    assert (d[sp["identical"]] == 0).all()
    row_of = np.repeat(np.arange(len(lens)), lens)
    for t in range(4):
        for k in sp[f"min{t}"]:
            assert d[k] == 1.0
            four = [np.sqrt(((left[row_of[k], q & 1].astype(np.float64) - cand[k, q >> 1]) ** 2).sum()) for q in range(4)]
            assert int(np.argmin(four)) == t and sorted(four)[1] > 1.0
    if n_pairs >= 12:
        assert all(len(sp[f"min{t}"]) == 2 for t in range(4))


def test_distance_reading_on_case_descriptors():
    """real descriptors (saturated and all-zero ones included) against each other: every left edge against the next three"""
    for name in ("step32", "step_odd"):
        d = sc.oracle_descriptors(name)
        n = len(d)
        row_ptr = np.arange(0, 3 * n + 1, 3, dtype=np.int32)
        cand = d[(np.repeat(np.arange(n), 3) + np.tile([0, 1, 5], n)) % n]
        assert_bit_equal(sr.min_distances(d, cand, row_ptr), orc.sift_min_distances(d, cand, row_ptr), name)
