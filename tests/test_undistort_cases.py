"""tests/undistort_reading.py (a second, direct reading of OpenCV's cv::undistort) agrees with the C restatement byte for
byte on every case of tests/undistort_cases.py, and every case still meets the condition it was chosen for: sampling over
each border, the (short) wrap, the saturated rounding, stripes of one, two and three rows.  CPU only."""
import numpy as np
import pytest

from edge_based_visual_odometry_amd import synth
from tests import oracle as orc
from tests import undistort_cases as uc
from tests import undistort_reading as ur


@pytest.mark.parametrize("name", list(uc.CASES))
def test_reading_equals_oracle_and_case_meets_its_condition(name):
    _, K, dist = uc.CASES[name]
    got, counts = uc.reading(name)
    ref = orc.undistort(uc.image(name), K, dist)
    assert (got == ref).all(), f"{int((got != ref).sum())} pixels differ"
    h, w = got.shape
    # the classes partition the image: all taps / some taps / no tap inside
    some = sum(counts[s] for s in uc.SIDES)
    assert counts["inside"] + counts["none"] <= h * w <= counts["inside"] + counts["none"] + some
    print(name, {k: v for k, v in counts.items() if k not in ("row_y", "stripes", "none_mask")})
    assert uc.condition(name), counts


def test_suite_images_never_left_the_image_before():
    """What this case list is for: the EuRoC model of tests/test_gpu_undistort.py samples strictly inside"""
    ce = synth.CALIB["euroc"]
    h, w = 97, 131
    K = (ce["K"][0] * w / 752, ce["K"][1] * h / 480, ce["K"][2] * w / 752, ce["K"][3] * h / 480)
    _, c = ur.undistort(synth.s2_image(h, w, noise_seed=3), K, ce["dist"])
    assert c["inside"] == h * w and c["wrapped"] == c["saturated"] == 0


def test_reading_on_a_strided_image_and_zero_distortion():
    img = uc.image("pincushion")
    assert (ur.undistort(img, uc.K_PIN, (0, 0, 0, 0))[0] == img).all()
    wide = np.zeros((img.shape[0], img.shape[1] + 13), dtype=np.uint8)
    wide[:, :img.shape[1]] = img
    _, K, dist = uc.CASES["pincushion"]
    assert (orc.undistort(wide[:, :img.shape[1]], K, dist) == uc.reading("pincushion")[0]).all()


def test_rounding_wrap_and_saturation_primitives():
    v = np.array([0.5, 1.5, 2.5, -0.5, -1.5, 2147483646.5, 2147483647.0, 1e300, -2147483648.0, -2147483649.0, -1e300,
                  np.nan, np.inf, -np.inf])
    r, sat = ur.cv_round_sat(v)
    assert r.tolist() == [0, 2, 2, 0, -2, 2147483646, ur.INT_MAX, ur.INT_MAX, ur.INT_MIN, ur.INT_MIN, ur.INT_MIN,
                          ur.INT_MIN, ur.INT_MAX, ur.INT_MIN]
    assert sat.tolist() == [False] * 6 + [True] * 8
    q = np.array([0, -1, 32767, 32768, 65535, 65536, -32768, -32769, ur.INT_MAX >> 5, ur.INT_MIN >> 5], dtype=np.int64)
    assert ur.to_short(q).tolist() == [0, -1, 32767, -32768, -1, 0, -32768, 32767, -1, 0]
    assert (np.array([-1, -33], dtype=np.int64) >> 5).tolist() == [-1, -2] and (np.array([-1]) & 31).tolist() == [31]
