"""The identity behind the scaled tap tables of the exact TOED stage, stated in numpy, no device.

A pixel byte v in the low word of a zero register pair is the fp64 subnormal d = v * 2^-1074.  With the column taps
scaled by 2^K1 and the row taps by 2^K2, K1 + K2 = 1074, the term (d * ck') * rk' must be the bit pattern of
(v * ck) * rk for every byte and every pair of entries of the two committed tap tables -- in either role, since a table
serves as column taps in one phase and as row taps in another."""
import os
import re

import numpy as np

SRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "edge_based_visual_odometry_amd", "csrc",
                   "toed_kernels.hip")


def _source():
    with open(SRC) as f:
        return f.read()


def _taps():
    text = _source()
    out = []
    for name in ("h_TAP_INT", "h_TAP_HALF"):
        m = re.search(r"const double %s\[4\]\[19\] = \{(.*?)\};" % name, text, re.S)
        rows = re.findall(r"\{(.*?)\}", m.group(1), re.S)
        t = np.array([[float(x) for x in r.replace("\n", " ").split(",") if x.strip()] for r in rows])
        assert t.shape == (4, 19), name
        out.append(t)
    return np.concatenate([t.ravel() for t in out])


def _split():
    text = _source()
    m = re.search(r"constexpr int TAP_K1 = (\d+), TAP_K2 = (\d+);", text)
    return int(m.group(1)), int(m.group(2))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_scaled_taps_give_the_reference_terms_bit_for_bit():
    taps = _taps()
    assert taps.size == 152
    k1, k2 = _split()
    assert k1 + k2 == 1074
    v = np.arange(256, dtype=np.float64)
    d = np.arange(256, dtype=np.uint64).view(np.float64)  # the byte as a subnormal
    assert (d[1:] == np.ldexp(v[1:], -1074)).all() and _bits(d)[0] == 0
    ck, rk = np.ldexp(taps, k1), np.ldexp(taps, k2)
    # every scaled tap is finite, and scaling back is exact (a power of two only moved the exponent)
    assert np.isfinite(ck).all() and np.isfinite(rk).all()
    assert (_bits(np.ldexp(ck, -k1)) == _bits(taps)).all() and (_bits(np.ldexp(rk, -k2)) == _bits(taps)).all()

    col_ref = v[:, None] * taps[None, :]  # fl(v * ck)                     [256, 152]
    col_new = d[:, None] * ck[None, :]    # fl(v 2^-1074 * ck 2^K1)
    # the exact rescale of the column product is fl(v * ck), signed zeros included
    assert (_bits(np.ldexp(col_new, k2)) == _bits(col_ref)).all()
    # every non-zero column product is a normal number
    nz = col_new != 0.0
    assert (nz == (col_ref != 0.0)).all()
    assert np.abs(col_new[nz]).min() >= 2.0 ** -1022

    n = 0
    for j in range(taps.size):  # row tap j against every (byte, column tap): 256 * 152 terms a turn
        ref = col_ref * taps[j]
        new = col_new * rk[j]
        assert (_bits(new) == _bits(ref)).all(), j
        n += ref.size
    assert n == 256 * 152 * 152
