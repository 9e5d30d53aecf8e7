"""The sample coordinates of a patch row (sample_row in csrc/match_kernels.hip, fast path), in numpy.

The reference writes, for row i and column j of the 7 x 7 grid (src/utility.cpp:141-161),
    x = cs * i - sn * j + cx,      y = sn * i + cs * j + cy                                  (form A)
The kernel forms cs * i and sn * i once per row and the products P_m = sn * m, Q_m = cs * m (m = 1, 2, 3) once:
    j > 0: x = (cs * i - P_j) + cx,   y = (sn * i + Q_j) + cy
    j < 0: x = (cs * i + P_|j|) + cx, y = (sn * i - Q_|j|) + cy
    j = 0: x = cs * i + cx,           y = sn * i + cy                                          (form B)
Form B must give the bits of form A: sn * (-m) = -(sn * m), a - (-b) = a + b, and at j = 0 a signed zero (the product,
and possibly the whole first term) vanishes in the last addition because cx, cy are not zero -- on the fast path every
edge lies at least 9.3 px inside the image, so cx, cy >= 4.3.  numpy evaluates both forms operation by operation in
IEEE double (no contraction), as the device build does (-ffp-contract=off)."""
import numpy as np

N_ORIENT = 100_000
TINY = np.float64(5e-324)            # smallest subnormal
SUB = np.float64(2.2250738585072014e-308) / 8


def _orientations():
    """(sn, cs) of 10^5 orientations: the axis directions as the library's sincos may return them (exact zeros of either
    sign, or numpy's nearly-zero values), sines / cosines that are subnormal, and random angles"""
    rng = np.random.default_rng(20260921)
    special_theta = np.array([0.0, -0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, np.pi / 4, -3 * np.pi / 4, 1e-310, -1e-310, 1e-160])
    sn, cs = [np.sin(special_theta)], [np.cos(special_theta)]
    z = [0.0, -0.0, TINY, -TINY, SUB, -SUB]
    for a in z:                                  # sine (cosine) a zero or a subnormal of either sign, the other +-1
        for b in (1.0, -1.0):
            sn.append(np.array([a, b]))
            cs.append(np.array([b, a]))
    sn, cs = np.concatenate(sn), np.concatenate(cs)
    theta = rng.uniform(-np.pi, np.pi, N_ORIENT - len(sn))
    return np.concatenate([sn, np.sin(theta)]), np.concatenate([cs, np.cos(theta)])


def _positions(n):
    """edge positions from 9.3 (the fast path's lower limit, patch_inside) upward: the limit itself, its neighbourhood, a
    frame's width"""
    rng = np.random.default_rng(7)
    ex = rng.uniform(9.3, 1300.0, n)
    ey = rng.uniform(9.3, 500.0, n)
    ex[:4000] = rng.uniform(9.3, 10.5, 4000)
    ey[2000:6000] = rng.uniform(9.3, 10.5, 4000)
    ex[::97] = 9.3
    ey[::89] = 9.3
    ex[5::101] = np.floor(ex[5::101]) + 10.0      # whole-pixel positions (integer sample coordinates on axis directions)
    ey[7::103] = np.floor(ey[7::103]) + 10.0
    return ex, ey


def _centres(ex, ey, sn, cs, side):
    # sample_row: cx = side ? ex + 5 * (-sn) : ex + 5 * sn,  cy = side ? ey + 5 * cs : ey + 5 * (-cs)
    if side:
        return ex + 5.0 * (-sn), ey + 5.0 * cs
    return ex + 5.0 * sn, ey + 5.0 * (-cs)


def _form_a(sn, cs, cx, cy, i, j):
    fi, fj = np.float64(i), np.float64(j)
    return (cs * fi - sn * fj) + cx, (sn * fi + cs * fj) + cy


def _form_b(sn, cs, cx, cy, i, j, P, Q):
    ci, si = cs * np.float64(i), sn * np.float64(i)
    if j > 0:
        return (ci - P[j]) + cx, (si + Q[j]) + cy
    if j < 0:
        return (ci + P[-j]) + cx, (si - Q[-j]) + cy
    return ci + cx, si + cy


def test_shared_products_give_the_bits_of_the_expression_as_written():
    sn, cs = _orientations()
    assert len(sn) == N_ORIENT
    assert (sn == 0).any() and (cs == 0).any() and np.signbit(sn[sn == 0]).any() and np.signbit(cs[cs == 0]).any()
    assert ((np.abs(sn) < 2.3e-308) & (sn != 0)).any() and ((np.abs(cs) < 2.3e-308) & (cs != 0)).any()
    ex, ey = _positions(N_ORIENT)
    assert ex.min() == 9.3 and ey.min() == 9.3
    P = [None] + [sn * np.float64(m) for m in (1, 2, 3)]
    Q = [None] + [cs * np.float64(m) for m in (1, 2, 3)]
    for side in (0, 1):
        cx, cy = _centres(ex, ey, sn, cs, side)
        assert cx.min() >= 4.3 - 1e-12 and cy.min() >= 4.3 - 1e-12          # the precondition of the j = 0 shortcut
        for i in range(-3, 4):
            for j in range(-3, 4):
                xa, ya = _form_a(sn, cs, cx, cy, i, j)
                xb, yb = _form_b(sn, cs, cx, cy, i, j, P, Q)
                assert np.array_equal(xa.view(np.uint64), xb.view(np.uint64)), (side, i, j, "x")
                assert np.array_equal(ya.view(np.uint64), yb.view(np.uint64)), (side, i, j, "y")


def test_the_shortcut_of_column_zero_needs_a_nonzero_centre():
    """why sample_row_border keeps form A: with cx = 0 the sign of a zero first term survives the last addition"""
    sn, cs, cx, cy = np.float64(1.0), np.float64(-0.0), np.float64(0.0), np.float64(0.0)
    xa, _ = _form_a(sn, cs, cx, cy, 1, 0)                  # (-0 * 1 - 1 * 0) + 0 = (-0 - 0) + 0 = +0
    xb, _ = _form_b(sn, cs, cx, cy, 1, 0, None, None)      # -0 * 1 + 0 = +0 ... and with cx = -0:
    assert xa.view(np.uint64) == xb.view(np.uint64)
    cxn = np.float64(-0.0)
    xa, _ = _form_a(sn, cs, cxn, cy, 1, 0)                 # (-0 - 0) + -0 = -0 + -0 = -0
    xa2, _ = _form_a(sn, -cs, cxn, cy, 1, 0)               # (+0 - 0) + -0 = +0
    xb2, _ = _form_b(sn, -cs, cxn, cy, 1, 0, None, None)   # +0 + -0 = +0
    assert np.signbit(xa) and not np.signbit(xa2) and not np.signbit(xb2)
    sn2 = np.float64(-1.0)                                 # product sn * 0 = -0: (-0 - -0) + -0 = +0 + -0 = +0, form B: -0 + -0 = -0
    xa3, _ = _form_a(sn2, cs, cxn, cy, 1, 0)
    xb3, _ = _form_b(sn2, cs, cxn, cy, 1, 0, None, None)
    assert not np.signbit(xa3) and np.signbit(xb3)
