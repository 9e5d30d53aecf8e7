"""csrc/ebvo_math.h (the atan2 / sincos / exp both the oracle's portable mode and the HIP kernels use)
against glibc: identical except where glibc itself is not correctly rounded (<= 1 ulp, rare)."""
import numpy as np

from tests import oracle as orc


def test_atan2_agrees_with_libm():
    rng = np.random.default_rng(0)
    n = 400_000
    ang = rng.uniform(-np.pi, np.pi, n)
    y, x = np.sin(ang), np.cos(ang)
    a, b = orc.atan2_v(y, x, orc.PORTABLE), orc.atan2_v(y, x, orc.LIBM)
    diff = a != b
    assert diff.mean() < 2e-3
    assert (np.abs(a - b)[diff] <= np.spacing(np.abs(b[diff]))).all()


def test_atan2_special_values():
    sp = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, 1e-300, -1e-300, 0.5, 3.0])
    Y, X = [v.ravel().copy() for v in np.meshgrid(sp, sp)]
    a, b = orc.atan2_v(Y, X, orc.PORTABLE), orc.atan2_v(Y, X, orc.LIBM)
    assert (a == b).all()
    assert (np.signbit(a) == np.signbit(b)).all()
    assert np.isnan(orc.atan2_v(np.array([np.nan, 1.0]), np.array([1.0, np.nan]), orc.PORTABLE)).all()


def test_sincos_agrees_with_libm():
    rng = np.random.default_rng(1)
    t = np.concatenate([rng.uniform(-np.pi, np.pi, 300_000), rng.uniform(-50, 50, 100_000),
                        np.array([0.0, np.pi / 2, -np.pi / 2, np.pi, -np.pi, np.pi / 4, 1e-9, -1e-9])])
    s, c = orc.sincos_v(t, orc.PORTABLE)
    sm, cm = orc.sincos_v(t, orc.LIBM)
    for a, b in ((s, sm), (c, cm)):
        diff = a != b
        assert diff.mean() < 4e-3
        assert (np.abs(a - b)[diff] <= np.spacing(np.abs(b[diff]))).all()


def test_exp_agrees_with_libm_and_mpmath():
    import mpmath as mp
    rng = np.random.default_rng(2)
    x = np.concatenate([-rng.uniform(0, 90, 200_000), rng.uniform(-2, 2, 100_000), -rng.exponential(1e-3, 50_000),
                        np.array([0.0, -0.0, -1e-300, -745.0, -746.0, 709.0, 710.0, -np.inf, np.inf, 1e-17, -0.5])])
    a, b = orc.exp_v(x, orc.PORTABLE), orc.exp_v(x, orc.LIBM)
    diff = a != b
    assert diff.mean() < 2e-3
    assert (np.abs(a - b)[diff] <= np.spacing(np.abs(b[diff]))).all()
    assert np.isnan(orc.exp_v(np.array([np.nan]), orc.PORTABLE)).all()
    # where the two disagree the shared routine is the correctly rounded one
    mp.mp.prec = 200
    for xv, av, bv in list(zip(x[diff], a[diff], b[diff]))[:200]:
        exact = mp.exp(mp.mpf(float(xv)))
        assert abs(mp.mpf(float(av)) - exact) <= abs(mp.mpf(float(bv)) - exact)


def _is_nearest(mp, value, exact):
    """`value` (a double) is the double closest to the arbitrary-precision `exact`"""
    d = abs(mp.mpf(float(value)) - exact)
    lo, hi = np.nextafter(value, -np.inf), np.nextafter(value, np.inf)
    return d <= abs(mp.mpf(float(lo)) - exact) and d <= abs(mp.mpf(float(hi)) - exact)


def test_atan2_sincos_are_correctly_rounded_against_mpmath():
    """An anchor that does not go through csrc/ebvo_math.h: the oracle's portable mode and the kernels share that header,
    so their agreement on theta / sin / cos says nothing about the routine itself.  Here every result is compared with the
    200-bit value of mpmath: the shared routine returns the nearest double on all sampled inputs, including every input
    on which glibc returns the other neighbour."""
    import mpmath as mp
    mp.mp.prec = 200
    rng = np.random.default_rng(3)
    # atan2 as the detector calls it: a unit vector (cpu_toed.cpp:226-229), plus general magnitudes
    ang = rng.uniform(-np.pi, np.pi, 6000)
    y = np.concatenate([np.sin(ang), rng.normal(0, 50, 2000), np.array([1e-8, -1e-8, 1.0, -1.0, 3.0])])
    x = np.concatenate([np.cos(ang), rng.normal(0, 50, 2000), np.array([1.0, -1.0, 1e-8, -1e-8, -4.0])])
    a, b = orc.atan2_v(y, x, orc.PORTABLE), orc.atan2_v(y, x, orc.LIBM)
    for yv, xv, av in zip(y, x, a):
        assert _is_nearest(mp, av, mp.atan2(mp.mpf(float(yv)), mp.mpf(float(xv)))), (yv, xv, av)
    # the inputs on which glibc disagrees, from a larger sample: the shared routine is the nearest one there too
    ang = rng.uniform(-np.pi, np.pi, 300_000)
    y, x = np.sin(ang), np.cos(ang)
    a, b = orc.atan2_v(y, x, orc.PORTABLE), orc.atan2_v(y, x, orc.LIBM)
    dis = np.flatnonzero(a != b)
    assert len(dis) > 20
    for k in dis[:300]:
        assert _is_nearest(mp, a[k], mp.atan2(mp.mpf(float(y[k])), mp.mpf(float(x[k]))))
    # sin / cos on the orientation range and beyond
    t = np.concatenate([rng.uniform(-np.pi, np.pi, 6000), rng.uniform(-50, 50, 1500), np.array([1e-9, -1e-9, np.pi / 2, np.pi])])
    s, c = orc.sincos_v(t, orc.PORTABLE)
    for tv, sv, cv in zip(t, s, c):
        m = mp.mpf(float(tv))
        assert _is_nearest(mp, sv, mp.sin(m)) and _is_nearest(mp, cv, mp.cos(m)), tv
    t = rng.uniform(-np.pi, np.pi, 300_000)
    s, c = orc.sincos_v(t, orc.PORTABLE)
    sm, cm = orc.sincos_v(t, orc.LIBM)
    for k in np.flatnonzero(s != sm)[:200]:
        assert _is_nearest(mp, s[k], mp.sin(mp.mpf(float(t[k]))))
    for k in np.flatnonzero(c != cm)[:200]:
        assert _is_nearest(mp, c[k], mp.cos(mp.mpf(float(t[k]))))


# ---- the two single-precision routines of the SIFT descriptor ------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_floats(a, b):
    """bit-equal, any NaN equal to any NaN"""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return bool(((_bits(a) == _bits(b)) | (np.isnan(a) & np.isnan(b))).all())


EXPF_MAX_ULP = 2.73        # measured below: the largest error on [-2, 0] (the header's "about 1 ulp" was an estimate)


def test_expf_equals_its_float32_restatement_on_every_float_of_the_weight_range():
    """ebvo_expf against tests/sift_reading.py: expf (numpy float32, written from the formula) on EVERY float of
    [-2, -2^-6] -- the descriptor's Gaussian weights use (-1.5625, 0] -- and on the special values and both cutoffs."""
    from tests import sift_reading as sr
    lo, hi = int(np.float32(2.0 ** -6).view(np.uint32)), int(np.float32(2.0).view(np.uint32))
    for a in range(lo, hi + 1, 1 << 22):
        x = -np.arange(a, min(a + (1 << 22), hi + 1), dtype=np.uint32).view(np.float32)
        assert (_bits(orc.expf_v(x)) == _bits(sr.expf(x))).all(), hex(a)
    near = lambda v: [np.nextafter(np.nextafter(np.float32(v), np.float32(-np.inf)), np.float32(-np.inf)),
                      np.nextafter(np.float32(v), np.float32(-np.inf)), np.float32(v),
                      np.nextafter(np.float32(v), np.float32(np.inf)),
                      np.nextafter(np.nextafter(np.float32(v), np.float32(np.inf)), np.float32(np.inf))]
    sp = np.array([0.0, -0.0, np.nan, np.inf, -np.inf, -1e-30, 1e-30, -2.0 ** -7, -1.5625, 1.0, 20.0] + near(-87.0) + near(88.0),
                  dtype=np.float32)
    got = orc.expf_v(sp)
    assert _same_floats(got, sr.expf(sp))
    assert got[0] == 1 and got[1] == 1 and np.isnan(got[2]) and got[3] == np.inf and got[4] == 0
    below, above = got[11:16], got[16:21]                      # around -87 and around 88
    assert (below[:2] == 0).all() and (below[2:] > 0).all()    # x < -87 -> 0; -87 itself is still evaluated
    assert np.isfinite(above[:3]).all() and (above[3:] == np.inf).all()


def test_expf_error_against_mpmath():
    """The measured accuracy of ebvo_expf on the weight range: 10^5 random inputs of [-2, 0] against mpmath, in units of the
    last place of the correctly rounded float.  Measured maximum 2.73 ulp (csrc/ebvo_math.h); the
    assertion leaves a quarter on top of the measurement, as a guard against a change of the routine."""
    import mpmath as mp
    mp.mp.prec = 100
    x = np.random.default_rng(7).uniform(-2, 0, 100_000).astype(np.float32)
    got = orc.expf_v(x)
    worst = 0.0
    for xv, g in zip(x, got):
        exact = mp.exp(mp.mpf(float(xv)))
        ulp = float(np.spacing(np.float32(float(exact))))
        worst = max(worst, float(abs(mp.mpf(float(g)) - exact) / ulp))
    print("ebvo_expf max error on [-2, 0]: %.4f ulp" % worst)
    assert 1.0 < worst <= EXPF_MAX_ULP * 1.25


def test_fast_atan2_equals_its_float32_restatement():
    from tests import sift_reading as sr
    rng = np.random.default_rng(8)
    n = 1_000_000
    y = np.concatenate([rng.normal(0, 40, n // 2), rng.uniform(-1, 1, n // 2) * 10.0 ** rng.integers(-30, 30, n // 2)])
    x = np.concatenate([rng.normal(0, 40, n // 2), rng.uniform(-1, 1, n // 2) * 10.0 ** rng.integers(-30, 30, n // 2)])
    y, x = y.astype(np.float32), x.astype(np.float32)
    assert (_bits(orc.fast_atan2_deg_v(y, x)) == _bits(sr.fast_atan2_deg(y, x))).all()
    # axes, the origin, signed zeros, the diagonals, tiny values
    v = np.array([0.0, -0.0, 1.0, -1.0, 3.5, -3.5, 1e-30, -1e-30, 1e-45, -1e-45, 255.0, -255.0, 1e30, -1e30], dtype=np.float32)
    Y, X = [g.ravel().copy() for g in np.meshgrid(v, v)]
    got = orc.fast_atan2_deg_v(Y, X)
    assert (_bits(got) == _bits(sr.fast_atan2_deg(Y, X))).all()
    at = lambda yy, xx: float(orc.fast_atan2_deg_v([yy], [xx])[0])
    assert (at(0, 0), at(-0.0, 0), at(0, 1), at(0, -1), at(1, 0), at(-1, 0)) == (0, 0, 0, 180, 90, 270)
    assert (at(-0.0, 1), at(-0.0, -1)) == (0, 180)            # y < 0 is false for -0.0: no reflection
    # |y| == |x|: the polynomial at c = 1 (up to the 2.2e-16 added to the denominator, which a float does not see)
    d45, f = np.float32(at(1, 1)), np.float32
    assert abs(d45 - 45) < 0.01
    assert (at(1, -1), at(-1, -1), at(-1, 1)) == (f(180) - d45, f(360) - (f(180) - d45), f(360) - d45)
    # a tiny negative y: 360 - (something below half an ulp of 360) rounds to 360 itself, NOT a value in [0, 360)
    assert at(-1e-30, 1) == 360.0 and at(-1e-45, 1) == 360.0 and at(-1e-7, 1) == 360.0 and at(-1e-6, 1) < 360.0


def test_fast_atan2_within_the_published_bound_of_mpmath():
    """OpenCV documents fastAtan2 as accurate to about 0.3 degrees"""
    import mpmath as mp
    mp.mp.prec = 100
    rng = np.random.default_rng(9)
    ang = rng.uniform(-np.pi, np.pi, 20_000)
    mag = 10.0 ** rng.uniform(-3, 3, 20_000)
    y = np.concatenate([np.sin(ang) * mag, [1, -1, 1, -1, 0, 0, 1, -1, -1e-30]]).astype(np.float32)
    x = np.concatenate([np.cos(ang) * mag, [1, 1, -1, -1, 1, -1, 0, 0, 1]]).astype(np.float32)
    got = orc.fast_atan2_deg_v(y, x)
    worst = 0.0
    for yv, xv, g in zip(y, x, got):
        exact = mp.degrees(mp.atan2(mp.mpf(float(yv)), mp.mpf(float(xv)))) % 360
        err = abs(mp.mpf(float(g)) - exact)
        worst = max(worst, float(min(err, 360 - err)))
    print("ebvo_fast_atan2_deg max error: %.4f degrees" % worst)
    assert worst <= 0.3
