"""Scenes for the handover of the depths on promotion (tests/test_carry_oracle.py, tests/carry_cases.py): the multi-frame
curve scenes of tests/depth_scenes.py (imported, not edited) whose LAST later frame also gets MATES -- the same curves sampled
at yet other parameters, moved by that frame's planted pose, projected into both of its cameras, with N(0, sigma_disp) px of
disparity noise of its own on the right mate's x.  lambda_true' (the new mate's triangulated depth over its true one) is
therefore known.

tests/depth_scenes.py::scene does not return its curves, so they are recorded while it runs (every curve it draws comes
from tests/align_scenes.py::_curve) and the ones it kept are recognised by their keyframe samples."""
import numpy as np

from tests import align_scenes as asc
from tests import depth_scenes as ds
from tests import oracle as orc

W, H = ds.W, ds.H
FIXED_POINT, NOISY, SIGMA_DISP, FRAMES = ds.FIXED_POINT, ds.NOISY, ds.SIGMA_DISP, ds.FRAMES

# Fixed point (tests/test_carry_oracle.py::test_fixed_point): the largest |lambda' - 1| over the carried mates that the oracle
# shows on the noise-free scenes (frames 1 .. 4 fused at the planted poses, then carried to frame 4 with the defaults).
# Measured with tests/oracle_carry.py; the test asserts 10 x this.  As in the filter's study it is sampling geometry, not
# rounding: the fused lambda carries the arcs' sagitta, and the new mate sits up to `radius` along the curve from the old
# projection it takes its depth from, at another depth on a slanted curve.
FIXED_POINT_MEASURED = 0.022254138906994236   # euroc seed 1; kitti 0: 0.0090, kitti 1: 0.0125, euroc 0: 0.0102

# Carried share (test_recovery): carried mates over live new mates per noisy scene, in the order of NOISY, as the oracle
# shows it with the defaults; the test asserts at least half of each.
CARRIED_SHARE_MEASURED = (0.9385, 0.9670, 0.9664, 0.9305, 0.9719, 0.9712, 0.9535, 0.9632, 0.9651, 0.9529, 0.9490, 0.9490)


def scene(rig_name, seed, kind="mixed", sigma=0.0, clutter=0, sigma_disp=0.0, kf_px=1.0):
    """tests/depth_scenes.py::scene plus new_left / new_right (the mates of the last frame, the right ones with their own
    disparity noise), new_right_true and new_lambda_true"""
    drawn = []
    real = asc._curve

    def recording(rng, k, K):
        c = real(rng, k, K)
        drawn.append(c)
        return c
    asc._curve = recording
    try:
        sc = ds.scene(rig_name, seed, kind, sigma, clutter, sigma_disp=sigma_disp, kf_px=kf_px)
    finally:
        asc._curve = real
    K, Kr, R21, T21 = sc["calib"]
    Rg, tg = sc["poses"][-1]
    rng = np.random.default_rng(77100 + 131 * seed + (0 if rig_name == "kitti" else 17))
    at, nl, nr = 0, [], []
    for f, L, step in drawn:
        # the curve's keyframe samples as the scene formed them: kept iff they are the next block of its mates
        Xk, Dk = f(np.arange(0.0, L, kf_px * step))
        eL, okL = asc._see(K, Xk, Dk)
        eR, okR = asc._see(Kr, Xk @ R21.T + T21, Dk @ R21.T)
        fin = orc.finalize_pairs(K, Kr, R21, T21, eL, eR)
        good = okL & okR & (np.abs(fin[:, 6:9] - Xk).max(axis=1) < 1e-6) & (np.abs(np.einsum("ij,ij->i", fin[:, 9:12], Dk)) > 0.999)
        n = int(good.sum())
        blk = sc["kf_left"][at:at + n]
        if n < 20 or len(blk) != n or not (np.array_equal(blk["x"], eL["x"][good]) and np.array_equal(blk["y"], eL["y"][good])):
            continue
        at += n
        Xs, Ds = f(np.arange(0.71 * kf_px * step, L, kf_px * step))
        Xc, Dc = Xs @ Rg.T + tg, Ds @ Rg.T
        cL, vL = asc._see(K, Xc, Dc)
        cR, vR = asc._see(Kr, Xc @ R21.T + T21, Dc @ R21.T)
        fin = orc.finalize_pairs(K, Kr, R21, T21, cL, cR)
        ok = vL & vR & (np.abs(fin[:, 6:9] - Xc).max(axis=1) < 1e-6) & (np.abs(np.einsum("ij,ij->i", fin[:, 9:12], Dc)) > 0.999)
        nl.append(cL[ok])
        nr.append(cR[ok])
    assert at == len(sc["kf_left"]), "a kept curve was not recognised"
    new_left, new_true = np.concatenate(nl), np.concatenate(nr)
    new_left["index"] = new_true["index"] = np.arange(len(new_left))
    new_right = new_true.copy()
    if sigma_disp > 0:
        new_right["x"] += rng.normal(0.0, sigma_disp, len(new_right))
    with np.errstate(all="ignore"):
        z_noisy = orc.finalize_pairs(K, Kr, R21, T21, new_left, new_right)[:, 8]
        z_true = orc.finalize_pairs(K, Kr, R21, T21, new_left, new_true)[:, 8]
    return dict(sc, new_left=new_left, new_right=new_right, new_right_true=new_true, new_lambda_true=z_noisy / z_true)


def carried(sc, frames=None, **params):
    """the filter over the scene's frames at the planted poses (tests/depth_scenes.py::fuse), then the handover to the last
    frame under its planted pose: (the fused state, the oracle's result)"""
    from tests import oracle_carry as oc
    lam, info, nobs, _ = ds.fuse(sc, frames)[-1]
    R, t = sc["poses"][-1]
    return (lam, info, nobs), oc.carry(sc["kf_left"], sc["kf_right"], sc["new_left"], sc["new_right"], W, H, sc["calib"], R, t,
                                       state=(lam, info, nobs), **params)
