"""Noisy synthetic quads for the refit tests (tests/test_pose_refit_oracle.py, tests/test_gpu_pose_refit.py): the quads of
tests/oracle_pose.py::synthetic_quads under the known motion of tests/pose_scenes.py, with sub-pixel noise on every edge
location."""
import numpy as np

from tests import oracle_pose as op
from tests import pose_scenes as ps

RIGS = ("kitti", "euroc")
# (quads, outlier fraction, sigma in px) of the 40 noisy scenes: each on both rigs with seeds 0..3
NOISY = ((64, 0.3, 0.3), (300, 0.3, 0.3), (300, 0.5, 0.2), (1000, 0.3, 0.3), (64, 0.3, 0.1))
SEEDS = (0, 1, 2, 3)
SEARCH = dict(max_iterations=600, min_iterations=100)   # the search that supplies the start pose


def calib(rig_name):
    """(K_left, K_right := K_left, R21, T21)"""
    return ps.rig(rig_name)


def noisy_quads(rig_name, n, frac, sigma, seed):
    """(kf_left, kf_right, row_ptr, cf_left, cf_right, planted inlier mask): independent N(0, sigma) on x and y of the four
    edge arrays, in that order, x then y per array, from default_rng(1000 + seed)"""
    K, _, R21, T21 = ps.rig(rig_name)
    kfL, kfR, rp, cfL, cfR, inl = op.synthetic_quads(n, frac, (K, R21, T21), ps.R_GT, ps.T_GT, seed=seed)
    if sigma > 0:
        rng = np.random.default_rng(1000 + seed)
        for e in (kfL, kfR, cfL, cfR):
            e["x"] += rng.normal(0.0, sigma, len(e))
            e["y"] += rng.normal(0.0, sigma, len(e))
    return kfL, kfR, rp, cfL, cfR, inl
