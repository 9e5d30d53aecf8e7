"""Scenes shared by the pose tests (tests/test_gpu_pose.py) and tools/gpu_pose_time.py: the synthetic rigs, the known
motion, and the resident temporal chain of the half-size EuRoC frames."""
import numpy as np

from edge_based_visual_odometry_amd import synth
from tests import oracle_pose as op

R_GT, T_GT = op.rot((0.3, 1.0, -0.2), 0.04), np.array([0.12, -0.03, 0.6])


def rig(name):
    """(K_left, K_right := K_left, R21, T21) of a dataset's calibration"""
    c = synth.CALIB[name]
    K = op._kmat(c["K"])
    return K, K, np.asarray(c["R21"], dtype=np.float64), np.asarray(c["T21"], dtype=np.float64)


def euroc_calib():
    ce = synth.CALIB["euroc"]
    K = tuple(v / 2 for v in ce["K"])
    Kr = tuple(v / 2 for v in ce["K_right"])
    return ([K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1], [Kr[0], 0, Kr[2], 0, Kr[1], Kr[3], 0, 0, 1], ce["R21"], ce["T21"]), K, Kr


def resident_chain(ctx, frame):
    """keyframe 0 and frame `frame` of the EuRoC half-size sequence of tests/test_gpu_temporal.py through the temporal chain
    (stages = 1); returns the calibration, the keyframe mates, the fetched final quads and the counts"""
    h, w = 240, 376
    calib, K, Kr = euroc_calib()
    ce = synth.CALIB["euroc"]
    F = synth.fundamental_21(K, Kr, ce["R21"], ce["T21"])

    def run(k):
        l, r = synth.stereo_pair("s2", h, w, scene=7, noise_base=2 * k, disparity=9)
        ctx.stereo_upload(np.roll(l, k, axis=1), np.roll(r, k, axis=1))
        c = ctx.stereo_run(ctx.default_params(F))
        left = ctx.stereo_fetch(c)["left"]
        _, fin = ctx.stereo_finalize(calib)
        return left, fin

    left0, kf = run(0)
    ctx.temporal_set_keyframe()
    run(frame)
    counts, q = ctx.temporal_match(stages=1)
    return calib, left0[kf["left_index"]], kf["right"], q["final"], counts
