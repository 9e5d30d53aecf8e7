"""What the temporal ground truth costs on the half-scale EuRoC pair of the temporal tests (240 x 376, keyframe 0 against
frame 2, stages = 1): host wall milliseconds per ebvo_temporal_set_gt (projection, veridical count and fill, the rows of
three stages; synchronous) and per ebvo_temporal_gt_metrics, mean of 10, next to ebvo_temporal_match for scale, and the
device time per launch of the three kernels from the library's profiler.  Then the same with the stage trail kept
(ebvo_temporal_keep_stages): the match with the switch on, ebvo_temporal_set_gt over eight stages instead of three, and the
device time of tgt_grid_rows.  The measurement is a child process under its own time limit; a child that fails ends the
run.  Prints one JSON line."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT = 240


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    return round((time.perf_counter() - t0) / reps * 1e3, 3), r


def child():
    import numpy as np

    from edge_based_visual_odometry_amd import synth
    from edge_based_visual_odometry_amd.api import Context

    h, w = 240, 376
    ce = synth.CALIB["euroc"]
    K, Kr = tuple(v / 2 for v in ce["K"]), tuple(v / 2 for v in ce["K_right"])
    F = synth.fundamental_21(K, Kr, ce["R21"], ce["T21"])
    calib = ([K[0], 0, K[2], 0, K[1], K[3], 0, 0, 1], [Kr[0], 0, Kr[2], 0, Kr[1], Kr[3], 0, 0, 1], ce["R21"], ce["T21"])
    R, t = np.eye(3), np.array([1.25 * -ce["T21"][0] / 9.0, 0.0, 0.0])     # tests/tgt_cases.py: resident_pose(1.25)
    out = {}
    with Context(512, 1280, device=0) as ctx:
        def frame(k):
            l, r = synth.stereo_pair("s2", h, w, scene=7, noise_base=2 * k, disparity=9)
            ctx.stereo_upload(np.roll(l, k, axis=1), np.roll(r, k, axis=1))
            ctx.stereo_run(ctx.default_params(F))
            ctx.stereo_finalize(calib)

        frame(0)
        ctx.temporal_set_keyframe()
        frame(2)
        ms_match, (counts, _) = timed(lambda: ctx.temporal_match(stages=1, fetch=False), 10)
        ms_arm, sz = timed(lambda: ctx.temporal_set_gt(R, t, calib), 10)
        ms_metrics, m = timed(ctx.temporal_gt_metrics, 10)
        out.update(temporal_match_ms=ms_match, set_gt_ms=ms_arm, gt_metrics_ms=ms_metrics, n_cf=counts["n_cf"],
                   n_candidates=counts["n_candidates"], n_final=counts["n_final"], **sz)
        out["stages"] = {s["name"]: dict(recall=round(s["recall"], 4), precision=round(s["precision"], 4),
                                         ambiguity=round(s["ambiguity"], 4)) for s in m if s["present"]}
        ctx.profile_reset()
        ctx.profile_enable(True)
        for _ in range(10):
            ctx.temporal_set_gt(R, t, calib)
        ctx.profile_enable(False)
        prof = ctx.profile_get()
        out["kernel_us_per_launch"] = {k: round(prof[k][0] / prof[k][1] * 1e3, 1) for k in
                                       ("tgt_project", "tgt_veridical", "tgt_rows", "gt_misc") if prof[k][1]}
        # the same slot with the stage trail kept: eight stages
        ctx.temporal_keep_stages(True)
        ms_match_on, (counts_on, _) = timed(lambda: ctx.temporal_match(stages=1, fetch=False), 10)
        ms_arm8, _ = timed(lambda: ctx.temporal_set_gt(R, t, calib), 10)
        ms_metrics8, m8 = timed(ctx.temporal_gt_metrics, 10)
        assert counts_on == counts and sum(s["present"] for s in m8) == 8
        out.update(temporal_match_trail_ms=ms_match_on, set_gt_8_ms=ms_arm8, gt_metrics_8_ms=ms_metrics8)
        out["stages_8"] = {s["name"]: dict(sum_n=s["sum_n"], sum_tp=s["sum_tp"], recall=round(s["recall"], 4)) for s in m8}
        ctx.profile_reset()
        ctx.profile_enable(True)
        for _ in range(10):
            ctx.temporal_set_gt(R, t, calib)
        ctx.profile_enable(False)
        prof = ctx.profile_get()
        out["kernel_us_per_launch_8"] = {k: round(prof[k][0] / prof[k][1] * 1e3, 1) for k in
                                         ("tgt_grid_rows", "tgt_rows", "gt_misc") if prof[k][1]}
        ctx.temporal_keep_stages(False)
        ms_match_off, _ = timed(lambda: ctx.temporal_match(stages=1, fetch=False), 10)    # off again, after on: the order
        out["temporal_match_again_ms"] = ms_match_off
    print(json.dumps(out))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child()
    # a fresh process; after a fault, an abort or a time limit nothing more is started
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], timeout=LIMIT, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        sys.exit(p.returncode)
    print(p.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    main()
