"""What the ground-truth evaluation costs on the ETH3D-shaped pair (942x489, bench.py --workload eth3d's generator arguments):
milliseconds per ebvo_stereo_set_gt (upload of the map, locate, pool, census, NCC rows; synchronous), and per
ebvo_stereo_finalize unarmed against armed (the armed chain adds one gt_rows + totals launch pair per stage), next to the
pair run itself for scale.  Each measurement is a child process under its own time limit; a child that fails ends the
run.  Prints one JSON line."""
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = (("arm", 120), ("finalize", 180))


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    return round((time.perf_counter() - t0) / reps * 1e3, 3), r


def child(step):
    import numpy as np

    from edge_based_visual_odometry_amd import synth
    from edge_based_visual_odometry_amd.api import Context

    h, w = synth.SHAPES["eth3d"]
    c = synth.CALIB["eth3d"]
    K = [c["K"][0], 0, c["K"][2], 0, c["K"][1], c["K"][3], 0, 0, 1]
    calib = (K, K, c["R21"], c["T21"])
    l, r = synth.stereo_pair("s2", h, w, scene=11, noise_base=4, disparity=9)
    yy, xx = np.mgrid[0:h, 0:w]
    disp = (9.0 + 0.35 * np.sin((xx + 3 * yy) * 0.07)).astype(np.float32)      # finite everywhere: every edge is located
    out = {}
    with Context(512, 1280, device=0) as ctx:
        params = ctx.default_params(synth.fundamental_for("eth3d"))
        ctx.stereo_upload(l, r)
        ms_run, counts = timed(lambda: ctx.stereo_run(params), 10)
        out.update(n_left=counts.n_left, n_right=counts.n_right, n_pairs=counts.n_pairs, pair_run_ms=ms_run)
        if step == "arm":
            ms, sz = timed(lambda: ctx.stereo_set_gt(disp, calib), 10)
            epi = ctx.stereo_gt_metrics()[0]
            out.update(set_gt_ms=ms, epipolar_stage_pairs=epi["sum_n"], **sz)
            # device time per launch (event brackets of the library's profiler): the census against the candidate search
            ctx.profile_reset()
            ctx.profile_enable(True)
            for _ in range(5):
                ctx.stereo_run(params)
                ctx.stereo_set_gt(disp, calib)
            ctx.profile_enable(False)
            prof = ctx.profile_get()
            out["kernel_us_per_launch"] = {k: round(prof[k][0] / prof[k][1] * 1e3, 1) for k in
                                           ("cand_count", "cand_fill", "gt_misc", "gt_pool", "gt_census", "gt_rows") if prof[k][1]}
        else:
            fin = lambda: ctx.stereo_finalize(calib)[0]
            ms0, c0 = timed(fin, 10)
            ctx.stereo_set_gt(disp, calib)
            ms1, c1 = timed(fin, 10)
            ms1m, _ = timed(lambda: (fin(), ctx.stereo_gt_metrics()), 10)
            assert c0 == c1
            out.update(finalize_unarmed_ms=ms0, finalize_armed_ms=ms1, finalize_armed_plus_metrics_ms=ms1m, n_final=c1["n_final"])
    print(json.dumps(out))


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(sys.argv[2])
    out = {}
    for step, limit in STEPS:
        # a fresh process per step; after a fault, an abort or a time limit nothing more is started
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step], timeout=limit, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout + p.stderr)
            sys.exit(p.returncode)
        out[step] = json.loads(p.stdout.strip().splitlines()[-1])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
