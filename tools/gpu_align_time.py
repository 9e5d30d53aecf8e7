"""What a pose costs per tracked frame at the EuRoC frame size (480 x 752, the synthetic frames of the temporal tools: keyframe
0 against frame 2, the rig of config/euroc.yaml with its undistortion), host wall microseconds per call on the same resident
scene:

  align_c2_r4 / align_c2_r1 / align_c1_r4 / align_c1_r1   ebvo_temporal_align_pose, cameras 2 or 1, rounds 4 or 1 (ten steps)
  align_c2_r4_i0                                          ... with iterations = 0: what the associations and one sum per
                                                          round cost without the forty step launches
  refine                                                  ebvo_temporal_refine_pose (default parameters) on the final quads
  match_search                                            ebvo_temporal_match (stages = 1, nothing fetched) plus
                                                          ebvo_temporal_estimate_pose: what a quad-based pose costs after
                                                          the stereo chain of the frame

The forms alternate in one process (a round runs each once), REPS rounds after WARMUP; mean, median and the fastest round per
form.  The start pose of the alignment and of the refit is the search's.  --baseline-only measures refine and match_search
alone; --root DIR imports the package from another checkout (a build of the parent commit: it has no alignment), so that the
two can be compared in one GPU session.  The measurement is a child process under its own time limit; a child that fails
ends the run.  Prints one JSON line."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LIMIT = 420
WARMUP, REPS = 10, 100


def launches(cameras, rounds, iterations):
    """kernel launches of one alignment call: init, prepare, three grid kernels per camera, an association and iterations + 1
    sums per round, the last association and the metric pass (plus one memset per camera and the copies back)"""
    return 2 + 3 * cameras + rounds * (1 + iterations + 1) + 2


def child(root, baseline_only):
    sys.path.insert(0, root)
    import numpy as np

    from edge_based_visual_odometry_amd import synth
    from edge_based_visual_odometry_amd.api import Context

    h, w = synth.SHAPES["euroc"]
    cal = synth.CALIB["euroc"]
    F = synth.fundamental_for("euroc")
    calib = ([cal["K"][0], 0, cal["K"][2], 0, cal["K"][1], cal["K"][3], 0, 0, 1],
             [cal["K_right"][0], 0, cal["K_right"][2], 0, cal["K_right"][1], cal["K_right"][3], 0, 0, 1], cal["R21"], cal["T21"])
    with Context(h, w, device=0) as ctx:
        if "dist" in cal:
            ctx.set_undistort(cal["K"], cal["dist"], cal["K_right"], cal["dist_right"])

        def frame(k):
            l, r = synth.stereo_pair("s2", h, w, scene=7, noise_base=2 * k, disparity=9)
            ctx.stereo_upload(np.roll(l, k, axis=1), np.roll(r, k, axis=1))
            c = ctx.stereo_run(ctx.default_params(F))
            ctx.stereo_finalize(calib, use_sift=True)
            return c

        frame(0)
        ctx.temporal_set_keyframe()
        pair = frame(2)
        counts = ctx.temporal_match(stages=1, fetch=False)[0]
        start = ctx.temporal_estimate_pose(calib, rand_seed=7)
        R, t = (start["R"], start["t"]) if start["found"] else (np.eye(3), np.zeros(3))

        def match_search():
            ctx.temporal_match(stages=1, fetch=False)
            return ctx.temporal_estimate_pose(calib, rand_seed=7)["best_inliers"]

        forms = {"refine": lambda: ctx.temporal_refine_pose(calib, R, t)["inliers"], "match_search": match_search}
        info = {}
        if not baseline_only:
            def align(name, **kw):
                def run():
                    r = ctx.temporal_align_pose(calib, R, t, **kw)
                    info[name] = dict(status=r["status"], stop_reason=r["stop_reason"], rounds_run=r["rounds_run"],
                                      steps_kept=r["steps_kept"], n_assoc=list(r["n_assoc"]), inliers=r["inliers"],
                                      rms_normal=round(r["rms_normal"], 4),
                                      launches=launches(kw.get("cameras", 2), kw.get("rounds", 4), kw.get("iterations", 10)))
                    return r["inliers"]
                return run
            forms = dict({"align_c2_r4": align("align_c2_r4"), "align_c2_r1": align("align_c2_r1", rounds=1),
                          "align_c1_r4": align("align_c1_r4", cameras=1), "align_c1_r1": align("align_c1_r1", cameras=1, rounds=1),
                          "align_c2_r4_i0": align("align_c2_r4_i0", iterations=0)}, **forms)
        us = {k: [] for k in forms}
        seen = {}
        for rnd in range(WARMUP + REPS):
            for name, fn in forms.items():
                t0 = time.perf_counter()
                v = fn()
                dt = (time.perf_counter() - t0) * 1e6
                if rnd >= WARMUP:
                    us[name].append(dt)
                assert seen.setdefault(name, v) == v, name            # every round of a form computes the same thing
        out = {"rounds": REPS, "frame": [h, w], "n_kf": counts["n_kf"], "n_final": counts["n_final"], "edges": [pair.n_left, pair.n_right],
               "tiles": -(-counts["n_kf"] // 1024), "search_found": bool(start["found"])}
        for name in forms:
            out[name] = dict(mean_us=round(statistics.fmean(us[name]), 1), median_us=round(statistics.median(us[name]), 1),
                             min_us=round(min(us[name]), 1), **info.get(name, {}))
    print(json.dumps(out))


def main():
    args = sys.argv[1:]
    root = os.path.abspath(args[args.index("--root") + 1]) if "--root" in args else ROOT
    baseline_only = "--baseline-only" in args
    if "--child" in args:
        return child(root, baseline_only)
    # a fresh process; after a fault, an abort or a time limit nothing more is started
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--root", root] + (["--baseline-only"] if baseline_only else [])
    p = subprocess.run(cmd, timeout=LIMIT, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        sys.exit(p.returncode)
    print(p.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    main()
