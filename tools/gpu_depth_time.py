"""What the inverse-depth filter costs per tracked frame at the EuRoC frame size (480 x 752, the synthetic frames of
tools/gpu_align_time.py: keyframe 0 against frame 2, the rig of config/euroc.yaml with its undistortion), host wall microseconds
per call on the same resident scene:

  refine_depth_c2 / refine_depth_c1   ebvo_temporal_refine_depth, cameras 2 or 1 (default parameters): the alignment's grids
                                      and one association, then the update and the record
  align_off                           ebvo_temporal_align_pose, default parameters, ebvo_temporal_use_depth off -- the form the
                                      parent commit has too
  align_on                            the same with the switch on and a fused state (one more launch over the prepared planes)

The forms alternate in one process (a round runs each once), REPS rounds after WARMUP; mean, median and the fastest round per
form.  The start pose is the search's.  The state is fused once before the rounds and every refine_depth form starts from a
reset, so that every round of a form computes the same thing.  --baseline-only measures align_off alone; --root DIR imports the
package from another checkout (a build of the parent commit: it has no filter), so that the two can be compared in one GPU
session.  The measurement is a child process under its own time limit; a child that fails ends the run.  Prints one JSON line."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

LIMIT = 420
WARMUP, REPS = 10, 100


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
        info = {}

        def align(name, on):
            def run():
                if not baseline_only:
                    ctx.temporal_use_depth(on)
                r = ctx.temporal_align_pose(calib, R, t)
                info[name] = dict(status=r["status"], rounds_run=r["rounds_run"], steps_kept=r["steps_kept"], n_assoc=list(r["n_assoc"]),
                                  rms_normal=round(r["rms_normal"], 4))
                return r["inliers"]
            return run

        forms = {"align_off": align("align_off", False)}
        if not baseline_only:
            def refine(name, cameras):
                def run():
                    ctx.temporal_depth_reset()                 # a flag on the host: every round starts from the prior
                    r = ctx.temporal_refine_depth(calib, R, t, cameras=cameras)
                    info[name] = dict(n_updated=r["n_updated"], n_restored=r["n_restored"], n_dead=r["n_dead"], n_terms=list(r["n_terms"]),
                                      n_gated=list(r["n_gated"]), rms_before=round(r["rms_before"], 4), rms_after=round(r["rms_after"], 4))
                    return r["n_updated"]
                return run
            # refine_depth_c2 runs last in a round: align_on of the next round finds the state it left
            forms["align_on"] = align("align_on", True)
            forms["refine_depth_c1"] = refine("refine_depth_c1", 1)
            forms["refine_depth_c2"] = refine("refine_depth_c2", 2)
            ctx.temporal_refine_depth(calib, R, t)
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
        if not baseline_only:
            ctx.temporal_use_depth(False)
        out = {"rounds": REPS, "frame": [h, w], "n_kf": counts["n_kf"], "edges": [pair.n_left, pair.n_right],
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
