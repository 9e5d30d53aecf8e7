"""What the keyframe coverage and the frame step cost at the EuRoC frame size (480 x 752, the synthetic frames of
tools/gpu_depth_time.py and tools/gpu_carry_time.py: keyframe 0, frame 2 on slot 0, the rig of config/euroc.yaml with its
undistortion), host wall microseconds per call:

  cover           ebvo_temporal_keyframe_cover of slot 0 (default parameters, record only) after one fused frame
  track_keep      ebvo_temporal_track_frame with a policy that never switches: align, refine the depths, measure, decide
  track_switch    ebvo_temporal_track_frame with a policy that always switches: the same, then ebvo_stereo_finalize of the
                  slot and ebvo_temporal_promote_keyframe
  align_off       ebvo_temporal_align_pose, default parameters, ebvo_temporal_use_depth off         } the parts, which the
  refine_depth    ebvo_temporal_refine_depth, default parameters, from the prior                    } parent commit has
  finalize        ebvo_stereo_finalize of slot 0 (default parameters, with the calibration, no fetch)} too
  promote         ebvo_temporal_promote_keyframe of slot 0 from a keyframe that has fused frame 2   }

The forms alternate in one process (a round runs each once), REPS rounds after WARMUP; mean, median and the fastest round per
form.  Before every form that starts from the prior or follows one that replaced the keyframe, frame 0 is installed again from
slot 1 (not timed), so that every round of a form computes the same thing.  --baseline-only leaves the new forms out; --root DIR
imports the package from another checkout (a build of the parent commit), so that the two can be compared in one GPU session.
The measurement is a child process under its own time limit; a child that fails ends the run.  Prints one JSON line."""
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
        ctx.set_slots(2)
        if "dist" in cal:
            ctx.set_undistort(cal["K"], cal["dist"], cal["K_right"], cal["dist_right"])

        def frame(k, slot):
            l, r = synth.stereo_pair("s2", h, w, scene=7, noise_base=2 * k, disparity=9)
            ctx.stereo_upload(np.roll(l, k, axis=1), np.roll(r, k, axis=1), slot=slot)
            ctx.stereo_submit(ctx.default_params(F), slot=slot)
            c = ctx.stereo_wait(slot=slot)
            ctx.stereo_finalize(calib, slot=slot)
            return c

        frame(0, 1)
        ctx.temporal_set_keyframe(slot=1)
        pair = frame(2, 0)
        counts = ctx.temporal_match(stages=1, fetch=False)[0]
        start = ctx.temporal_estimate_pose(calib, rand_seed=7)
        R, t = (start["R"], start["t"]) if start["found"] else (np.eye(3), np.zeros(3))
        info = {}

        def restore():
            ctx.temporal_set_keyframe(slot=1)

        def refine():
            r = ctx.temporal_refine_depth(calib, R, t)
            info["refine_depth"] = dict(n_updated=r["n_updated"], n_restored=r["n_restored"], n_terms=list(r["n_terms"]))
            return r["n_updated"]

        def align():
            r = ctx.temporal_align_pose(calib, R, t)
            info["align_off"] = dict(status=r["status"], rounds_run=r["rounds_run"], steps_kept=r["steps_kept"], n_assoc=list(r["n_assoc"]))
            return r["inliers"]

        def finalize():
            ctx.stereo_finalize_submit(calib, slot=0)
            c, _ = ctx.stereo_finalize_wait(slot=0, fetch=False)
            info["finalize"] = dict(n_final=c["n_final"])
            return c["n_final"]

        def promote():
            r = ctx.temporal_promote_keyframe(calib, R, t)
            info["promote"] = r
            return r["n_carried"]

        def cover():
            r = ctx.temporal_keyframe_cover(calib, R, t, arrays=False)
            info["cover"] = {k: v for k, v in r.items() if k != "hist"}
            return r["n_assoc"]

        def track(name, policy):
            def run():
                r = ctx.temporal_track_frame(calib, R, t, policy=policy)
                info[name] = dict(decision=r["decision"], reasons=r["reasons"], switched=r["switched"], steps_kept=r["pose"]["steps_kept"],
                                  n_updated=r["depth"]["n_updated"], n_assoc=r["cover"]["n_assoc"], n_carried=r["carried"]["n_carried"])
                return (r["switched"], r["cover"]["n_assoc"], r["carried"]["n_carried"])
            return run

        never = dict(min_assoc=0, max_disp_bins=64, min_in_frame_share=0.0, min_assoc_share=0.0, min_cell_cover=0.0)
        always = dict(never, max_disp_bins=0)
        # (name, timed call, runs before it untimed); refine_depth leaves the fused state the cover call and the promotion read
        forms = [("refine_depth", refine, restore), ("align_off", align, None)]
        if not baseline_only:
            forms.append(("cover", cover, None))
        forms += [("finalize", finalize, None), ("promote", promote, None)]
        if not baseline_only:
            forms += [("track_keep", track("track_keep", never), restore), ("track_switch", track("track_switch", always), restore)]
        us = {k: [] for k, _, _ in forms}
        seen = {}
        for rnd in range(WARMUP + REPS):
            for name, fn, before in forms:
                if before:
                    before()
                t0 = time.perf_counter()
                v = fn()
                dt = (time.perf_counter() - t0) * 1e6
                if rnd >= WARMUP:
                    us[name].append(dt)
                assert seen.setdefault(name, v) == v, name            # every round of a form computes the same thing
        out = {"rounds": REPS, "frame": [h, w], "n_old": counts["n_kf"], "n_new": counts["n_cf"], "edges": [pair.n_left, pair.n_right],
               "search_found": bool(start["found"])}
        for name, _, _ in forms:
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
