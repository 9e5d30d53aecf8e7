"""What a pose prior costs and saves in the temporal match at the EuRoC frame size (480 x 752, the synthetic frames of the
temporal tools: keyframe 0 against frame 2, the rig of config/euroc.yaml with its undistortion): host wall milliseconds per
ebvo_temporal_match (stages = 1, ending in the wait, nothing fetched) in three forms -- without a prior; under the identity
prior at the default radius of 30 px; under the identity prior at a radius of 8 px -- with the candidate and final counts of
each form beside the times.  The forms alternate in one process (a round runs each once), REPS rounds after WARMUP; mean,
median and the fastest round per form.  --unprimed-only measures the first form alone (a library built before the prior
existed has nothing else).  The measurement is a child process under its own time limit; a child that fails ends the run.
Prints one JSON line."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LIMIT = 420
WARMUP, REPS = 10, 200


def child(unprimed_only):
    import numpy as np

    from edge_based_visual_odometry_amd import synth
    from edge_based_visual_odometry_amd.api import Context

    h, w = synth.SHAPES["euroc"]
    cal = synth.CALIB["euroc"]
    F = synth.fundamental_for("euroc")
    calib = ([cal["K"][0], 0, cal["K"][2], 0, cal["K"][1], cal["K"][3], 0, 0, 1],
             [cal["K_right"][0], 0, cal["K_right"][2], 0, cal["K_right"][1], cal["K_right"][3], 0, 0, 1], cal["R21"], cal["T21"])
    R, t = np.eye(3), np.zeros(3)
    with Context(h, w, device=0) as ctx:
        if "dist" in cal:
            ctx.set_undistort(cal["K"], cal["dist"], cal["K_right"], cal["dist_right"])

        def frame(k):
            l, r = synth.stereo_pair("s2", h, w, scene=7, noise_base=2 * k, disparity=9)
            ctx.stereo_upload(np.roll(l, k, axis=1), np.roll(r, k, axis=1))
            ctx.stereo_run(ctx.default_params(F))
            ctx.stereo_finalize(calib, use_sift=True)

        frame(0)
        ctx.temporal_set_keyframe()
        frame(2)

        def unprimed():
            return ctx.temporal_match(stages=1, fetch=False)[0]

        def primed(radius):
            ctx.temporal_set_prior(R, t, calib)
            return ctx.temporal_match(stages=1, fetch=False, grid_radius=radius)[0]

        forms = {"unprimed": unprimed}
        if not unprimed_only:
            forms.update({"identity_r30": lambda: primed(30.0), "identity_r8": lambda: primed(8.0)})
        ms = {k: [] for k in forms}
        counts = {}
        for rnd in range(WARMUP + REPS):
            for name, fn in forms.items():
                t0 = time.perf_counter()
                c = fn()
                dt = (time.perf_counter() - t0) * 1e3
                if rnd >= WARMUP:
                    ms[name].append(dt)
                assert counts.setdefault(name, c) == c, name     # every round of a form finds the same quads
        out = {"rounds": REPS, "frame": [h, w]}
        for name in forms:
            c = counts[name]
            out[name] = dict(mean_ms=round(statistics.fmean(ms[name]), 3), median_ms=round(statistics.median(ms[name]), 3),
                             min_ms=round(min(ms[name]), 3), n_kf=c["n_kf"], n_cf=c["n_cf"], n_candidates=c["n_candidates"],
                             n_kept=c["n_kept"], n_final=c["n_final"])
        if not unprimed_only:
            out["live"] = int(ctx.temporal_prior_fetch()["live"].sum())
    print(json.dumps(out))


def main():
    flags = [a for a in sys.argv[1:] if a == "--unprimed-only"]
    if "--child" in sys.argv[1:]:
        return child(bool(flags))
    # a fresh process; after a fault, an abort or a time limit nothing more is started
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", *flags], timeout=LIMIT, capture_output=True, text=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout + p.stderr)
        sys.exit(p.returncode)
    print(p.stdout.strip().splitlines()[-1])


if __name__ == "__main__":
    main()
