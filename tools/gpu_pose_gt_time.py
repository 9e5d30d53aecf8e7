"""Microseconds per call of the pose stage under ground truth on the armed half-size EuRoC slot (tests/tgt_cases.py
RESIDENT["euroc-half"]: keyframe "kf", frame "cf2", armed with the relative pose alone): the GT-row search
(ebvo_temporal_estimate_pose_gt), the constraint cascade at the reference's 20 x 5000 draws and at 1 x 5000 draws
(ebvo_temporal_pose_constraint_metrics), and the unfiltered search on the same slot for comparison.  Prints one JSON line."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from edge_based_visual_odometry_amd import synth  # noqa: E402
from edge_based_visual_odometry_amd.api import Context  # noqa: E402
from tests import temporal_cases as tc  # noqa: E402
from tests import tgt_cases as cases  # noqa: E402


def timed(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        r = fn()
    return (time.perf_counter() - t0) / reps * 1e6, r


def main():
    F, calib = tc.rig()
    kf, cf, px = cases.RESIDENT["euroc-half"]
    R, t = cases.resident_pose(px)
    out = {}
    with Context(*synth.SHAPES["euroc"], device=0) as ctx:
        for name in (kf, cf):
            ctx.stereo_upload(*tc.images(name))
            ctx.stereo_run(ctx.default_params(F))
            ctx.stereo_finalize(calib)
            if name == kf:
                ctx.temporal_set_keyframe()
        counts, _ = ctx.temporal_match(stages=1)
        armed = ctx.temporal_set_gt(R, t, calib)
        out["slot"] = dict(n_final=int(counts["n_final"]), n_listed_rows=armed["n_rows"], n_veridical=armed["n_veridical"])
        us, r = timed(lambda: ctx.temporal_estimate_pose(calib), 50)
        out["search_all_rows"] = dict(n_quads=int(r["n_quads"]), us_per_call=round(us, 1), draws=int(r["draws"]))
        us, r = timed(lambda: ctx.temporal_estimate_pose_gt(calib), 50)
        out["search_gt_rows"] = dict(n_quads=int(r["n_quads"]), us_per_call=round(us, 1), draws=int(r["draws"]))
        for n_runs, reps in ((20, 20), (1, 50)):
            us, runs = timed(lambda: ctx.temporal_pose_constraint_metrics(calib, n_runs=n_runs), reps)
            out[f"cascade_{n_runs}x5000"] = dict(n_quads=int(runs[0].n_quads), us_per_call=round(us, 1),
                                                 surviving=[g["surviving"] for g in runs[0]])
    print(json.dumps(out))


if __name__ == "__main__":
    main()
