"""CPU restatement of the pose stage under ground truth (src/MotionTracker.cpp:68-106, :175-253, :255-434) -- the checker of
ebvo_pose_from_quads_gt / ebvo_temporal_estimate_pose_gt and ebvo_pose_constraint_metrics /
ebvo_temporal_pose_constraint_metrics (test infrastructure).  tests/oracle_pose.py is imported unchanged.

Both functions are restated literally: get_Quad_for_Pose_Solution skips the rows that are not listed (not in quads_by_kf) or
whose keyframe mate is not a true positive (:78), pushes the quads of the others and SORTS them (:92-103); then the search
(:175-253) or the five-stage cascade of Solution_Constraints_Application (:255-381) runs over that list with a GlibcRand.
The four constraints are restated one function each, as the reference has them (:108-134)."""
from __future__ import annotations

import math

import numpy as np

from tests import oracle_pose as op

STAGE_NAMES = ("Baseline", "Normalized Length Constraint", "T1 Angle Similarity Constraint", "T2 Angle Similarity Constraint",
               "Tangent Angle Similarity Constraint")
VERIDICAL_BIT = 0x80


def selected_quads(row_ptr, row_listed=None, kf_is_tp=None):
    """get_Quad_for_Pose_Solution under has_gt(): (n_listed, [(KF index, candidate index, CSR index)] in rank order)"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n_kf = len(row_ptr) - 1
    n_listed = 0
    quads = []
    for k in range(n_kf):
        if row_listed is not None and not row_listed[k]:
            continue                                    # the mate has no veridical quad: it is not in quads_by_kf
        n_listed += 1
        if kf_is_tp is not None and not kf_is_tp[k]:
            continue                                    # :78
        for j in range(int(row_ptr[k]), int(row_ptr[k + 1])):
            quads.append((k, j - int(row_ptr[k]), j))
    size = np.diff(row_ptr)
    quads.sort(key=lambda q: (int(size[q[0]]), q[0], q[1]))   # :92-103
    return n_listed, quads


def length_constraint(q1, q2, tau):
    lG = math.sqrt(op._dot(op._sub(q1[0:3], q2[0:3]), op._sub(q1[0:3], q2[0:3])))
    lGb = math.sqrt(op._dot(op._sub(q1[3:6], q2[3:6]), op._sub(q1[3:6], q2[3:6])))
    return op._div(abs(lG - lGb), lG) < tau


def _cos_pair(q1, q2, T, Tb):
    d, db = op._sub(q2[0:3], q1[0:3]), op._sub(q2[3:6], q1[3:6])
    return (op._div(op._dot(d, T), math.sqrt(op._dot(d, d))), op._div(op._dot(db, Tb), math.sqrt(op._dot(db, db))))


def t1_constraint(q1, q2, tau):
    c, cb = _cos_pair(q1, q2, q1[6:9], q1[9:12])
    return abs(abs(c) - abs(cb)) < tau


def t2_constraint(q1, q2, tau):
    c, cb = _cos_pair(q1, q2, q2[6:9], q2[9:12])
    return abs(abs(c) - abs(cb)) < tau


def tangent_constraint(q1, q2, tau):
    c, cb = op._dot(q1[6:9], q2[6:9]), op._dot(q1[9:12], q2[9:12])
    return abs(abs(c) - abs(cb)) < tau


CONSTRAINTS = (length_constraint, t1_constraint, t2_constraint, tangent_constraint)


def _draw(rng, top_n):
    while True:
        i1 = rng.rand() % top_n
        i2 = rng.rand() % top_n
        if i1 != i2:
            return i1, i2


def _setup(kf_left, kf_right, row_ptr, cf_left, cf_right, K_left, R21, T21, row_listed, kf_is_tp, p):
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n_full = int(row_ptr[-1])
    n_listed, quads = selected_quads(row_ptr, row_listed, kf_is_tp)
    n = len(quads)
    top_n = int(p["top_rank_fraction"] * float(n))
    insufficient = n_listed < 2 or n < 2 or top_n < 2
    geom = None
    if not insufficient:
        geom = op.quad_geometry(kf_left, kf_right, row_ptr, cf_left, cf_right, K_left, R21, T21)
    return n_full, quads, n, top_n, insufficient, geom


def estimate_pose_gt(kf_left, kf_right, row_ptr, cf_left, cf_right, K_left, R21, T21, row_listed=None, kf_is_tp=None, rng=None,
                     **params):
    """The search over the selected quads.  Returns the fields of ebvo_pose_result (n_quads = the selected count, best_q1 /
    best_q2 = positions in the selected rank order) plus inlier and quad_geom in the full CSR order (zero off the selection),
    rank_order (full-CSR indices, -1 beyond the selected count) and the generator.  Status 1: quad_geom and rank_order None."""
    p = dict(op.DEFAULTS, **params)
    if rng is None:
        rng = op.GlibcRand(p["rand_seed"])
    n_full, quads, n, top_n, insufficient, geom_full = _setup(kf_left, kf_right, row_ptr, cf_left, cf_right, K_left, R21, T21,
                                                              row_listed, kf_is_tp, p)
    out = dict(status=0, found=False, n_quads=n, top_n=top_n, iterations=0, draws=0, hypotheses=0, best_inliers=0,
               dynamic_max_iter=p["max_iterations"], inlier_ratio=0.0, best_q1=-1, best_q2=-1, R=np.eye(3), t=np.zeros(3),
               inlier=np.zeros(n_full, dtype=np.uint8), quad_geom=None, rank_order=None, rng=rng)
    if insufficient:
        out["status"] = 1
        return out
    csr = np.array([q[2] for q in quads], dtype=np.int64)          # the list, in rank order
    K = tuple(op._kmat(K_left).reshape(9).tolist())
    sel = np.zeros(n_full, dtype=bool)
    sel[csr] = True
    out["quad_geom"] = np.where(sel[:, None], geom_full, 0.0)
    out["rank_order"] = np.concatenate([csr, np.full(n_full - n, -1)]).astype(np.int32)
    rows = [tuple(r) for r in geom_full[csr].tolist()]
    G = np.ascontiguousarray(geom_full[csr, 0:3])                  # the score runs over the list (:155-173)
    cf = np.asarray(cf_left)[csr]
    cf_xy = np.stack([cf["x"], cf["y"]], axis=1)
    tau = (p["tau_length"], p["tau_t1"], p["tau_t2"], p["tau_tangent"])
    max_it, min_it, thr = p["max_iterations"], p["min_iterations"], p["max_reproj_error"]
    log_prob_missing_model = math.log(1.0 - p["success_prob"])
    it, dyn, best, ratio, draws, hyps = 0, max_it, 0, 0.0, 0, 0
    best_rt = None
    status = 0
    while True:
        if not (it < max_it) or (it > min_it and it > dyn):
            break
        if draws >= p["max_draws"]:
            status = 2
            break
        i1, i2 = _draw(rng, top_n)
        draws += 1
        q1, q2 = rows[i1], rows[i2]
        if not all(c(q1, q2, t) for c, t in zip(CONSTRAINTS, tau)):
            it = it - 1 if it > 0 else 0
            it += 1
            continue
        hyps += 1
        R, t = op.pose_from_pair(q1, q2)
        c = int(op.inliers(R, t, G, cf_xy, K, thr).sum())
        if c > best:
            best, ratio, best_rt = c, c / n, (R, t)
            out["best_q1"], out["best_q2"] = i1, i2
        if ratio >= 0.95:
            dyn = min_it
        elif ratio <= 0.05:
            dyn = max_it
        else:
            prob_outlier = 1.0 - ratio * ratio
            v = log_prob_missing_model / math.log(prob_outlier) * p["dyn_num_trials_mult"]
            v = 0 if not (v > 0) else min(math.ceil(v), 1 << 62) if math.isfinite(v) else 1 << 62
            dyn = v
        it += 1
    out.update(status=status, iterations=it, draws=draws, hypotheses=hyps, best_inliers=best, dynamic_max_iter=dyn,
               inlier_ratio=ratio, found=best > 0)
    if best > 0:
        R, t = best_rt
        out["R"], out["t"] = np.array(R).reshape(3, 3), np.array(t)
        out["inlier"][csr] = op.inliers(R, t, G, cf_xy, K, thr).astype(np.uint8)
    return out


def _ratio(a, b):
    """static_cast<double>(a) / static_cast<double>(b), 0 / 0 included"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def constraint_metrics(kf_left, kf_right, row_ptr, cf_left, cf_right, K_left, R21, T21, row_listed=None, kf_is_tp=None,
                       quad_is_tp=None, n_runs=1, rng=None, **params):
    """Solution_Constraints_Application, n_runs times over one generator.  Returns dict(runs, draw_idx, draw_stage, rng); a run
    is dict(status, n_quads, top_n, draws, stages) and a stage dict(name, stage, surviving, veridical, recall, precision).
    Insufficient quads: status 1 and zeros in every run, draw_idx / draw_stage None."""
    p = dict(op.DEFAULTS, **params)
    if rng is None:
        rng = op.GlibcRand(p["rand_seed"])
    n_full, quads, n, top_n, insufficient, geom_full = _setup(kf_left, kf_right, row_ptr, cf_left, cf_right, K_left, R21, T21,
                                                              row_listed, kf_is_tp, p)
    max_it = p["max_iterations"]
    if insufficient:
        zero = [dict(name=STAGE_NAMES[k], stage=k, surviving=0, veridical=0, recall=0.0, precision=0.0) for k in range(5)]
        runs = [dict(status=1, n_quads=n, top_n=top_n, draws=0, stages=[dict(s) for s in zero]) for _ in range(n_runs)]
        return dict(runs=runs, draw_idx=None, draw_stage=None, rng=rng)
    csr = [q[2] for q in quads]
    rows = [tuple(r) for r in geom_full[csr].tolist()]
    ver = [bool(quad_is_tp[c]) if quad_is_tp is not None else False for c in csr]   # b_is_veridical (:85)
    tau = (p["tau_length"], p["tau_t1"], p["tau_t2"], p["tau_tangent"])
    draw_idx = np.zeros((n_runs, max_it, 2), dtype=np.int32)
    draw_stage = np.zeros((n_runs, max_it), dtype=np.uint8)
    runs = []
    for r in range(n_runs):
        indices = []
        num_veridical = 0
        for _ in range(max_it):                                   # :274-290
            i1, i2 = _draw(rng, top_n)
            indices.append((i1, i2))
            if ver[i1] and ver[i2]:
                num_veridical += 1
        initial = num_veridical
        stages = [dict(name=STAGE_NAMES[0], stage=0, surviving=max_it, veridical=num_veridical, recall=1.0,
                       precision=_ratio(num_veridical, max_it))]
        passed = [0] * max_it
        last = list(range(max_it))                                # positions in `indices` of the surviving pairs
        for k, (fn, t) in enumerate(zip(CONSTRAINTS, tau), start=1):
            num_veridical, surviving = 0, []
            for i in last:
                i1, i2 = indices[i]
                if fn(rows[i1], rows[i2], t):
                    surviving.append(i)
                    passed[i] = k
                    if ver[i1] and ver[i2]:
                        num_veridical += 1
            stages.append(dict(name=STAGE_NAMES[k], stage=k, surviving=len(surviving), veridical=num_veridical,
                               recall=_ratio(num_veridical, initial),
                               precision=0.0 if len(surviving) == 0 else _ratio(num_veridical, len(surviving))))
            last = surviving
        for i, (i1, i2) in enumerate(indices):
            draw_idx[r, i] = (i1, i2)
            draw_stage[r, i] = passed[i] | (VERIDICAL_BIT if ver[i1] and ver[i2] else 0)
        runs.append(dict(status=0, n_quads=n, top_n=top_n, draws=max_it, stages=stages))
    return dict(runs=runs, draw_idx=draw_idx, draw_stage=draw_stage, rng=rng)


def compact(kf_left, kf_right, row_ptr, cf_left, cf_right, on):
    """the CSR of the rows with on[i] set, and the CSR index of each of its quads"""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    on = np.asarray(on).astype(bool)
    lens = np.diff(row_ptr)
    keep_q = np.repeat(on, lens)
    rp = np.concatenate([[0], np.cumsum(lens[on])]).astype(np.int32)
    return (np.asarray(kf_left)[on], np.asarray(kf_right)[on], rp, np.asarray(cf_left)[keep_q], np.asarray(cf_right)[keep_q],
            np.flatnonzero(keep_q))


def mean_over_runs(runs):
    """Print_Quad_Pairs_Metrics_Statistics (:383-434): per stage of the first run, sums in run order over the run count"""
    out = []
    for ref in runs[0]["stages"]:
        sr, sp, sv, count = 0.0, 0.0, 0, 0
        for run in runs:
            for m in run["stages"]:
                if m["name"] == ref["name"]:
                    sr += m["recall"]
                    sp += m["precision"]
                    sv += m["veridical"]
                    count += 1
                    break
        if count:
            out.append(dict(name=ref["name"], recall=sr / float(count), precision=sp / float(count), veridical=sv / float(count)))
    return out
