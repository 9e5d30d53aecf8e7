"""Oracle-side temporal ground truth: a float64 restatement, from the reference text, of

  Temporal_Matches::build_Veridical_Quads                   src/Temporal_Matches.cpp:57-166
  Temporal_Matches::orientation_mapping                     src/Temporal_Matches.cpp:294-333
  SpatialGrid::getCandidatesWithinRadius(cv::Point2d, r)     include/Dataset.h:92-113
  Temporal_Matches::Evaluate_Temporal_Edge_Pairs_on_Quads    src/Temporal_Matches.cpp:220-292
  Utility::get_Relative_Pose                                src/utility.cpp:121-128

Test infrastructure: the device path (ebvo_temporal_set_gt / ebvo_tgt_veridical / ebvo_tgt_evaluate_rows) is compared with
THIS, bit for bit.  Every product of a 3x3 matrix and a vector is (a + b) + c per row, one numpy ufunc per operation (IEEE
double, no FMA); sin / cos / atan2 are the portable ones of the C oracle (tests/oracle.py), the keyframe mate's triangulated
point and 3-D tangent are columns 6-11 of its finalize_pairs.  Parity with the reference binary is UNPINNED, as for the rest
of the temporal path (no reference build here): the restatement follows the source text, and two of its choices are
conventions -- (R_stereo * rel_pose.R) * T_1 is formed as the expression binds (the 3x3 product first), and the four doubles
of a stage are summed in keyframe index order, the reference's one-thread order (its own order depends on OpenMP
scheduling).  A projection with a NaN coordinate is outside the image (the reference casts it to an int: undefined).
"""
from __future__ import annotations

import math

import numpy as np

from tests import oracle as orc
from tests.oracle_gt import inverse3

RAD_TO_DEG = 180.0 / math.pi
DEFAULTS = dict(orient_thr_deg=10.0, tp_dist=2.0, search_radius=20.0, img_margin=10.0)
STAGE_NAMES = ("Location Proximity", "Orientation", "NCC", "SIFT", "BNB-NCC", "BNB-SIFT", "Photometric Refinement",
               "Edge Clustering")
(GRID, ORIENTATION, NCC, SIFT, BNB_NCC, BNB_SIFT, REFINE, CLUSTER) = range(8)


def relative_pose(R_source, t_source, R_target, t_target):
    """Utility::get_Relative_Pose: rel_R = R_target R_source^T, rel_T = -rel_R t_source + t_target."""
    R = np.asarray(R_target, dtype=np.float64).reshape(3, 3) @ np.asarray(R_source, dtype=np.float64).reshape(3, 3).T
    return R, -R @ np.asarray(t_source, dtype=np.float64) + np.asarray(t_target, dtype=np.float64)


def _m(M):
    return [[float(v) for v in row] for row in np.asarray(M, dtype=np.float64).reshape(3, 3)]


def _mv(M, v):
    """rows of v through the 3x3 M: (m0 v0 + m1 v1) + m2 v2"""
    return np.stack([(M[i][0] * v[:, 0] + M[i][1] * v[:, 1]) + M[i][2] * v[:, 2] for i in range(3)], axis=1)


def _project(K, G):
    p = _mv(K, G)
    z = p[:, 2].copy()
    return np.stack([p[:, 0] / z, p[:, 1] / z, p[:, 2] / z], axis=1)          # projected_point /= projected_point.z()


def _mapped_orientation(T2, p, Kinv):
    g = np.stack([p[:, 0] / p[:, 2], p[:, 1] / p[:, 2], p[:, 2] / p[:, 2]], axis=1)      # :325
    ray = _mv(Kinv, g)                                                                     # :327-329
    t = np.stack([T2[:, i] - T2[:, 2] * ray[:, i] for i in range(3)], axis=1)              # src/utility.cpp:116
    z = (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]
    n = np.sqrt(z)
    pos = z > 0                                                                            # Eigen's normalize()
    tx, ty = np.where(pos, t[:, 0] / n, t[:, 0]), np.where(pos, t[:, 1] / n, t[:, 1])
    return orc.atan2_v(ty, tx, orc.PORTABLE)                                               # :332


def project(kf_left, kf_right, R, t, calib, img_w, img_h, kf_gamma=None, img_margin=10.0):
    """:82-105 per keyframe mate: in_image, proj_left / proj_right [n, 2], orient_left / orient_right."""
    K_left, K_right, R21, T21 = calib
    Kl, Kr, S = _m(K_left), _m(K_right), _m(R21)
    Kli, Kri = inverse3(Kl), inverse3(Kr)
    T21 = [float(v) for v in np.asarray(T21, dtype=np.float64).reshape(3)]
    Rm = _m(R)
    tv = [float(v) for v in np.asarray(t, dtype=np.float64).reshape(3)]
    n = len(kf_left)
    with np.errstate(all="ignore"):
        fin = orc.finalize_pairs(K_left, K_right, R21, T21, kf_left, kf_right)
        G = fin[:, 6:9] if kf_gamma is None else np.ascontiguousarray(kf_gamma, dtype=np.float64).reshape(n, 3)
        T1 = fin[:, 9:12]
        Gc = _mv(Rm, G)
        Gc = np.stack([Gc[:, i] + tv[i] for i in range(3)], axis=1)                        # :83
        ql = _project(Kl, Gc)
        Gr = _mv(S, Gc)
        Gr = np.stack([Gr[:, i] + T21[i] for i in range(3)], axis=1)                       # :87
        qr = _project(Kr, Gr)
        SR = [[(S[i][0] * Rm[0][j] + S[i][1] * Rm[1][j]) + S[i][2] * Rm[2][j] for j in range(3)] for i in range(3)]
        ol = _mapped_orientation(_mv(Rm, T1), ql, Kli)                                     # :317
        orr = _mapped_orientation(_mv(SR, T1), qr, Kri)                                    # :321
        x_max, y_max = float(img_w) - img_margin, float(img_h) - img_margin
        inside = ((ql[:, 0] > img_margin) & (ql[:, 1] > img_margin) & (ql[:, 0] < x_max) & (ql[:, 1] < y_max) &
                  (qr[:, 0] > img_margin) & (qr[:, 1] > img_margin) & (qr[:, 0] < x_max) & (qr[:, 1] < y_max))
    return dict(in_image=inside.astype(np.uint8), proj_left=np.ascontiguousarray(ql[:, :2]),
                proj_right=np.ascontiguousarray(qr[:, :2]), orient_left=ol, orient_right=orr)


class SpatialGrid:
    """add_edges_to_spatial_grid (:16-55) for one camera: mate i is in cell (int)x / cell, (int)y / cell if both lie inside"""

    def __init__(self, edges, img_w, img_h, cell):
        self.cell, self.gw, self.gh = cell, (img_w + cell - 1) // cell, (img_h + cell - 1) // cell
        self.cells = [[] for _ in range(self.gw * self.gh)]
        gx = np.trunc(np.trunc(edges["x"]) / cell).astype(np.int64)
        gy = np.trunc(np.trunc(edges["y"]) / cell).astype(np.int64)
        for i in range(len(edges)):
            if 0 <= gx[i] < self.gw and 0 <= gy[i] < self.gh:
                self.cells[gy[i] * self.gw + gx[i]].append(i)

    def within_radius(self, x, y, radius):
        """getCandidatesWithinRadius(cv::Point2d, radius) (include/Dataset.h:92-113)"""
        gx, gy = int(x) // self.cell, int(y) // self.cell      # x, y > 0 here: floor division is C's
        sr = int(math.ceil(radius / self.cell)) if math.isfinite(radius) else self.gw + self.gh
        sr = min(sr, self.gw + self.gh)                        # cells further out are outside the grid either way
        out = []
        for dy in range(-sr, sr + 1):
            for dx in range(-sr, sr + 1):
                nx, ny = gx + dx, gy + dy
                if 0 <= nx < self.gw and 0 <= ny < self.gh:
                    out.extend(self.cells[ny * self.gw + nx])
        return out


def _orient_ok(po, th, thr):
    od = np.abs((po - th) * RAD_TO_DEG)                        # :124
    od = np.where(od > 180.0, 360.0 - od, od)
    return (od < thr) | (np.abs(od - 180.0) < thr)             # :132


def veridical(proj, cf_left, cf_right, img_w, img_h, cell=15, orient_thr_deg=10.0, tp_dist=2.0, search_radius=20.0):
    """:107-144: CSR (row_ptr, idx) of the veridical current-frame mates per keyframe mate, in the order of left_candidates."""
    gl, gr = SpatialGrid(cf_left, img_w, img_h, cell), SpatialGrid(cf_right, img_w, img_h, cell)
    lx, ly, lth = (np.ascontiguousarray(cf_left[f], dtype=np.float64) for f in ("x", "y", "theta"))
    rx, ry, rth = (np.ascontiguousarray(cf_right[f], dtype=np.float64) for f in ("x", "y", "theta"))
    n = len(proj["in_image"])
    rows, cnt = [], np.zeros(n, dtype=np.int64)
    for i in np.flatnonzero(proj["in_image"]):
        plx, ply = (float(v) for v in proj["proj_left"][i])
        prx, pry = (float(v) for v in proj["proj_right"][i])
        left_c = gl.within_radius(plx, ply, search_radius)
        right_set = set(gr.within_radius(prx, pry, search_radius))
        c = np.array([j for j in left_c if j in right_set], dtype=np.int64)
        if not len(c):
            continue
        with np.errstate(all="ignore"):
            dxl, dyl, dxr, dyr = lx[c] - plx, ly[c] - ply, rx[c] - prx, ry[c] - pry
            ok = ((np.sqrt(dxl * dxl + dyl * dyl) < tp_dist) & (np.sqrt(dxr * dxr + dyr * dyr) < tp_dist) &
                  _orient_ok(float(proj["orient_left"][i]), lth[c], orient_thr_deg) &
                  _orient_ok(float(proj["orient_right"][i]), rth[c], orient_thr_deg))
        c = c[ok]
        cnt[i] = len(c)
        rows.append(c)
    row_ptr = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)
    idx = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
    return row_ptr, idx


def build_veridical_quads(kf_left, kf_right, cf_left, cf_right, R, t, calib, img_w, img_h, kf_gamma=None, cell=15, **params):
    """build_Veridical_Quads: the projections plus ver_row_ptr / ver_idx."""
    p = dict(DEFAULTS, **params)
    out = project(kf_left, kf_right, R, t, calib, img_w, img_h, kf_gamma, p["img_margin"])
    out["ver_row_ptr"], out["ver_idx"] = veridical(out, cf_left, cf_right, img_w, img_h, cell, p["orient_thr_deg"], p["tp_dist"],
                                                   p["search_radius"])
    return out


def row_on(ver_row_ptr, kf_is_tp=None):
    """the rows of the evaluation: a veridical quad (the mate is in `out`) and KF_stereo_mate->b_is_TP (:233)"""
    on = np.diff(ver_row_ptr) > 0
    if kf_is_tp is not None:
        on &= np.asarray(kf_is_tp) != 0
    return on.astype(np.uint8)


def evaluate_rows(row_ptr, left_centres, right_centres, on, proj_left, proj_right, tp_dist=2.0):
    """:242-257: (n, tp) per keyframe mate (zero where off) and b_is_TP per quad (zero on rows that are off)."""
    n_kf = len(row_ptr) - 1
    n_tp = np.zeros((n_kf, 2), dtype=np.int32)
    flags = np.zeros(int(row_ptr[-1]), dtype=np.uint8)
    lx, ly = (np.ascontiguousarray(left_centres[f], dtype=np.float64) for f in ("x", "y"))
    rx, ry = (np.ascontiguousarray(right_centres[f], dtype=np.float64) for f in ("x", "y"))
    for i in np.flatnonzero(on):
        b, e = int(row_ptr[i]), int(row_ptr[i + 1])
        if e > b:
            with np.errstate(all="ignore"):
                dxl, dyl = lx[b:e] - proj_left[i, 0], ly[b:e] - proj_left[i, 1]
                dxr, dyr = rx[b:e] - proj_right[i, 0], ry[b:e] - proj_right[i, 1]
                hit = (np.sqrt(dxl * dxl + dyl * dyl) < tp_dist) & (np.sqrt(dxr * dxr + dyr * dyr) < tp_dist)   # :248
            flags[b:e] = hit
            n_tp[i] = (e - b, int(hit.sum()))
    return n_tp, flags


def metrics(n_tp, on):
    """:258-291 from the per-row (n, tp), rows in keyframe index order; the zero-return rule of :274-278."""
    rows = matched = with_tp = sum_tp = sum_n = 0
    recall_sum = precision_sum = ambiguity_sum = 0.0
    for i in range(len(on)):
        if not on[i]:
            continue
        n, tp = int(n_tp[i][0]), int(n_tp[i][1])
        recall_sum = recall_sum + (1.0 if tp >= 1 else 0.0)                     # :259, :263
        precision_sum = precision_sum + (0.0 if n == 0 else float(tp) / float(n))  # :260, :264
        ambiguity_sum = ambiguity_sum + float(n)                                # :261, :265
        rows += 1
        matched += n > 0
        with_tp += tp > 0
        sum_tp += tp
        sum_n += n
    out = dict(rows=rows, nonempty=int(matched), rows_with_tp=int(with_tp), sum_tp=sum_tp, sum_n=sum_n, recall=0.0, precision=0.0,
               precision_pair=0.0, ambiguity=0.0)
    if rows == 0 or matched == 0:                                               # :274
        return out
    out["recall"] = recall_sum / float(rows)                                    # :280
    out["precision"] = out["precision_pair"] = precision_sum / float(matched)   # :281, :291
    out["ambiguity"] = (ambiguity_sum / float(matched)) - 1.0                   # :282
    return out


def evaluate_stage(row_ptr, left_centres, right_centres, on, proj, tp_dist=2.0):
    n_tp, flags = evaluate_rows(row_ptr, left_centres, right_centres, on, proj["proj_left"], proj["proj_right"], tp_dist)
    return n_tp, flags, metrics(n_tp, on)
