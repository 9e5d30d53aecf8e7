"""Oracle-side ground-truth evaluation: a float64 restatement, from the reference text, of

  Stereo_Matches::Find_Stereo_GT_Locations              src/Stereo_Matches.cpp:133-200
  Bilinear_Interpolation<float>                         include/utility.h:81-104
  Stereo_Matches::get_Stereo_Edge_GT_Pairs              src/Stereo_Matches.cpp:202-268 (with :111-131 and :91-109)
  Stereo_Matches::Evaluate_Stereo_Edge_Correspondences  src/Stereo_Matches.cpp:270-379

and of the per-stage evaluation of get_Stereo_Edge_Pairs (:1377-1536).  Test infrastructure: the device path
(ebvo_stereo_set_gt / ebvo_stereo_gt_metrics) is compared with THIS, bit for bit.  Python floats are IEEE doubles and
`a * b + c` is two roundings here (no FMA), as in the reference's x86-64 build.  Every sum of the metrics is a plain
sequential addition in row order (std::accumulate, :366-368): no math.fsum, no numpy.sum.

The stage lists come from the functions of tests/oracle.py composed as tests/oracle_chain.py composes them
(stereo_edge_pairs there returns the final list only; `stage_lists` below is the same composition that keeps every
intermediate list, and checks its last one against oracle_chain's).
"""
from __future__ import annotations

import math

import numpy as np

from tests import oracle as orc
from tests import oracle_chain as oc

RAD_TO_DEG = 180.0 / math.pi  # include/utility.h:290: theta * (180.0 / M_PI)

# stage ids in the reference's order and the names of Frame_Evaluation_Metrics (:1382-1535)
STAGE_NAMES = ("Epipolar Proximity", "Location Proximity", "Orientation", "SIFT", "NCC", "BNB-NCC", "BNB-SIFT",
               "Photometric Refinement", "Edge Clustering", "NCC", "Best", "Final")
(EPIPOLAR, DISPARITY, ORIENTATION, SIFT, NCC, BNB_NCC, BNB_SIFT, REFINE, CLUSTER, NCC2, BEST, FINAL) = range(12)


def bilinear_f32(m: np.ndarray, x: float, y: float) -> float:
    """Bilinear_Interpolation<float>(meshGrid, P) (include/utility.h:81-104), expression for expression.  At an integer
    x (or y) Q21.x - Q11.x is 0 and the weights are 0 / 0: NaN, as in the reference."""
    rows, cols = m.shape
    q12 = (math.floor(x), math.floor(y))      # :90
    q22 = (math.ceil(x), math.floor(y))       # :91
    q11 = (math.floor(x), math.ceil(y))       # :92
    q21 = (math.ceil(x), math.ceil(y))        # :93
    if (q11[0] < 0 or q11[1] < 0 or q21[0] >= cols or q21[1] >= rows or
            q12[0] < 0 or q12[1] < 0 or q22[0] >= cols or q22[1] >= rows):            # :95-96
        return math.nan

    def div(a, b):  # IEEE division: 0 / 0 = NaN, x / 0 = inf
        return float(np.float64(a) / np.float64(b))

    at = lambda q: float(m[q[1], q[0]])       # meshGrid.at<float>(y, x) widened to double
    with np.errstate(all="ignore"):
        wx1 = div(q21[0] - x, q21[0] - q11[0])
        wx2 = div(x - q11[0], q21[0] - q11[0])
        f_x_y1 = wx1 * at(q11) + wx2 * at(q21)                                        # :101
        f_x_y2 = wx1 * at(q12) + wx2 * at(q22)                                        # :102
        return div(q12[1] - y, q12[1] - q11[1]) * f_x_y1 + div(y - q11[1], q12[1] - q11[1]) * f_x_y2   # :103


def _cof(m, i, j):
    i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
    return m[i1][j1] * m[i2][j2] - m[i1][j2] * m[i2][j1]


def inverse3(m):
    """Eigen's Matrix3d::inverse() (cofactor form, Eigen/src/LU/InverseImpl.h), as tests/oracle_pose.py and the
    finalisation rows use it."""
    m = [[float(m[i][j]) for j in range(3)] for i in range(3)]
    c0, c1, c2 = _cof(m, 0, 0), _cof(m, 1, 0), _cof(m, 2, 0)
    det = (c0 * m[0][0] + c1 * m[1][0]) + c2 * m[2][0]
    invdet = 1.0 / det
    inv = [[0.0] * 3 for _ in range(3)]
    inv[0] = [c0 * invdet, c1 * invdet, c2 * invdet]
    for i in (1, 2):
        for j in range(3):
            inv[i][j] = _cof(m, j, i) * invdet
    return inv


def _mv(m, v):
    return [(m[i][0] * v[0] + m[i][1] * v[1]) + m[i][2] * v[2] for i in range(3)]


def find_gt_locations(left_edges, disp, K_left, R21, T21, gate_deg=4.0):
    """Find_Stereo_GT_Locations (:133-200), is_left = true, per left edge: valid (the edge reaches :162), gt_xy, gamma_left,
    gamma_right ((-1, -1) / (-1, -1, -1) where skipped: the device's fill values; the reference stores nothing there).
    An edge with a NaN or infinite coordinate is skipped (valid 0, fill -1): the reference would index the map with it;
    the device calls it out of bounds (gt_kernels.hip: bilinear_f32_nan), and that is the rule stated here."""
    K = np.asarray(K_left, dtype=np.float64).reshape(3, 3)
    R = [[float(v) for v in row] for row in np.asarray(R21, dtype=np.float64).reshape(3, 3)]
    T = [float(v) for v in np.asarray(T21, dtype=np.float64).reshape(3)]
    Ki = inverse3(K)                                                                   # calib_matrix.inverse(), :179-180
    n = len(left_edges)
    valid = np.zeros(n, dtype=np.uint8)
    gt_xy = np.full((n, 2), -1.0)
    gl, gr = np.full((n, 3), -1.0), np.full((n, 3), -1.0)
    for i in range(n):
        x, y, th = float(left_edges["x"][i]), float(left_edges["y"][i]), float(left_edges["theta"][i])
        deg = th * RAD_TO_DEG
        if abs(deg) < gate_deg or abs(deg - 180.0) < gate_deg or abs(deg + 180.0) < gate_deg:     # :146
            continue
        if not (math.isfinite(x) and math.isfinite(y)):                                # the stated rule (docstring)
            continue
        d = bilinear_f32(disp, x, y)                                                   # :152
        if math.isnan(d) or math.isinf(d) or d < 0:                                    # :154
            continue
        gx, gy = x - d, y                                                              # :159
        g1 = _mv(Ki, [x, y, 1.0])                                                      # :179
        g2 = _mv(Ki, [gx, gy, 1.0])                                                    # :180 (LEFT inverse again)
        Rg1 = _mv(R, g1)
        with np.errstate(all="ignore"):
            numerator = T[0] - T[2] * g2[0]                                            # src/utility.cpp:98
            denominator = Rg1[2] * g2[0] - Rg1[0]                                      # :99
            rho1 = float(np.float64(numerator) / np.float64(denominator))              # :100
        G = [rho1 * g1[0], rho1 * g1[1], rho1 * g1[2]]                                 # :101
        RG = _mv(R, G)
        valid[i] = 1
        gt_xy[i] = (gx, gy)
        gl[i] = G
        gr[i] = [RG[0] + T[0], RG[1] + T[1], RG[2] + T[2]]                             # :189
    return dict(valid=valid, gt_xy=gt_xy, gamma_left=gl, gamma_right=gr)


def gt_pool(left_edges, right_edges, lines, valid, gt_xy, epi_thr=0.5, dist_tol=1.0, orient_tol=5.0):
    """get_Stereo_Edge_GT_Pairs (:202-268): per valid left edge the right edges with extract_Epipolar_Edge_Indices(line,
    right, 0.5) (:99-101), cv::norm(GT - loc) < 1.0 (:120) and |deg(theta_R) - deg(theta_L)| < 5.0 (:124, no wrap),
    ascending.  Only right edges with |y_R - y_GT| < dist_tol + 1 are looked at (the norm test fails for all others)."""
    rx, ry, rth = (np.ascontiguousarray(right_edges[f], dtype=np.float64) for f in ("x", "y", "theta"))
    by_y = np.argsort(ry, kind="stable")
    ys = ry[by_y]
    nL = len(left_edges)
    cnt = np.zeros(nL, dtype=np.int64)
    pools = []
    for i in range(nL):
        if not valid[i]:
            continue
        gx, gy = float(gt_xy[i, 0]), float(gt_xy[i, 1])
        lo, hi = np.searchsorted(ys, gy - dist_tol - 1.0), np.searchsorted(ys, gy + dist_tol + 1.0, side="right")
        k = np.sort(by_y[lo:hi])
        if not len(k):
            continue
        a, b, c = (float(v) for v in lines[i])
        with np.errstate(all="ignore"):
            dist = np.abs(a * rx[k] + b * ry[k] + c) / math.sqrt((a * a) + (b * b))    # :99
            dx, dy = gx - rx[k], gy - ry[k]
            near = np.sqrt(dx * dx + dy * dy) < dist_tol                               # :120
            orient = np.abs(rth[k] * RAD_TO_DEG - float(left_edges["theta"][i]) * RAD_TO_DEG) < orient_tol   # :124
        k = k[(dist < epi_thr) & near & orient]
        cnt[i] = len(k)
        pools.append(k)
    focused = (np.asarray(valid) != 0) & (cnt > 0)                                     # :230-233, :253-267
    focused_index = np.flatnonzero(focused).astype(np.int32)
    pool_rp = np.concatenate([[0], np.cumsum(cnt[focused_index])]).astype(np.int32)
    pool_idx = (np.concatenate(pools) if pools else np.zeros(0)).astype(np.int32)
    return dict(focused=focused.astype(np.uint8), focused_index=focused_index, pool_row_ptr=pool_rp, pool_idx=pool_idx,
                pool_count=cnt)


def row_counts(row_ptr, cand_x, cand_y, focused, gt_xy, tp_dist=1.0):
    """(n, tp) per left edge (zero where not focused): the inner loop of :296-331; TP is `<=` (:305)."""
    nL = len(row_ptr) - 1
    out = np.zeros((nL, 2), dtype=np.int32)
    cx, cy = np.ascontiguousarray(cand_x, dtype=np.float64), np.ascontiguousarray(cand_y, dtype=np.float64)
    for i in np.flatnonzero(focused):
        b, e = int(row_ptr[i]), int(row_ptr[i + 1])
        if e > b:
            dx, dy = cx[b:e] - gt_xy[i, 0], cy[b:e] - gt_xy[i, 1]
            out[i] = (e - b, int(np.count_nonzero(np.sqrt(dx * dx + dy * dy) <= tp_dist)))
    return out


def metrics(n_tp, focused, drop_empty=False):
    """Evaluate_Stereo_Edge_Correspondences' totals and four doubles (:284-368) from the per-row (n, tp), rows in index
    order; drop_empty: after remove_empty_clusters (:1526).  0 / 0 is NaN, as the expression gives."""
    rows = nonempty = with_tp = sum_tp = sum_n = 0
    acc_precision = acc_pair = acc_n = 0.0
    for i in range(len(focused)):
        if not focused[i]:
            continue
        n, tp = int(n_tp[i][0]), int(n_tp[i][1])
        if drop_empty and n == 0:
            continue
        rows += 1
        if n > 0:                                                                      # :296
            nonempty += 1
            with_tp += tp > 0                                                          # :324
            sum_tp += tp
            sum_n += n
            q = float(tp) / float(n)                                                   # :328-329
            acc_precision = acc_precision + q
            acc_pair = acc_pair + q
            acc_n = acc_n + float(n)                                                   # :330
        else:
            acc_precision = acc_precision + 0.0                                        # :334

    def div(a, b):
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))

    return dict(rows=rows, nonempty=nonempty, rows_with_tp=int(with_tp), sum_tp=sum_tp, sum_n=sum_n,
                recall=div(float(with_tp), float(rows)), precision=div(acc_precision, float(rows)),            # :365-366
                precision_pair=div(acc_pair, float(nonempty)), ambiguity=div(acc_n, float(nonempty)))         # :367-368


def geometric_lists(L, R, lines, epi_thr=0.5, max_disp=25.0, orient_thr_deg=10.0, stage_mask=7):
    """The three geometric lists (:1374, :1387, :1399) of a run with `stage_mask`: the candidate lists at stage_mask & 1,
    stage_mask & 3 and stage_mask & 7, each predicate on top of the previous ones -- a stage that is switched off passes
    every pair it is given.  With no predicate enabled yet the list is every right edge on every row (built densely)."""
    out = {}
    for sid, bits in ((EPIPOLAR, 1), (DISPARITY, 3), (ORIENTATION, 7)):
        mask = stage_mask & bits
        if mask:
            r_, c_ = orc.epi_candidates(L, R, lines, epi_thr, max_disp, orient_thr_deg, stage_mask=mask)
        else:
            r_ = (np.arange(len(L) + 1, dtype=np.int64) * len(R)).astype(np.int32)
            c_ = np.tile(np.arange(len(R), dtype=np.int32), len(L))
        out[sid] = (r_, R["x"][c_].copy(), R["y"][c_].copy())
    return out


def stage_lists(left_img, right_img, F, stage1, sift=False, bnb_ratio=0.9, ncc_thr=0.6, sift_thr=500.0, bnb_sift=0.4,
                max_iter=20, tol=1e-3, huber_delta=3.0, epi_thr=0.5, max_disp=25.0, orient_thr_deg=10.0, stage_mask=7):
    """Every list Evaluate_Stereo_Edge_Correspondences sees (:1377-1536) as {stage id: (row_ptr, x, y)}; the composition of
    tests/oracle_chain.py:stereo_edge_pairs.  stage1: dict(left, right, row_ptr, col_idx, best, keep) of the oracle, formed
    with the same epi_thr, max_disp, orient_thr_deg and stage_mask."""
    L, R, rp, ci, best, keep = (stage1[k] for k in ("left", "right", "row_ptr", "col_idx", "best", "keep"))
    lines = orc.epipolar_lines(F, L)
    out = geometric_lists(L, R, lines, epi_thr, max_disp, orient_thr_deg, stage_mask)
    assert (out[ORIENTATION][0] == rp).all()
    put = lambda sid, rp_, cand: out.__setitem__(sid, (np.asarray(rp_).copy(), cand["x"].copy(), cand["y"].copy()))
    conf = None
    if sift:
        dl, dr = orc.sift_descriptors(left_img, L), orc.sift_descriptors(right_img, R)
        d = orc.sift_min_distances(dl, dr[ci], rp)
        ok = d < sift_thr                                                              # :1414
        put(SIFT, oc.filter_rows(rp, ok), R[ci[ok]])
        keep = (keep.astype(bool) & ok).astype(np.uint8)
        conf = d
    k = keep.astype(bool)
    cand = R[ci[k]].copy()
    cand["index"] = 0
    score = best[k]
    rp = oc.filter_rows(rp, k)
    if conf is not None:
        conf = conf[k]
    put(NCC, rp, cand)                                                                 # :1427
    cnt, order = orc.bnb_test(rp, score, bnb_ratio, True)                              # :1440
    idx, rp = oc.csr_select(rp, cnt, order)
    cand, score = cand[idx], score[idx]
    put(BNB_NCC, rp, cand)
    if conf is not None:
        conf = conf[idx]
        cnt, order = orc.bnb_test(rp, conf, bnb_sift, False)                           # :1452
        idx, rp = oc.csr_select(rp, cnt, order)
        cand, score, conf = cand[idx], score[idx], conf[idx]
        put(BNB_SIFT, rp, cand)
    cand = orc.epipolar_shift(cand, lines, rp)                                         # :1465
    ref = orc.gn_refine_stereo(left_img, right_img, L, lines, rp, np.stack([cand["x"], cand["y"]], 1), max_iter, tol,
                               huber_delta)                                            # :1468
    cand = cand.copy()
    cand["x"], cand["y"] = ref["refined_xy"][:, 0], ref["refined_xy"][:, 1]
    put(REFINE, rp, cand)
    cand = orc.epipolar_shift(cand, lines, rp)                                         # :1483 as its arguments bind
    cnt, centres, _ = orc.cluster_rows(cand, rp, True, False)
    idx, rp = oc.csr_select(rp, cnt, None)
    cand = centres[idx]
    put(CLUSTER, rp, cand)
    _, best2, keep2, _ = orc.ncc_pairs(left_img, right_img, L, cand, rp, ncc_thr)     # :1500
    k2 = keep2.astype(bool)
    rp = oc.filter_rows(rp, k2)
    cand, best2 = cand[k2], best2[k2]
    put(NCC2, rp, cand)
    cnt, order = orc.keep_best(rp, best2)                                              # :1513
    idx, rp = oc.csr_select(rp, cnt, order)
    cand = cand[idx]
    put(BEST, rp, cand)
    put(FINAL, rp, cand)                                                               # :1526 drops rows, not candidates
    return out, dict(left_index=np.flatnonzero(np.asarray(cnt) > 0).astype(np.int32), right=cand)


def evaluate_stages(lists, focused, gt_xy, tp_dist=1.0):
    """{stage id: (n_tp, metrics dict)} for every list of stage_lists."""
    res = {}
    for sid, (rp, x, y) in lists.items():
        n_tp = row_counts(rp, x, y, focused, gt_xy, tp_dist)
        res[sid] = (n_tp, metrics(n_tp, focused, drop_empty=(sid == FINAL)))
    return res


def disparity_map(h, w, shift, seed=0, zero_patch=False):
    """A float32 left disparity map for a synth.stereo_pair of constant `shift`: that constant, with a smooth ramp region
    (so the bilinear weights matter), a NaN band, a +inf patch and a negative patch.  zero_patch: also a patch of exact
    0.0 -- d = 0 is valid (:154 refuses only d < 0), the GT location is the edge itself, and with an identity R21 the
    back-projection's denominator (src/utility.cpp:99) is exactly 0."""
    yy, xx = np.mgrid[0:h, 0:w]
    d = np.full((h, w), float(shift), dtype=np.float32)
    ramp = (xx >= w // 2) & (xx < w // 2 + w // 4)
    d[ramp] = (float(shift) + 0.35 * np.sin((xx + 3 * yy + seed) * 0.07))[ramp].astype(np.float32)
    d[h // 3:h // 3 + 6, :] = np.nan
    d[h // 2:h // 2 + 12, w // 8:w // 8 + 20] = np.inf
    d[2 * h // 3:2 * h // 3 + 10, w // 3:w // 3 + 24] = -3.0
    if zero_patch:
        d[h // 6:h // 6 + 12, 5 * w // 8:5 * w // 8 + 30] = 0.0
    return d
