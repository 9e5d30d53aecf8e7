"""CPU restatement of the inlier refit of the relative pose (ebvo_pose_refine_from_quads / ebvo_temporal_refine_pose) -- the
checker of the device kernel (test infrastructure).  The contract is written once in include/ebvo_hip.h; this file follows it
operation by operation:

- the per-quad terms (28 per quad: the 21 upper entries of w J^T J, the 6 of w J^T r, the robust cost) with one numpy ufunc
  per operation (IEEE double, no FMA), both cameras, `left + right`;
- the deterministic sums over 1024 virtual lanes (virtual_lane_sums);
- the 6 x 6 Cholesky, Exp and the round logic with Python floats, sin through the oracle's portable sincos.
"""
from __future__ import annotations

import math

import numpy as np

from tests import oracle as orc
from tests import oracle_pose as op

LANES, GROUP = 1024, 64
DEFAULTS = dict(rounds=2, iterations=10, huber_px=1.5, step_eps=1e-10)
STOP_EPS, STOP_CAP, STOP_COST, STOP_PIVOT, STOP_FEW = range(5)
UPPER = [(i, j) for i in range(6) for j in range(i, 6)]   # the order of the 21 entries of H in the sums


def virtual_lane_sums(terms):
    """terms: n x m (row k = the term of selected quad k, +0.0 outside the fit set) -> the m sums of the contract."""
    terms = np.asarray(terms, dtype=np.float64)
    n, m = terms.shape
    chunks = -(-n // LANES)
    pad = np.zeros((max(chunks, 1) * LANES, m))
    pad[:n] = terms
    lanes = np.zeros((LANES, m))
    for c in range(chunks):                                  # lane v adds quads v, v + 1024, ... in ascending k from +0.0
        lanes = np.add(lanes, pad[c * LANES:(c + 1) * LANES])
    x = lanes.reshape(LANES // GROUP, GROUP, m).copy()
    s = GROUP // 2
    while s >= 1:                                            # x[l] += x[l + s], l < s, within each group of 64 lanes
        x[:, :s] = np.add(x[:, :s], x[:, s:2 * s])
        s //= 2
    g = x[:, 0].copy()
    s = LANES // GROUP // 2
    while s >= 1:                                            # the 16 group sums, the same tree
        g[:s] = np.add(g[:s], g[s:2 * s])
        s //= 2
    return g[0].copy()


def _mvv(M, v):
    """mv3 of ebvo_geom.h over arrays: M 9 floats, v three arrays"""
    return [np.add(np.add(M[i * 3] * v[0], M[i * 3 + 1] * v[1]), M[i * 3 + 2] * v[2]) for i in range(3)]


def _camera(Y, RG, A, K, cx, cy, delta):
    """the 28 terms of one camera over every quad: Y the point in the camera's frame, A = None (identity) or R21"""
    p = _mvv(K, Y)
    pix, piy = p[0] / p[2], p[1] / p[2]
    rx, ry = pix - cx, piy - cy
    rho = np.sqrt(np.add(rx * rx, ry * ry))
    valid = rho < math.inf
    small = rho <= delta
    w = np.where(small, 1.0, delta / rho)
    cost = np.where(small, (rho * rho) * 0.5, delta * (rho - delta * 0.5))
    ip = 1.0 / p[2]
    jx = [ip * (K[j] - pix * K[6 + j]) for j in range(3)]
    jy = [ip * (K[3 + j] - piy * K[6 + j]) for j in range(3)]
    if A is not None:                                        # row . R21: (j0 A0j + j1 A1j) + j2 A2j
        jx = [np.add(np.add(jx[0] * A[j], jx[1] * A[3 + j]), jx[2] * A[6 + j]) for j in range(3)]
        jy = [np.add(np.add(jy[0] * A[j], jy[1] * A[3 + j]), jy[2] * A[6 + j]) for j in range(3)]

    def cross(a, b):
        return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    Jx = cross(RG, jx) + jx                                  # m . [-[RG]x | I] = [RG x m | m]
    Jy = cross(RG, jy) + jy
    out = [w * np.add(Jx[i] * Jx[j], Jy[i] * Jy[j]) for i, j in UPPER]
    out += [w * np.add(Jx[i] * rx, Jy[i] * ry) for i in range(6)]
    out.append(cost)
    return [np.where(valid, v, 0.0) for v in out]


def quad_terms(R, t, G, u, ub, K, R21, T21, delta):
    """n x 28: the term of every quad under the pose (R 9 floats row-major, t 3 floats): left + right"""
    with np.errstate(all="ignore"):
        Gc = [G[:, 0], G[:, 1], G[:, 2]]
        RG = _mvv(R, Gc)
        X = [RG[i] + t[i] for i in range(3)]
        left = _camera(X, RG, None, K, u[:, 0], u[:, 1], delta)
        Y = _mvv(R21, X)
        Y = [Y[i] + T21[i] for i in range(3)]
        right = _camera(Y, RG, R21, K, ub[:, 0], ub[:, 1], delta)
        return np.stack([np.add(a, b) for a, b in zip(left, right)], axis=1)


def cholesky_solve(sums):
    """H d = -g from the 28 sums: pivots in order, + - x / sqrt only.  None when a pivot is not > 0."""
    H = [[0.0] * 6 for _ in range(6)]
    for k, (i, j) in enumerate(UPPER):
        H[i][j] = float(sums[k])
    b = [-float(sums[21 + i]) for i in range(6)]
    L = [[0.0] * 6 for _ in range(6)]
    for j in range(6):
        s = H[j][j]
        for k in range(j):
            s = s - L[j][k] * L[j][k]
        if not (s > 0):
            return None
        L[j][j] = math.sqrt(s)
        for i in range(j + 1, 6):
            s = H[j][i]
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            L[i][j] = op._div(s, L[j][j])
    y = [0.0] * 6
    for i in range(6):
        s = b[i]
        for k in range(i):
            s = s - L[i][k] * y[k]
        y[i] = op._div(s, L[i][i])
    d = [0.0] * 6
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * d[k]
        d[i] = op._div(s, L[i][i])
    return d


def exp_so3(w):
    """Exp(w), 9 floats row-major"""
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    I = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0]
    if th2 == 0:
        return I
    th = math.sqrt(th2)
    sn, _ = orc.sincos_v(np.array([th, th * 0.5]), orc.PORTABLE)
    a = op._div(float(sn[0]), th)
    sh = float(sn[1])
    b = op._div(2.0 * (sh * sh), th2)
    W = [0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0]
    W2 = _mm(W, W)
    return [(I[i] + a * W[i]) + b * W2[i] for i in range(9)]


def _mm(A, B):
    return [(A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j]) + A[i * 3 + 2] * B[6 + j] for i in range(3) for j in range(3)]


def refit(kf_left, kf_right, row_ptr, cf_left, cf_right, K_left, R21, T21, R0, t0, row_listed=None, kf_is_tp=None,
          max_reproj_error=1.5, **params):
    """The refit on host arrays.  Returns the fields of ebvo_pose_refined, R (3 x 3), t and `inlier` (full CSR order)."""
    p = dict(DEFAULTS, **params)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n_kf, n_full = len(row_ptr) - 1, int(row_ptr[-1])
    on = np.ones(n_kf, dtype=bool)
    if row_listed is not None:
        on &= np.asarray(row_listed).astype(bool)
    if kf_is_tp is not None:
        on &= np.asarray(kf_is_tp).astype(bool)
    sel = np.flatnonzero(np.repeat(on, np.diff(row_ptr)))    # selected quads in CSR order: k = position in sel
    n = len(sel)
    R = tuple(float(v) for v in np.asarray(R0, dtype=np.float64).reshape(9))
    t = tuple(float(v) for v in np.asarray(t0, dtype=np.float64).reshape(3))
    out = dict(status=0, stop_reason=STOP_FEW, rounds_run=0, steps_kept=0, n_quads=n, fit_quads=0, inliers=0, cost_first=0.0,
               cost_last=0.0, inlier=np.zeros(n_full, dtype=np.uint8))
    if n < 2:
        out.update(status=1, R=np.array(R).reshape(3, 3), t=np.array(t))
        return out
    K = tuple(op._kmat(K_left).reshape(9).tolist())
    R21 = tuple(np.asarray(R21, dtype=np.float64).reshape(9).tolist())
    T21 = tuple(np.asarray(T21, dtype=np.float64).reshape(3).tolist())
    geom = op.quad_geometry(kf_left, kf_right, row_ptr, cf_left, cf_right, K_left, R21, T21)
    G = np.ascontiguousarray(geom[sel, 0:3])
    cl, cr = np.asarray(cf_left)[sel], np.asarray(cf_right)[sel]
    u = np.stack([cl["x"], cl["y"]], axis=1).astype(np.float64)
    ub = np.stack([cr["x"], cr["y"]], axis=1).astype(np.float64)
    thr, delta, eps = float(max_reproj_error), float(p["huber_px"]), float(p["step_eps"])
    for rnd in range(p["rounds"]):
        out["rounds_run"] += 1
        S = op.inliers(R, t, G, u, K, thr)
        out["fit_quads"] = int(S.sum())
        if out["fit_quads"] < 3:
            out["stop_reason"] = STOP_FEW
            if rnd == 0:
                out["status"] = 1
            break
        Rp = tp = cost_prev = None
        for it in range(p["iterations"] + 1):
            terms = quad_terms(R, t, G, u, ub, K, R21, T21, delta)
            sums = virtual_lane_sums(np.where(S[:, None], terms, 0.0))
            cost = float(sums[27])
            if it == 0:
                out["cost_first"] = cost
            if it > 0 and not (cost <= cost_prev):
                R, t = Rp, tp
                out["steps_kept"] -= 1
                out["stop_reason"] = STOP_COST
                break
            out["cost_last"] = cost
            if it == p["iterations"]:
                out["stop_reason"] = STOP_CAP
                break
            d = cholesky_solve(sums)
            if d is None:
                out["stop_reason"] = STOP_PIVOT
                if rnd == 0 and it == 0:
                    out["status"] = 2
                break
            Rp, tp, cost_prev = R, t, cost
            R = tuple(_mm(exp_so3(d[0:3]), R))
            t = tuple(t[i] + d[3 + i] for i in range(3))
            out["steps_kept"] += 1
            m = 0.0
            for v in d:
                if abs(v) > m:
                    m = abs(v)
            if m < eps:
                out["stop_reason"] = STOP_EPS
                break
        if out["status"] == 2 or out["stop_reason"] == STOP_FEW:
            break
    mask = op.inliers(R, t, G, u, K, thr)
    out["inliers"] = int(mask.sum())
    out["inlier"][sel] = mask.astype(np.uint8)
    out.update(R=np.array(R).reshape(3, 3), t=np.array(t))
    return out


def pose_error(R, t, R_gt, t_gt):
    """independent statement of the pose-error metric (the host function under test is api.pose_error)"""
    E = np.asarray(R_gt, dtype=np.float64).reshape(3, 3).T @ np.asarray(R, dtype=np.float64).reshape(3, 3)
    v = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    rot = math.degrees(math.atan2(float(np.linalg.norm(v)) / 2.0, (float(np.trace(E)) - 1.0) / 2.0))
    t, t_gt = np.asarray(t, dtype=np.float64).reshape(3), np.asarray(t_gt, dtype=np.float64).reshape(3)
    na, nb = float(np.linalg.norm(t)), float(np.linalg.norm(t_gt))
    if na == 0 or nb == 0:
        ang = math.nan
    else:
        ang = math.degrees(math.atan2(float(np.linalg.norm(np.cross(t, t_gt))), float(t @ t_gt)))
    return dict(rot_deg=rot, trans_abs=float(np.linalg.norm(t - t_gt)), trans_dir_deg=ang)
