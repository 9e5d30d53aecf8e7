"""CPU restatement of the alignment of the pose to the current frame's TOED edges by normal distance (ebvo_pose_align_edges /
ebvo_temporal_align_pose) -- the checker of the device kernels (test infrastructure).  The contract is written once in
include/ebvo_hip.h; this file follows it operation by operation:

- the projections and mapped orientations are tests/oracle_tgt.py::project (the prior's projection, the TRUE K_right);
- the association is stated over ALL edges that are in a cell: an edge with d2 <= radius^2 lies in a cell within
  ceil(radius / cell_size) of the projection's cell (the difference of two truncated quotients never exceeds the ceiling of
  the quotient of the difference, and truncation towards zero only moves an edge of (-cell_size, 0) nearer), so the cell walk
  of the device selects the same candidates; the pick is the smallest (d2, j);
- the per-term arithmetic with one numpy ufunc per operation (IEEE double, no FMA);
- the tile sums are tests/oracle_pose_refit.py::virtual_lane_sums per tile of 1024 mates, the tiles added in ascending order;
- Cholesky, Exp and the loop are those of tests/oracle_pose_refit.py.
"""
from __future__ import annotations

import math

import numpy as np

from tests import oracle as orc
from tests import oracle_pose as op
from tests import oracle_pose_refit as opr
from tests import oracle_tgt as ot

TILE = 1024
DEFAULTS = dict(rounds=4, iterations=10, radius=4.0, cell_size=4, orient_thr_deg=10.0, huber_px=1.0, inlier_px=1.0,
                step_eps=1e-10, min_terms=12, img_margin=10.0, cameras=2)
STOP_EPS, STOP_CAP, STOP_COST, STOP_PIVOT, STOP_FEW = range(5)
UPPER = opr.UPPER


def in_cell(edges, img_w, img_h, cell):
    """the edges that are in a cell of the grid: (int)x / cell in [0, gw) and (int)y / cell in [0, gh), C division"""
    gw, gh = (img_w + cell - 1) // cell, (img_h + cell - 1) // cell
    x, y = np.asarray(edges["x"], dtype=np.float64), np.asarray(edges["y"], dtype=np.float64)
    with np.errstate(all="ignore"):
        return (x > -float(cell)) & (x < float(gw) * float(cell)) & (y > -float(cell)) & (y < float(gh) * float(cell))


def tile_sums(terms):
    """n x m per-mate terms -> the m sums: per tile of 1024 mates the lane trees, the tiles added in ascending order from +0.0"""
    terms = np.asarray(terms, dtype=np.float64)
    total = np.zeros(terms.shape[1])
    for b in range(0, len(terms), TILE):
        total = np.add(total, opr.virtual_lane_sums(terms[b:b + TILE]))
    return total


class Scene:
    """what does not depend on the pose: Gamma per mate, the edge lists and which of their edges are in a cell"""

    def __init__(self, kf_left, kf_right, edges_left, edges_right, img_w, img_h, calib, p):
        self.kfL = np.ascontiguousarray(kf_left, dtype=orc.EDGE_DTYPE)
        self.kfR = np.ascontiguousarray(kf_right, dtype=orc.EDGE_DTYPE)
        self.n = len(self.kfL)
        self.calib = tuple(np.asarray(v, dtype=np.float64) for v in calib)
        K_left, K_right, R21, T21 = self.calib
        self.Kl, self.Kr = (tuple(op._kmat(K).reshape(9).tolist()) for K in (K_left, K_right))
        self.R21, self.T21 = tuple(R21.reshape(9).tolist()), tuple(T21.reshape(3).tolist())
        self.w, self.h, self.p = int(img_w), int(img_h), p
        self.cams = p["cameras"]
        empty = np.zeros(0, dtype=orc.EDGE_DTYPE)
        lists = [edges_left, edges_right if self.cams > 1 and edges_right is not None else empty]
        self.E = [np.ascontiguousarray(e, dtype=orc.EDGE_DTYPE) for e in lists]
        self.ok = [in_cell(e, self.w, self.h, p["cell_size"]) for e in self.E]
        with np.errstate(all="ignore"):
            fin = orc.finalize_pairs(op._kmat(K_left), op._kmat(K_right), R21, T21, self.kfL, self.kfR)
        self.G = np.ascontiguousarray(fin[:, 6:9])

    def associate(self, R, t):
        """per camera: the edge index (or -1) of every mate under the pose"""
        p = self.p
        out = [np.full(self.n, -1, dtype=np.int32) for _ in range(2)]
        if self.n == 0:
            return out
        pr = ot.project(self.kfL, self.kfR, np.array(R).reshape(3, 3), np.array(t), self.calib, self.w, self.h,
                        img_margin=p["img_margin"])
        Rm, S = ot._m(np.array(R).reshape(3, 3)), ot._m(self.calib[2])
        m, x_max, y_max = float(p["img_margin"]), float(self.w) - float(p["img_margin"]), float(self.h) - float(p["img_margin"])
        r2 = float(p["radius"]) * float(p["radius"])
        with np.errstate(all="ignore"):
            Gc = ot._mv(Rm, self.G)
            Gc = np.stack([Gc[:, i] + float(t[i]) for i in range(3)], axis=1)
            Gr = ot._mv(S, Gc)
            Gr = np.stack([Gr[:, i] + self.T21[i] for i in range(3)], axis=1)
        for c in range(self.cams):
            E, ok = self.E[c], self.ok[c]
            if not len(E):
                continue
            q = pr["proj_left" if c == 0 else "proj_right"]
            o = pr["orient_left" if c == 0 else "orient_right"]
            z = (Gc if c == 0 else Gr)[:, 2]
            with np.errstate(all="ignore"):
                live = (q[:, 0] > m) & (q[:, 1] > m) & (q[:, 0] < x_max) & (q[:, 1] < y_max) & (z > 0.0)
            terms = np.flatnonzero(live)
            if not len(terms):
                continue
            # candidate (term, edge) pairs from a generous strip in x; every test of the contract is applied after it
            cand = np.flatnonzero(ok)
            order = cand[np.argsort(E["x"][cand], kind="stable")]
            xs = E["x"][order]
            lo = np.searchsorted(xs, q[terms, 0] - (p["radius"] + 1.0), side="left")
            hi = np.searchsorted(xs, q[terms, 0] + (p["radius"] + 1.0), side="right")
            cnt = hi - lo
            ti = np.repeat(np.arange(len(terms)), cnt)
            pos = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
            j = order[pos]
            i = terms[ti]
            with np.errstate(all="ignore"):
                dx, dy = E["x"][j] - q[i, 0], E["y"][j] - q[i, 1]
                d2 = np.add(dx * dx, dy * dy)
                keep = (d2 <= r2) & ot._orient_ok(o[i], E["theta"][j], float(p["orient_thr_deg"]))
            i, j, d2 = i[keep], j[keep], d2[keep]
            srt = np.lexsort((j, d2, i))                         # per mate: ascending (d2, j)
            i, j = i[srt], j[srt]
            first = np.concatenate([[True], i[1:] != i[:-1]]) if len(i) else np.zeros(0, dtype=bool)
            out[c][i[first]] = j[first]
        return out

    def _camera(self, c, R, t, assoc):
        """per mate: r, valid (associated and rho < +inf), w, cost and the six entries of the Jacobian row of camera c"""
        K = self.Kl if c == 0 else self.Kr
        E = self.E[c]
        a = assoc[c]
        has = a >= 0
        ja = np.where(has, a, 0)
        if len(E):
            ex, ey, th = E["x"][ja], E["y"][ja], E["theta"][ja]
        else:
            ex = ey = th = np.zeros(self.n)
        sn, cs = orc.sincos_v(np.where(has, th, 0.0), orc.PORTABLE)
        n0, n1 = sn, -cs
        Gc = [self.G[:, 0], self.G[:, 1], self.G[:, 2]]
        RG = opr._mvv(R, Gc)
        Y = [RG[i] + t[i] for i in range(3)]
        A = None
        if c == 1:
            Y = opr._mvv(self.R21, Y)
            Y = [Y[i] + self.T21[i] for i in range(3)]
            A = self.R21
        pp = opr._mvv(K, Y)
        pix, piy = pp[0] / pp[2], pp[1] / pp[2]
        r = np.add(n0 * (pix - ex), n1 * (piy - ey))
        rho = np.abs(r)
        valid = has & (rho < math.inf)
        ip = 1.0 / pp[2]
        jx = [ip * (K[k] - pix * K[6 + k]) for k in range(3)]
        jy = [ip * (K[3 + k] - piy * K[6 + k]) for k in range(3)]
        if A is not None:
            jx = [np.add(np.add(jx[0] * A[k], jx[1] * A[3 + k]), jx[2] * A[6 + k]) for k in range(3)]
            jy = [np.add(np.add(jy[0] * A[k], jy[1] * A[3 + k]), jy[2] * A[6 + k]) for k in range(3)]

        def cross(u, v):
            return [u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]]
        Jx, Jy = cross(RG, jx) + jx, cross(RG, jy) + jy
        J = [np.add(n0 * Jx[k], n1 * Jy[k]) for k in range(6)]
        return r, valid, rho, J

    def terms(self, R, t, assoc):
        """n x 28: camera 0 + camera 1 per mate"""
        delta = float(self.p["huber_px"])
        cams = []
        with np.errstate(all="ignore"):
            for c in range(2):
                if c >= self.cams:
                    cams.append([np.zeros(self.n)] * 28)
                    continue
                r, valid, rho, J = self._camera(c, R, t, assoc)
                small = rho <= delta
                w = np.where(small, 1.0, delta / rho)
                cost = np.where(small, (rho * rho) * 0.5, delta * (rho - delta * 0.5))
                out = [w * (J[i] * J[j]) for i, j in UPPER] + [w * (J[i] * r) for i in range(6)] + [cost]
                cams.append([np.where(valid, v, 0.0) for v in out])
            return np.stack([np.add(a, b) for a, b in zip(*cams)], axis=1)

    def metric(self, R, t, assoc):
        """(inliers, rms_normal, residuals per camera) of an association under the pose"""
        inl, sq, res = 0, [], []
        with np.errstate(all="ignore"):
            for c in range(2):
                if c >= self.cams:
                    sq.append(np.zeros(self.n))
                    res.append(np.full(self.n, np.nan))
                    continue
                r, valid, rho, _ = self._camera(c, R, t, assoc)
                inl += int((valid & (rho < float(self.p["inlier_px"]))).sum())
                sq.append(np.where(valid, r * r, 0.0))
                res.append(np.where(assoc[c] >= 0, r, np.nan))
            s = float(tile_sums(np.add(sq[0], sq[1])[:, None])[0])
        na = int((assoc[0] >= 0).sum() + (assoc[1] >= 0).sum())
        return inl, (math.sqrt(s / float(na)) if na > 0 else 0.0), res


def align(kf_left, kf_right, edges_left, edges_right, img_w, img_h, calib, R0, t0, **params):
    """The alignment on host arrays.  calib = (K_left, K_right, R21, T21).  Returns the fields of ebvo_aligned_pose, R (3 x 3),
    t, assoc_left / assoc_right, `residual` (per camera, NaN where not associated), `poses` (the pose after every round that formed its sums) and
    `round_log` ((stop reason, steps kept) of each of those rounds)."""
    p = dict(DEFAULTS, **params)
    p.pop("block_threads", None)
    sc = Scene(kf_left, kf_right, edges_left, edges_right, img_w, img_h, calib, p)
    R = tuple(float(v) for v in np.asarray(R0, dtype=np.float64).reshape(9))
    t = tuple(float(v) for v in np.asarray(t0, dtype=np.float64).reshape(3))
    n = sc.n
    out = dict(status=0, stop_reason=STOP_FEW, rounds_run=0, steps_kept=0, n_kf=n, fit_terms=0, n_assoc=(0, 0), inliers=0,
               cost_first=0.0, cost_last=0.0, rms_normal=0.0, poses=[], round_log=[])
    if n == 0 or len(sc.E[0]) + len(sc.E[1]) == 0:            # nothing launched
        none = np.full(n, -1, dtype=np.int32)
        out.update(status=1, R=np.array(R).reshape(3, 3), t=np.array(t), assoc_left=none, assoc_right=none.copy(),
                   residual=[np.full(n, np.nan)] * 2)
        return out
    eps = float(p["step_eps"])
    for rnd in range(p["rounds"]):
        assoc = sc.associate(R, t)
        out["rounds_run"] += 1
        out["fit_terms"] = int((assoc[0] >= 0).sum() + (assoc[1] >= 0).sum())
        if out["fit_terms"] < p["min_terms"]:
            out["stop_reason"] = STOP_FEW
            if rnd == 0:
                out["status"] = 1
            break
        Rp = tp = cost_prev = None
        steps_before = out["steps_kept"]
        for it in range(p["iterations"] + 1):
            sums = tile_sums(sc.terms(R, t, assoc))
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
            d = opr.cholesky_solve(sums)
            if d is None:
                out["stop_reason"] = STOP_PIVOT
                if rnd == 0 and it == 0:
                    out["status"] = 2
                break
            Rp, tp, cost_prev = R, t, cost
            R = tuple(opr._mm(opr.exp_so3(d[0:3]), R))
            t = tuple(t[i] + d[3 + i] for i in range(3))
            out["steps_kept"] += 1
            m = 0.0
            for v in d:
                if abs(v) > m:
                    m = abs(v)
            if m < eps:
                out["stop_reason"] = STOP_EPS
                break
        out["poses"].append((np.array(R).reshape(3, 3), np.array(t)))
        out["round_log"].append((out["stop_reason"], out["steps_kept"] - steps_before))
        if out["stop_reason"] in (STOP_PIVOT, STOP_FEW):
            break
    assoc = sc.associate(R, t)
    inl, rms, res = sc.metric(R, t, assoc)
    out.update(R=np.array(R).reshape(3, 3), t=np.array(t), assoc_left=assoc[0], assoc_right=assoc[1],
               n_assoc=(int((assoc[0] >= 0).sum()), int((assoc[1] >= 0).sum())), inliers=inl, rms_normal=rms, residual=res)
    return out
