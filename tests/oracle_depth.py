"""CPU restatement of the inverse-depth filter of the keyframe mates (ebvo_depth_refine_edges / ebvo_temporal_refine_depth) and
of the alignment on Gamma / lambda (ebvo_pose_align_edges_depth) -- the checker of the device kernels (test infrastructure).
The contract is written once in include/ebvo_hip.h; this file follows it operation by operation, one numpy ufunc per
arithmetic operation (IEEE double, no FMA).  Everything shared with the alignment -- Gamma per mate, the association, the tile
trees, sines and cosines -- is tests/oracle_align.py's.
"""
from __future__ import annotations

import math

import numpy as np

from tests import oracle as orc
from tests import oracle_align as oa
from tests import oracle_pose_refit as opr

DEFAULTS = dict(sigma_disp_px=0.25, sigma_normal_px=0.5, huber_px=1.0, gate_px=3.0, iterations=3, cameras=2, lambda_min=0.25,
                lambda_max=4.0, info_max=1e6, img_margin=10.0)
DEAD, UPDATED, RESTORED, GATED_LEFT, GATED_RIGHT = 1, 2, 4, 8, 16


def live_mates(G):
    with np.errstate(all="ignore"):
        return np.isfinite(G[:, 0]) & np.isfinite(G[:, 1]) & np.isfinite(G[:, 2]) & (G[:, 2] > 0.0)


def scaled_gamma(G, lambda_):
    """Gamma / lambda for the live mates (three divisions), Gamma itself for the dead ones: depth_scale_kernel"""
    lam = np.asarray(lambda_, dtype=np.float64)
    live = live_mates(G)
    with np.errstate(all="ignore"):
        return np.where(live[:, None], np.stack([G[:, k] / lam for k in range(3)], axis=1), G)


class DepthScene(oa.Scene):
    """oracle_align.Scene on Gamma / lambda"""

    def __init__(self, *a, lambda_=None):
        super().__init__(*a)
        self.G0 = self.G
        if lambda_ is not None:
            self.G = np.ascontiguousarray(scaled_gamma(self.G, lambda_))

    def associate(self, R, t):
        # Scene.associate projects through oracle_tgt.project, which forms Gamma itself unless it is handed one
        real = oa.ot.project
        oa.ot.project = lambda *a, **k: real(*a, kf_gamma=self.G, **k)
        try:
            return super().associate(R, t)
        finally:
            oa.ot.project = real


def align(kf_left, kf_right, lambda_, *a, **params):
    """oracle_align.align on Gamma / lambda (lambda_ = None: oracle_align.align itself)"""
    if lambda_ is None:
        return oa.align(kf_left, kf_right, *a, **params)
    real = oa.Scene
    oa.Scene = lambda *b: DepthScene(*b, lambda_=lambda_)
    try:
        return oa.align(kf_left, kf_right, *a, **params)
    finally:
        oa.Scene = real


def associate(kf_left, kf_right, lambda_, edges_left, edges_right, img_w, img_h, calib, R, t, **align_params):
    """the association ebvo_temporal_refine_depth makes: the alignment's, on Gamma / lambda"""
    p = dict(oa.DEFAULTS, **align_params)
    sc = DepthScene(kf_left, kf_right, edges_left, edges_right, img_w, img_h, calib, p, lambda_=lambda_)
    R = tuple(float(v) for v in np.asarray(R, dtype=np.float64).reshape(9))
    t = tuple(float(v) for v in np.asarray(t, dtype=np.float64).reshape(3))
    if sc.n == 0 or len(sc.E[0]) + len(sc.E[1]) == 0:
        return [np.full(sc.n, -1, dtype=np.int32) for _ in range(2)]
    return sc.associate(R, t)


def _term(c, K, R21, T21, R, t, G, lam, e):
    """one camera's r, j, pi_x, pi_y, Y_z over every mate at lambda (arrays)"""
    Gs = [G[:, k] / lam for k in range(3)]
    RG = opr._mvv(R, Gs)
    Y = [RG[k] + t[k] for k in range(3)]
    if c == 1:
        Y = opr._mvv(R21, Y)
        Y = [Y[k] + T21[k] for k in range(3)]
    p = opr._mvv(K, Y)
    pix, piy = p[0] / p[2], p[1] / p[2]
    r = np.add(e["n0"] * (pix - e["ex"]), e["n1"] * (piy - e["ey"]))
    ip = 1.0 / p[2]
    jx = [ip * (K[k] - pix * K[6 + k]) for k in range(3)]
    jy = [ip * (K[3 + k] - piy * K[6 + k]) for k in range(3)]
    if c == 1:                                               # mtv3(R21, .)
        jx = [np.add(np.add(R21[k] * jx[0], R21[3 + k] * jx[1]), R21[6 + k] * jx[2]) for k in range(3)]
        jy = [np.add(np.add(R21[k] * jy[0], R21[3 + k] * jy[1]), R21[6 + k] * jy[2]) for k in range(3)]
    m = [np.add(e["n0"] * jx[k], e["n1"] * jy[k]) for k in range(3)]
    d = np.add(np.add(m[0] * RG[0], m[1] * RG[1]), m[2] * RG[2])
    return r, -(d / lam), pix, piy, Y[2]


def _edge(E, assoc, n):
    """location and normal of the associated edge per mate; has: 0 <= a < len(E)"""
    if assoc is None:
        z = np.zeros(n)
        return dict(has=np.zeros(n, dtype=bool), ex=z, ey=z, n0=z, n1=z)
    a = np.asarray(assoc, dtype=np.int64)
    has = (a >= 0) & (a < len(E))
    ja = np.where(has, a, 0)
    if len(E):
        ex, ey, th = E["x"][ja], E["y"][ja], E["theta"][ja]
    else:
        ex = ey = th = np.zeros(n)
    sn, cs = orc.sincos_v(np.where(has, th, 0.0), orc.PORTABLE)
    return dict(has=has, ex=np.where(has, ex, 0.0), ey=np.where(has, ey, 0.0), n0=np.where(has, sn, 0.0), n1=np.where(has, -cs, 0.0))


def update(kf_left, kf_right, edges_left, edges_right, assoc_left, assoc_right, img_w, img_h, calib, R, t, state=None, **params):
    """One update on host arrays.  state: None (the prior) or (lambda, info, n_obs).  Returns the fields of ebvo_depth_refined
    and lambda_, info, n_obs, flags, plus `residual_in` (per camera: r at the incoming lambda, NaN without an edge)."""
    p = dict(DEFAULTS, **params)
    p.pop("block_threads", None)
    cams = p["cameras"]
    sc = oa.Scene(kf_left, kf_right, edges_left, edges_right if cams > 1 else None, img_w, img_h, calib,
                  dict(oa.DEFAULTS, cameras=cams))
    n, G = sc.n, sc.G
    out = dict(n_kf=n, n_dead=0, n_updated=0, n_restored=0, n_terms=(0, 0), n_gated=(0, 0), rms_before=0.0, rms_after=0.0)
    if n == 0:
        out.update(lambda_=np.ones(0), info=np.zeros(0), n_obs=np.zeros(0, dtype=np.int32), flags=np.zeros(0, dtype=np.uint8),
                   residual_in=[np.zeros(0), np.zeros(0)])
        return out
    R = tuple(float(v) for v in np.asarray(R, dtype=np.float64).reshape(9))
    t = tuple(float(v) for v in np.asarray(t, dtype=np.float64).reshape(3))
    K = (sc.Kl, sc.Kr)
    live = live_mates(G)
    with np.errstate(all="ignore"):
        if state is None:
            T = sc.T21
            b = math.sqrt((T[0] * T[0] + T[1] * T[1]) + T[2] * T[2])
            s = (float(p["sigma_disp_px"]) * G[:, 2]) / (sc.Kl[0] * b)
            l_in, f_in, o_in = np.ones(n), np.where(live, 1.0 / (s * s), 0.0), np.zeros(n, dtype=np.int32)
        else:
            l_in, f_in = (np.array(v, dtype=np.float64) for v in state[:2])
            o_in = np.array(state[2], dtype=np.int32)
        E = [_edge(sc.E[0], assoc_left, n), _edge(sc.E[1], assoc_right if cams > 1 else None, n)]
        m, x_max, y_max = float(p["img_margin"]), float(img_w) - float(p["img_margin"]), float(img_h) - float(p["img_margin"])
        gate, huber = float(p["gate_px"]), float(p["huber_px"])
        iv = 1.0 / (float(p["sigma_normal_px"]) * float(p["sigma_normal_px"]))
        lam = l_in.copy()
        surv, gated = [None, None], [None, None]
        for it in range(p["iterations"] + 1):
            ev = [_term(c, K[c], sc.R21, sc.T21, R, t, G, lam, E[c]) for c in range(2)]
            if it == 0:
                for c in range(2):
                    r, _, pix, piy, yz = ev[c]
                    alive = live & E[c]["has"] & (pix > m) & (piy > m) & (pix < x_max) & (piy < y_max) & (yz > 0.0)
                    rho = np.abs(r)
                    surv[c] = alive & (rho <= gate) & (rho < math.inf)
                    gated[c] = alive & ~surv[c]
                res_in = [np.where(E[c]["has"], ev[c][0], np.nan) for c in range(2)]
                sq_b = np.add(0.0, np.add(np.where(surv[0], ev[0][0] * ev[0][0], 0.0), np.where(surv[1], ev[1][0] * ev[1][0], 0.0)))
            Sh, Sg = np.zeros(n), np.zeros(n)
            for c in range(2):
                r, j = ev[c][0], ev[c][1]
                rho = np.abs(r)
                w = np.where(rho <= huber, 1.0, huber / rho)
                Sh = np.where(surv[c], np.add(Sh, w * (j * j)), Sh)
                Sg = np.where(surv[c], np.add(Sg, w * (j * r)), Sg)
            h = np.add(f_in, Sh * iv)
            if it == p["iterations"]:
                break
            g = np.add(f_in * (lam - l_in), Sg * iv)
            lam = lam - g / h
        any_term = surv[0] | surv[1]
        accept = live & np.isfinite(lam) & (lam >= float(p["lambda_min"])) & (lam <= float(p["lambda_max"])) & any_term & np.isfinite(h)
        restored = live & ~accept
        sq_a = np.add(0.0, np.add(np.where(surv[0], ev[0][0] * ev[0][0], 0.0), np.where(surv[1], ev[1][0] * ev[1][0], 0.0)))
        sq_a = np.where(accept, sq_a, sq_b)
        info_max = float(p["info_max"])
        lam_out = np.where(accept, lam, l_in)
        info_out = np.where(accept, np.where(h < info_max, h, info_max), f_in)
        nobs_out = np.where(accept, o_in + 1, o_in).astype(np.int32)
        flags = (np.where(live, 0, DEAD) | np.where(accept, UPDATED, 0) | np.where(restored, RESTORED, 0) |
                 np.where(gated[0], GATED_LEFT, 0) | np.where(gated[1], GATED_RIGHT, 0)).astype(np.uint8)
        sums = oa.tile_sums(np.stack([np.where(live, sq_b, 0.0), np.where(live, sq_a, 0.0)], axis=1))
    nt = (int(surv[0].sum()), int(surv[1].sum()))
    tot = nt[0] + nt[1]
    out.update(n_dead=int((~live).sum()), n_updated=int(accept.sum()), n_restored=int(restored.sum()), n_terms=nt,
               n_gated=(int(gated[0].sum()), int(gated[1].sum())),
               rms_before=math.sqrt(float(sums[0]) / float(tot)) if tot > 0 else 0.0,
               rms_after=math.sqrt(float(sums[1]) / float(tot)) if tot > 0 else 0.0,
               lambda_=lam_out, info=info_out, n_obs=nobs_out, flags=flags, residual_in=res_in)
    return out
