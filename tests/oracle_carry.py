"""CPU restatement of the handover of the refined depths to the next keyframe on promotion (ebvo_depth_carry /
ebvo_temporal_promote_keyframe) -- the checker of the device kernels (test infrastructure).  The contract is written once in
include/ebvo_hip.h; this file follows it operation by operation, one numpy ufunc per arithmetic operation (IEEE double, no
FMA).  Gamma per mate, the projection and the mapped orientation are tests/oracle_align.py's (tests/oracle_tgt.py::project on
Gamma / lambda, camera 0), the liveness of a mate and the prior are tests/oracle_depth.py's.

The association is stated over ALL live sources: a projection with d2 <= radius^2 lies in a cell within
ceil(radius / cell_size) of the new mate's cell (tests/oracle_align.py gives the argument), so the cell walk of the device
selects the same candidates; the pick is the smallest (d2, i).
"""
from __future__ import annotations

import math

import numpy as np

from tests import oracle as orc
from tests import oracle_align as oa
from tests import oracle_depth as od
from tests import oracle_tgt as ot

DEFAULTS = dict(sigma_disp_px=0.25, radius=1.5, cell_size=4, min_obs=1, orient_thr_deg=10.0, carry=0.5, gate_sigmas=3.0,
                lambda_min=0.25, lambda_max=4.0, info_max=1e6, img_margin=10.0)
DEAD, CARRIED, CARRY_GATED = od.DEAD, 32, 64
INT_FIELDS = ("n_old", "n_sources", "n_live", "n_new", "n_dead", "n_assoc", "n_carried", "n_gated")


def gamma(left, right, calib):
    """Gamma per mate as align_prepare_kernel forms it"""
    K_left, K_right, R21, T21 = calib
    with np.errstate(all="ignore"):
        fin = orc.finalize_pairs(oa.op._kmat(K_left), oa.op._kmat(K_right), R21, T21, left, right)
    return np.ascontiguousarray(fin[:, 6:9])


def sources(kf_left, kf_right, state, img_w, img_h, calib, R, t, p):
    """per old mate: source, live, q [n, 2], o, zp, a"""
    n = len(kf_left)
    lam, info = (np.asarray(v, dtype=np.float64) for v in state[:2])
    nobs = np.asarray(state[2], dtype=np.int32)
    G = gamma(kf_left, kf_right, calib)
    Rm = ot._m(np.asarray(R, dtype=np.float64).reshape(3, 3))
    tv = [float(v) for v in np.asarray(t, dtype=np.float64).reshape(3)]
    with np.errstate(all="ignore"):
        src = od.live_mates(G) & np.isfinite(lam) & (lam > 0.0) & (info > 0.0) & (nobs >= int(p["min_obs"]))
        Gs = np.stack([G[:, k] / lam for k in range(3)], axis=1)
        RG = ot._mv(Rm, Gs)
        X = np.stack([RG[:, k] + tv[k] for k in range(3)], axis=1)
        pr = ot.project(kf_left, kf_right, np.asarray(R).reshape(3, 3), np.asarray(t), calib, img_w, img_h, kf_gamma=Gs,
                        img_margin=p["img_margin"])
        q, o = pr["proj_left"], pr["orient_left"]
        zp = X[:, 2]
        a = RG[:, 2] / (zp * lam)
        m, x_max, y_max = float(p["img_margin"]), float(img_w) - float(p["img_margin"]), float(img_h) - float(p["img_margin"])
        live = src & (q[:, 0] > m) & (q[:, 1] > m) & (q[:, 0] < x_max) & (q[:, 1] < y_max) & (zp > 0.0)
    assert len(q) == n
    return dict(source=src, live=live, q=q, o=o, zp=zp, a=a, info=info, n_obs=nobs)


def carry(kf_left, kf_right, new_left, new_right, img_w, img_h, calib, R, t, state=None, **params):
    """The handover on host arrays.  state: None (nothing to carry) or the old mates' (lambda, info, n_obs).  Returns the fields
    of ebvo_depth_carried, lambda_, info, n_obs, flags, src_index of the new mates, and per new mate `lm`, `im` and `info0`
    (NaN where they were not formed)."""
    p = dict(DEFAULTS, **params)
    p.pop("reserved", None)
    kfL, kfR = (np.ascontiguousarray(v, dtype=orc.EDGE_DTYPE) for v in (kf_left, kf_right))
    nL, nR = (np.ascontiguousarray(v, dtype=orc.EDGE_DTYPE) for v in (new_left, new_right))
    calib = tuple(np.asarray(v, dtype=np.float64) for v in calib)
    n_old, n_new = len(kfL), len(nL)
    out = dict(n_old=n_old, n_sources=0, n_live=0, n_new=n_new, n_dead=0, n_assoc=0, n_carried=0, n_gated=0)
    nan = np.full(n_new, np.nan)
    if n_new == 0:
        out.update(lambda_=np.ones(0), info=np.zeros(0), n_obs=np.zeros(0, dtype=np.int32), flags=np.zeros(0, dtype=np.uint8),
                   src_index=np.zeros(0, dtype=np.int32), lm=nan, im=nan, info0=nan)
        return out
    K_left, _, _, T21 = calib
    Kl0 = float(oa.op._kmat(K_left).reshape(9)[0])
    T = [float(v) for v in T21.reshape(3)]
    G = gamma(nL, nR, calib)
    alive = od.live_mates(G)
    with np.errstate(all="ignore"):
        b = math.sqrt((T[0] * T[0] + T[1] * T[1]) + T[2] * T[2])
        s = (float(p["sigma_disp_px"]) * G[:, 2]) / (Kl0 * b)
        info0 = 1.0 / (s * s)
    src = np.full(n_new, -1, dtype=np.int32)
    S = None
    if state is not None and n_old > 0:
        S = sources(kfL, kfR, state, img_w, img_h, calib, R, t, p)
        out["n_sources"], out["n_live"] = int(S["source"].sum()), int(S["live"].sum())
        cell = int(p["cell_size"])
        # a source is a candidate only from inside a cell (every live source is: the margin is >= 0); so is the new mate
        in_cell = oa.in_cell(nL, img_w, img_h, cell)
        r2 = float(p["radius"]) * float(p["radius"])
        live_i = np.flatnonzero(S["live"])
        if len(live_i):
            order = live_i[np.argsort(S["q"][live_i, 0], kind="stable")]
            xs = S["q"][order, 0]
            mates = np.flatnonzero(alive & in_cell)
            lo = np.searchsorted(xs, nL["x"][mates] - (p["radius"] + 1.0), side="left")
            hi = np.searchsorted(xs, nL["x"][mates] + (p["radius"] + 1.0), side="right")
            cnt = hi - lo
            mi = np.repeat(np.arange(len(mates)), cnt)
            pos = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt) + np.repeat(lo, cnt)
            i, m = order[pos], mates[mi]
            with np.errstate(all="ignore"):
                dx, dy = S["q"][i, 0] - nL["x"][m], S["q"][i, 1] - nL["y"][m]
                d2 = np.add(dx * dx, dy * dy)
                keep = (d2 <= r2) & ot._orient_ok(S["o"][i], nL["theta"][m], float(p["orient_thr_deg"]))
            i, m, d2 = i[keep], m[keep], d2[keep]
            srt = np.lexsort((i, d2, m))                          # per new mate: ascending (d2, i)
            i, m = i[srt], m[srt]
            first = np.concatenate([[True], m[1:] != m[:-1]]) if len(m) else np.zeros(0, dtype=bool)
            src[m[first]] = i[first]
    has = src >= 0
    js = np.where(has, src, 0)
    lam, info, nobs = np.ones(n_new), np.where(alive, info0, 0.0), np.zeros(n_new, dtype=np.int32)
    flags = np.where(alive, 0, DEAD).astype(np.uint8)
    lm, im = nan.copy(), nan.copy()
    if S is not None and has.any():
        with np.errstate(all="ignore"):
            lm = G[:, 2] / S["zp"][js]
            c = lm * S["a"][js]
            im = (float(p["carry"]) * S["info"][js]) / (c * c)
            ok = np.isfinite(im) & (im > 0.0)
            d = lm - 1.0
            v = np.add(1.0 / info0, 1.0 / im)
            g2 = float(p["gate_sigmas"]) * float(p["gate_sigmas"])
            ok &= (lm >= float(p["lambda_min"])) & (lm <= float(p["lambda_max"])) & (d * d <= g2 * v)
            h = np.add(info0, im)
            lam_c = np.add(info0, im * lm) / h
            info_max = float(p["info_max"])
            info_c = np.where(h < info_max, h, info_max)
        acc, gated = has & ok, has & ~ok
        lam = np.where(acc, lam_c, lam)
        info = np.where(acc, info_c, info)
        nobs = np.where(acc, S["n_obs"][js], nobs).astype(np.int32)
        flags = (flags | np.where(acc, CARRIED, 0) | np.where(gated, CARRY_GATED, 0)).astype(np.uint8)
        lm, im = np.where(has, lm, np.nan), np.where(has, im, np.nan)
        out.update(n_assoc=int(has.sum()), n_carried=int(acc.sum()), n_gated=int(gated.sum()))
    out.update(n_dead=int((~alive).sum()), lambda_=lam, info=info, n_obs=nobs, flags=flags, src_index=src, lm=lm, im=im,
               info0=np.where(alive, info0, np.nan))
    return out
