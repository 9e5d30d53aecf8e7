"""Oracle side of temporal matching under a pose prior (ebvo_temporal_set_prior, ebvo_tprior_candidates): this project's own
stage, not the reference's -- the search of a keyframe mate is centred on its projections through a predicted relative pose
in place of its own keyframe position.

Test infrastructure: the device is compared with THIS, bit for bit.  No new search code: the projections, the mapped
orientations and the camera-frame points are those of tests/oracle_tgt.py (the same helpers, the same operation order as
oracle_tgt.project), and the candidate stage IS orc.temporal_candidates on pseudo-keyframe edges whose (x, y, theta) are the
projections and the mapped orientations (the mate's own theta with use_orientation = 0), run on the live mates only; the
rows of the other mates are empty.  A live mate's coordinates are positive, so the C oracle's (int)x / cell is the device's.
Everything behind the candidate list is the unprimed chain with the REAL keyframe mates: orc.ncc_quads on their patches,
oracle_chain.temporal_edge_pairs.
"""
from __future__ import annotations

import numpy as np

from tests import oracle as orc
from tests import oracle_chain
from tests import oracle_tgt as ot
from tests import oracle_tstages as ots

DEFAULTS = dict(img_margin=0.0, use_orientation=1)


def project(kf_left, kf_right, R, t, calib, img_w, img_h, img_margin=0.0):
    """oracle_tgt.project plus the depth rule: live = in the image (strictly, both cameras against img_w x img_h; NaN and
    infinite coordinates are outside) and Gc.z > 0 and Gr.z > 0.  Returns live, proj_left / proj_right [n, 2],
    orient_left / orient_right, depth_left / depth_right."""
    p = ot.project(kf_left, kf_right, R, t, calib, img_w, img_h, None, img_margin)
    K_left, K_right, R21, T21 = calib
    S, Rm = ot._m(R21), ot._m(R)
    T21 = [float(v) for v in np.asarray(T21, dtype=np.float64).reshape(3)]
    tv = [float(v) for v in np.asarray(t, dtype=np.float64).reshape(3)]
    with np.errstate(all="ignore"):
        G = orc.finalize_pairs(K_left, K_right, R21, T21, kf_left, kf_right)[:, 6:9]
        Gc = ot._mv(Rm, G)
        Gc = np.stack([Gc[:, i] + tv[i] for i in range(3)], axis=1)
        Gr = ot._mv(S, Gc)
        Gr = np.stack([Gr[:, i] + T21[i] for i in range(3)], axis=1)
        live = (p["in_image"] != 0) & (Gc[:, 2] > 0.0) & (Gr[:, 2] > 0.0)
    return dict(live=live.astype(np.uint8), proj_left=p["proj_left"], proj_right=p["proj_right"], orient_left=p["orient_left"],
                orient_right=p["orient_right"], depth_left=Gc[:, 2].copy(), depth_right=Gr[:, 2].copy())


def pseudo_keyframe(kf_left, kf_right, proj, use_orientation=1):
    """keyframe edges moved to their projections (and, with use_orientation, turned to their mapped orientations)"""
    pL, pR = kf_left.copy(), kf_right.copy()
    pL["x"], pL["y"] = proj["proj_left"][:, 0], proj["proj_left"][:, 1]
    pR["x"], pR["y"] = proj["proj_right"][:, 0], proj["proj_right"][:, 1]
    if use_orientation:
        pL["theta"], pR["theta"] = proj["orient_left"], proj["orient_right"]
    return pL, pR


def _spread_rows(live_idx, rp_live, n_kf):
    cnt = np.zeros(n_kf, dtype=np.int64)
    cnt[live_idx] = np.diff(rp_live)
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.int32)


def candidates(kf_left, kf_right, cf_left, cf_right, R, t, calib, img_w, img_h, cell=15, radius=30.0, orient_thr_deg=10.0,
               img_margin=0.0, use_orientation=1):
    """the prior stage: dict(the arrays of `project`, row_ptr, col_idx)"""
    proj = project(kf_left, kf_right, R, t, calib, img_w, img_h, img_margin)
    pL, pR = pseudo_keyframe(kf_left, kf_right, proj, use_orientation)
    idx = np.flatnonzero(proj["live"])
    if len(idx) and len(cf_left):
        rp, ci = orc.temporal_candidates(pL[idx], pR[idx], cf_left, cf_right, img_w, img_h, cell, radius, orient_thr_deg)
    else:
        rp, ci = np.zeros(len(idx) + 1, dtype=np.int32), np.zeros(0, dtype=np.int32)
    return dict(proj, row_ptr=_spread_rows(idx, rp, len(kf_left)), col_idx=ci.astype(np.int32))


def reference(kfL, kfR, cfL, cfR, kf_imgs, cf_imgs, R, t, calib, w, h, chain=True, ncc_thr=0.8, cell=15, radius=30.0,
              orient_thr_deg=10.0, img_margin=0.0, use_orientation=1, **chain_kw):
    """oracle_chain.temporal_reference with the prior stage in place of its candidate stage (same keys; `prior` holds the
    arrays of ebvo_temporal_prior_fetch).  kf_imgs / cf_imgs = (raw left, undistorted left, undistorted right)."""
    c = candidates(kfL, kfR, cfL, cfR, R, t, calib, w, h, cell, radius, orient_thr_deg, img_margin, use_orientation)
    rp, ci = c["row_ptr"], c["col_idx"]
    pkL, pkR = orc.edge_patches(kf_imgs[0], kfL), orc.edge_patches(kf_imgs[2], kfR)
    pcL, pcR = orc.edge_patches(cf_imgs[0], cfL), orc.edge_patches(cf_imgs[2], cfR)
    rows = oracle_chain.rows_of(rp)
    sl, sr, keep = orc.ncc_quads(pkL[rows], pkR[rows], pcL[ci], pcR[ci], ncc_thr)
    ref = dict(row_ptr=rp, col_idx=ci, sim_left=sl, sim_right=sr, keep=keep, prior=c,
               counts=dict(n_kf=len(kfL), n_cf=len(cfL), n_candidates=len(ci), n_kept=int(keep.sum())))
    if chain:
        ref["final"] = oracle_chain.temporal_edge_pairs(kfL, kfR, cfL, cfR, kf_imgs[1:], cf_imgs[1:], rp, ci, sl, keep, **chain_kw)
        ref["counts"].update(ref["final"]["counts"])
    return ref


def grid_rows(kfL, kfR, cfL, cfR, prior, img_w, img_h, cell, radius, on, proj_left, proj_right, tp_dist=2.0):
    """the grid stage of a match made under a prior: oracle_tstages.grid_rows fed with the pseudo-keyframe, on the rows that
    are on AND live (a mate that is not live searched nothing: (0, 0))"""
    pL, pR = pseudo_keyframe(kfL, kfR, prior, 0)
    on_live = (np.asarray(on) != 0) & (prior["live"] != 0)
    # (the coordinates of the other rows are never read: they may be NaN)
    pL["x"][~on_live] = pL["y"][~on_live] = pR["x"][~on_live] = pR["y"][~on_live] = 0.0
    return ots.grid_rows(pL, pR, cfL, cfR, img_w, img_h, cell, radius, on_live, proj_left, proj_right, tp_dist)
