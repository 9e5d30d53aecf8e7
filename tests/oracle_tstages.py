"""Oracle-side stage trail of the temporal chain: oracle_chain.temporal_edge_pairs restated so that the list every stage
after the NCC filter leaves is kept, and the grid stage ("Location Proximity", the output of
apply_spatial_grid_filtering_quads, src/Temporal_Matches.cpp:335-383) evaluated row by row.

Test infrastructure: the device's trail (ebvo_temporal_keep_stages, ebvo_temporal_fetch_stage) and its evaluation of all
eight stages (ebvo_temporal_set_gt, ebvo_tgt_grid_rows) are compared with THIS, bit for bit.  The chain below makes the
same orc calls and the same selections as oracle_chain.temporal_edge_pairs; tests/test_tstages_oracle.py asserts that its
final list is that function's, so the two cannot drift apart.
"""
from __future__ import annotations

import numpy as np

from tests import oracle as orc
from tests import oracle_chain
from tests import oracle_tgt as ot
from tests.oracle_chain import _select_rows


def _flag_select(rp, flags, n_kf):
    """(row_ptr, source index) of the entries of CSR `rp` whose flag is set, order kept"""
    cnt = np.array([int(flags[rp[i]:rp[i + 1]].sum()) for i in range(n_kf)], dtype=np.int32)
    order = np.full(len(flags), -1, dtype=np.int32)
    for i in range(n_kf):
        k = np.flatnonzero(flags[rp[i]:rp[i + 1]]) + rp[i]
        order[rp[i]:rp[i] + len(k)] = k
    return _select_rows(rp, cnt, order)


def temporal_edge_pairs_trail(kfL, kfR, cfL, cfR, kf_imgs, cf_imgs, rp, ci, sim_left, keep, sift_thr=200.0, bnb_ncc=0.8,
                              bnb_sift=0.8, max_iter=20, tol=1e-3, huber=3.0):
    """(final, trail): `final` as oracle_chain.temporal_edge_pairs returns it; trail[stage] = dict(row_ptr, cf_index, left,
    right, moved) for SIFT, BNB_NCC, BNB_SIFT and REFINE -- left / right are the centres the evaluation reads (the mate's
    edges before the refinement), moved (the BNB stages) the number of positions whose quad is not the one the input order
    would have put there."""
    n_kf = len(kfL)
    dkL, dkR = orc.sift_descriptors(kf_imgs[0], kfL), orc.sift_descriptors(kf_imgs[1], kfR)
    dcL, dcR = orc.sift_descriptors(cf_imgs[0], cfL), orc.sift_descriptors(cf_imgs[1], cfR)
    rp0, idx = _flag_select(rp, np.asarray(keep) != 0, n_kf)
    cf, simL = ci[idx], sim_left[idx]
    counts, trail = {}, {}

    def record(stage, row_ptr, cf_idx, left=None, right=None, moved=0):
        trail[stage] = dict(row_ptr=np.asarray(row_ptr, dtype=np.int32), cf_index=cf_idx.astype(np.int32),
                            left=(cfL[cf_idx] if left is None else left).copy(), right=(cfR[cf_idx] if right is None else right).copy(),
                            moved=int(moved))

    # apply_SIFT_filtering_quads (:471-515)
    siftL, siftR = orc.sift_min_distances(dkL, dcL[cf], rp0), orc.sift_min_distances(dkR, dcR[cf], rp0)
    rp1, idx = _flag_select(rp0, (siftL < sift_thr) & (siftR < sift_thr), n_kf)
    cf, simL, siftL, siftR = cf[idx], simL[idx], siftL[idx], siftR[idx]
    counts["n_sift"] = len(cf)
    record(ot.SIFT, rp1, cf)
    # apply_best_nearly_best_filtering_quads on the NCC, then on the SIFT scores (:517-570)
    for stage, name, thr, scores_of, higher in ((ot.BNB_NCC, "n_bnb_ncc", bnb_ncc, lambda: simL, True),
                                                (ot.BNB_SIFT, "n_bnb_sift", bnb_sift, lambda: siftL, False)):
        c, o = orc.bnb_test(rp1, scores_of(), thr, higher, always_sorted=True)
        new_rp, idx = _select_rows(rp1, c, o)
        _, first = _select_rows(rp1, c, np.arange(len(cf), dtype=np.int32))      # the same counts in the input order
        rp1 = new_rp
        moved = int((idx != first).sum())
        cf, simL, siftL, siftR = cf[idx], simL[idx], siftL[idx], siftR[idx]
        counts[name] = len(cf)
        record(stage, rp1, cf, moved=moved)
    kf = np.repeat(np.arange(n_kf), np.diff(rp1))
    # apply_photometric_refinement_quads (:572-634)
    out, cen = {}, {}
    for cam, kE, cE, kimg, cimg in (("L", kfL, cfL, kf_imgs[0], cf_imgs[0]), ("R", kfR, cfR, kf_imgs[1], cf_imgs[1])):
        ke, ce = kE[kf], cE[cf]
        init = np.stack([ke["x"] - ce["x"], ke["y"] - ce["y"]], 1)
        r = orc.gn_refine_temporal(kimg, cimg, ke, ce, init, max_iter, tol, huber)
        c = ce.copy()
        v = r["validity"] == 1
        c["x"][v] = ke["x"][v] - r["disp"][v, 0]
        c["y"][v] = ke["y"][v] - r["disp"][v, 1]
        out[cam], cen[cam] = r, c
    valid = ((out["L"]["validity"] == 1) & (out["R"]["validity"] == 1)).astype(np.uint8)
    counts["n_refined_valid"] = int(valid.sum())
    record(ot.REFINE, rp1, cf, cen["L"], cen["R"])
    # apply_temporal_edge_clustering_quads (:636-733)
    ncl, centres, cluster_of = orc.cluster_rows(cen["L"], rp1, True, True)
    f_rows, f_src, f_L, f_R = [0], [], [], []
    for i in range(n_kf):
        b, n = rp1[i], rp1[i + 1] - rp1[i]
        if n < 2:
            for k in range(n):
                f_src.append(b)
                f_L.append(cen["L"][b])
                f_R.append(cen["R"][b])
            f_rows.append(len(f_src))
            continue
        loc = np.stack([cen["L"]["x"][b:b + n], cen["L"]["y"][b:b + n]], 1)
        for c in range(ncl[i]):
            members = [m for m in range(n) if cluster_of[b + m] == c]
            rights, best = [], -1
            for m in members:
                d = np.sqrt((loc[m, 0] - loc[:, 0]) * (loc[m, 0] - loc[:, 0]) + (loc[m, 1] - loc[:, 1]) * (loc[m, 1] - loc[:, 1]))
                closest = int(np.argmin(d))                              # the first smallest: `d < closest_dist`
                rights.append(cen["R"][b + closest])
                best = closest
            right = rights[0].copy()
            if len(rights) > 1:
                sx = sy = st = 0.0
                for e in rights:
                    sx += float(e["x"])
                    sy += float(e["y"])
                    st += float(e["theta"])
                right["x"], right["y"], right["theta"] = sx / len(rights), sy / len(rights), st / len(rights)
            f_src.append(b + best)
            f_L.append(centres[b + c])
            f_R.append(right)
        f_rows.append(len(f_src))
    f_src = np.array(f_src, dtype=np.int64)
    counts["n_final"] = len(f_src)
    final = dict(counts=counts, row_ptr=np.array(f_rows, dtype=np.int32), cf_index=cf[f_src].astype(np.int32),
                 left=np.array(f_L, dtype=orc.EDGE_DTYPE) if f_L else np.zeros(0, orc.EDGE_DTYPE),
                 right=np.array(f_R, dtype=orc.EDGE_DTYPE) if f_R else np.zeros(0, orc.EDGE_DTYPE), ncc_left=simL[f_src],
                 sift_left=siftL[f_src], score_left=out["L"]["score"][f_src], score_right=out["R"]["score"][f_src],
                 valid=valid[f_src])
    return final, trail


def same_final(a, b):
    """the final lists of temporal_edge_pairs_trail and of oracle_chain.temporal_edge_pairs, bit for bit"""
    return (a["counts"] == b["counts"] and
            all(oracle_chain._same(a[k], b[k]) for k in ("row_ptr", "cf_index", "ncc_left", "sift_left", "score_left", "score_right",
                                                         "valid")) and
            all(oracle_chain._same_edges(a[k], b[k]) for k in ("left", "right")))


class Grid(ot.SpatialGrid):
    """SpatialGrid queried with any coordinate: static_cast<int>(x) / cell_size truncates towards zero (include/Dataset.h:95-96),
    which Python's floor division only matches for x >= 0"""

    def within_radius(self, x, y, radius):
        if x >= 0 and y >= 0:
            return super().within_radius(x, y, radius)
        gx, gy = int(np.trunc(int(x) / self.cell)), int(np.trunc(int(y) / self.cell))
        sr = min(int(np.ceil(radius / self.cell)), self.gw + self.gh + abs(gx) + abs(gy))
        out = []
        for ny in range(max(0, gy - sr), min(self.gh - 1, gy + sr) + 1):       # dy outer, dx inner, clipped to the grid
            for nx in range(max(0, gx - sr), min(self.gw - 1, gx + sr) + 1):
                out.extend(self.cells[ny * self.gw + nx])
        return out


def grid_rows(kfL, kfR, cfL, cfR, img_w, img_h, cell, radius, on, proj_left, proj_right, tp_dist=2.0):
    """(n, tp) per keyframe mate of the grid stage: the quads of row i are left_candidates (the left grid around the mate's
    left edge) that are in right_set (the right grid around its right edge), :345-362; a quad is a true positive when both
    edges of its current-frame mate lie < tp_dist from the row's projections (:246-248).  Zero where the row is off."""
    gl, gr = Grid(cfL, img_w, img_h, cell), Grid(cfR, img_w, img_h, cell)
    lx, ly = (np.ascontiguousarray(cfL[f], dtype=np.float64) for f in ("x", "y"))
    rx, ry = (np.ascontiguousarray(cfR[f], dtype=np.float64) for f in ("x", "y"))
    n_tp = np.zeros((len(kfL), 2), dtype=np.int32)
    for i in np.flatnonzero(on):
        left_c = gl.within_radius(float(kfL["x"][i]), float(kfL["y"][i]), radius)
        right_set = set(gr.within_radius(float(kfR["x"][i]), float(kfR["y"][i]), radius))
        c = np.array([j for j in left_c if j in right_set], dtype=np.int64)
        if not len(c):
            continue
        with np.errstate(all="ignore"):
            dxl, dyl = lx[c] - proj_left[i, 0], ly[c] - proj_left[i, 1]
            dxr, dyr = rx[c] - proj_right[i, 0], ry[c] - proj_right[i, 1]
            hit = (np.sqrt(dxl * dxl + dyl * dyl) < tp_dist) & (np.sqrt(dxr * dxr + dyr * dyr) < tp_dist)
        n_tp[i] = (len(c), int(hit.sum()))
    return n_tp
