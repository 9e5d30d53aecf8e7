"""Thin Python view of the C ABI, used by the tests and by bench.py.

The product's host side is C++ (include/ebvo/*.hpp adapters mirroring the reference classes);
this module only marshals numpy arrays to the same entry points, so that the parity tests read
like calls to the reference: ``get_Third_Order_Edges``, ``apply_NCC_Filtering`` ...
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _lib
from ._lib import EDGE_DTYPE, EbvoError, StereoCounts, StereoParams, ptr


def _u8(img: np.ndarray) -> np.ndarray:
    if img.dtype != np.uint8 or img.ndim != 2:
        raise TypeError("image must be a 2-D uint8 array (CV_8UC1)")
    if img.strides[1] != 1:
        img = np.ascontiguousarray(img)
    return img


def _edges(e: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(e, dtype=EDGE_DTYPE)


@dataclass
class ToedResult:
    edges: np.ndarray      # EDGE_DTYPE, toed_edges
    n_total: int           # Total_Num_Of_TOED
    all4: np.ndarray | None  # subpix_edge_pts_final rows (x, y, theta, mag)
    time_conv: float
    time_nms: float


class _CascadeRun(list):
    """one run of the constraint cascade: the list of its stage dicts, with the run's own fields as attributes"""

    def __init__(self, stages, **fields):
        super().__init__(stages)
        self.__dict__.update(fields)


def cascade_mean(runs) -> list:
    """Per-stage mean over the runs of pose_constraint_metrics as Print_Quad_Pairs_Metrics_Statistics forms it
    (src/MotionTracker.cpp:383-434): sums in run order divided by the run count.  One dict per stage of the first run: name,
    recall, precision, veridical (the mean number of surviving veridical quad pairs)."""
    out = []
    if not runs or not runs[0]:
        return out
    for ref in runs[0]:
        sum_recall, sum_precision, sum_veridical, count = 0.0, 0.0, 0, 0
        for run in runs:
            m = next((g for g in run if g["name"] == ref["name"]), None)
            if m is not None:
                sum_recall += m["recall"]
                sum_precision += m["precision"]
                sum_veridical += m["veridical"]
                count += 1
        if count:
            out.append(dict(name=ref["name"], recall=sum_recall / float(count), precision=sum_precision / float(count),
                            veridical=sum_veridical / float(count)))
    return out


def pose_error(R, t, R_gt, t_gt) -> dict:
    """Error of a relative pose against the true one (host arithmetic; the twin of ebvo::pose_error in adapters.hpp):
    rot_deg = the angle of E = R_gt^T R as atan2(|vee(E - E^T)| / 2, (tr E - 1) / 2) in degrees, trans_abs = |t - t_gt|,
    trans_dir_deg = the angle between t and t_gt in degrees (NaN when either is zero)."""
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    R_gt = np.asarray(R_gt, dtype=np.float64).reshape(3, 3)
    t = np.asarray(t, dtype=np.float64).reshape(3)
    t_gt = np.asarray(t_gt, dtype=np.float64).reshape(3)
    E = R_gt.T @ R
    vee = (E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1])
    s = math.sqrt(vee[0] * vee[0] + vee[1] * vee[1] + vee[2] * vee[2]) / 2.0
    c = (E[0, 0] + E[1, 1] + E[2, 2] - 1.0) / 2.0
    d = t - t_gt
    na, nb = math.sqrt(float(t @ t)), math.sqrt(float(t_gt @ t_gt))
    if na == 0.0 or nb == 0.0:
        direction = math.nan
    else:
        x = np.cross(t, t_gt)
        direction = math.degrees(math.atan2(math.sqrt(float(x @ x)), float(t @ t_gt)))
    return dict(rot_deg=math.degrees(math.atan2(s, c)), trans_abs=math.sqrt(float(d @ d)), trans_dir_deg=direction)


def predict_pose(T_prev, T_prev2=None):
    """Constant-velocity prediction of the next pose keyframe -> frame, for Context.temporal_set_prior (host arithmetic; the
    twin of ebvo::predict_pose in adapters.hpp).  T_prev = (R, t) of frame k, T_prev2 = (R, t) of frame k - 1, both
    keyframe -> frame: the motion of the last step, T_k T_{k-1}^-1, is applied once more to T_k.  With one earlier pose only
    (T_prev2 None) the prediction is that pose itself.  Returns (R [3, 3], t [3])."""
    Rk = np.asarray(T_prev[0], dtype=np.float64).reshape(3, 3)
    tk = np.asarray(T_prev[1], dtype=np.float64).reshape(3)
    if T_prev2 is None:
        return Rk.copy(), tk.copy()
    Rj = np.asarray(T_prev2[0], dtype=np.float64).reshape(3, 3)
    tj = np.asarray(T_prev2[1], dtype=np.float64).reshape(3)
    Rd = Rk @ Rj.T                      # T_k T_{k-1}^-1 = (Rd, tk - Rd tj)
    td = tk - Rd @ tj
    return Rd @ Rk, Rd @ tk + td


class Context:
    """One HIP device workspace (``ebvo_ctx``).  Not thread-safe; one per process and GPU."""

    def __init__(self, max_h: int, max_w: int, device: int = 0, toed_mode: str | None = None):
        self.lib = _lib.load_library()
        self._ctx = C.c_void_p()
        rc = self.lib.ebvo_ctx_create(device, max_h, max_w, C.byref(self._ctx))
        if rc != 0:
            raise EbvoError(rc, "ebvo_ctx_create", self.lib.ebvo_strerror(rc).decode())
        self.max_h, self.max_w, self.device = max_h, max_w, device
        self._tq_n_kf = {}      # slot -> keyframe mates of its completed temporal match (temporal_set_gt sizes its arrays by it)
        if toed_mode is not None:
            self.set_toed_mode(toed_mode)

    def set_toed_mode(self, mode: str):
        """'strict': direct-form convolution everywhere; 'hybrid': separable screen + exact re-evaluation."""
        m = {"strict": _lib.TOED_STRICT, "hybrid": _lib.TOED_HYBRID}[mode]
        self._check(self.lib.ebvo_set_toed_mode(self._ctx, m), "ebvo_set_toed_mode")

    def toed_stats(self, slot: int = 0) -> dict:
        out = np.zeros(8, dtype=np.int32)
        self._check(self.lib.ebvo_toed_stats(self._ctx, slot, ptr(out)), "ebvo_toed_stats")
        return {"left": dict(n_total=int(out[0]), n_kept=int(out[1]), n_candidates=int(out[2]), n_neighbour_points=int(out[3])),
                "right": dict(n_total=int(out[4]), n_kept=int(out[5]), n_candidates=int(out[6]),
                              n_neighbour_points=int(out[7]))}

    def toed_screen_audit(self, img: np.ndarray) -> dict:
        """ebvo_toed_screen_audit: max |screen - exact| of the hybrid detector's FP32 screen on this image, with its budget."""
        img = _u8(img)
        h, w = img.shape
        a = _lib.ScreenAudit()
        self._check(self.lib.ebvo_toed_screen_audit(self._ctx, ptr(img), h, w, img.strides[0], C.byref(a)),
                    "ebvo_toed_screen_audit")
        return {name: getattr(a, name) for name, _ in a._fields_}

    @property
    def toed_fallbacks(self) -> int:
        """Hybrid TOED runs the library repeated on the strict path (screened candidates > max_h * max_w)."""
        return int(self.lib.ebvo_toed_fallbacks(self._ctx))

    @property
    def graph_launches(self) -> int:
        """Pairs that ebvo_stereo_submit launched as a captured hipGraph."""
        return int(self.lib.ebvo_graph_launches(self._ctx))

    @property
    def toed_mode(self) -> str:
        return "hybrid" if self.lib.ebvo_get_toed_mode(self._ctx) == _lib.TOED_HYBRID else "strict"

    def close(self):
        if getattr(self, "_ctx", None):
            self.lib.ebvo_ctx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _check(self, rc: int, where: str):
        if rc != 0:
            raise EbvoError(rc, where, self.lib.ebvo_strerror(rc).decode() + "; " +
                            self.lib.ebvo_last_error(self._ctx).decode())

    # -- ThirdOrderEdgeDetectionCPU::get_Third_Order_Edges ---------------------------------
    def toed(self, img: np.ndarray, want_all: bool = False, cap: int | None = None) -> ToedResult:
        img = _u8(img)
        h, w = img.shape
        cap = h * w if cap is None else cap
        out = np.zeros(cap, dtype=EDGE_DTYPE)
        all4 = np.zeros((cap, 4), dtype=np.float64) if want_all else None
        nk, nt = C.c_int(), C.c_int()
        tc, tn = C.c_double(), C.c_double()
        rc = self.lib.ebvo_toed(self._ctx, ptr(img), h, w, img.strides[0], ptr(out), cap, C.byref(nk),
                                C.byref(nt), ptr(all4), cap if want_all else 0, C.byref(tc), C.byref(tn))
        if rc == _lib.EBVO_ERR_CAPACITY:
            raise EbvoError(rc, f"ebvo_toed (need kept={nk.value}, total={nt.value})")
        self._check(rc, "ebvo_toed")
        return ToedResult(out[: nk.value].copy(), nt.value,
                          all4[: nt.value].copy() if want_all else None, tc.value, tn.value)

    def toed_pair(self, left: np.ndarray, right: np.ndarray):
        left, right = _u8(left), _u8(right)
        h, w = left.shape
        assert right.shape == (h, w)
        cap = h * w
        ol, orr = np.zeros(cap, dtype=EDGE_DTYPE), np.zeros(cap, dtype=EDGE_DTYPE)
        nk, nt = (C.c_int * 2)(), (C.c_int * 2)()
        rc = self.lib.ebvo_toed_pair(self._ctx, ptr(left), ptr(right), h, w, left.strides[0], right.strides[0],
                                     ptr(ol), ptr(orr), cap, nk, nt)
        self._check(rc, "ebvo_toed_pair")
        return ol[: nk[0]].copy(), orr[: nk[1]].copy(), (nt[0], nt[1])

    # -- Stereo_Matches::CalculateEpipolarLine ----------------------------------------------
    def epipolar_lines(self, F: np.ndarray, edges: np.ndarray) -> np.ndarray:
        F = np.ascontiguousarray(F, dtype=np.float64).reshape(9)
        edges = _edges(edges)
        lines = np.zeros((len(edges), 3), dtype=np.float64)
        self._check(self.lib.ebvo_epipolar_lines(ptr(F), ptr(edges), len(edges), ptr(lines)), "ebvo_epipolar_lines")
        return lines

    # -- apply_Epipolar_Line_Distance_Filtering / Disparity / orientation -------------------
    def epi_candidates(self, L, R, lines, epi_thr=0.5, max_disp=25.0, orient_thr_deg=10.0,
                       stage_mask=_lib.STAGE_ALL):
        L, R = _edges(L), _edges(R)
        lines = np.ascontiguousarray(lines, dtype=np.float64).reshape(-1, 3)
        assert len(lines) == len(L)
        row_ptr = np.zeros(len(L) + 1, dtype=np.int32)
        n = C.c_int64()
        rc = self.lib.ebvo_epi_candidates(self._ctx, ptr(L), len(L), ptr(R), len(R), ptr(lines), epi_thr, max_disp,
                                          orient_thr_deg, stage_mask, ptr(row_ptr), None, 0, C.byref(n))
        self._check(rc, "ebvo_epi_candidates(size)")
        col = np.zeros(max(1, n.value), dtype=np.int32)
        rc = self.lib.ebvo_epi_candidates(self._ctx, ptr(L), len(L), ptr(R), len(R), ptr(lines), epi_thr, max_disp,
                                          orient_thr_deg, stage_mask, ptr(row_ptr), ptr(col), len(col), C.byref(n))
        self._check(rc, "ebvo_epi_candidates")
        return row_ptr, col[: n.value].copy()

    def epi_candidates_staged(self, L, R, lines, epi_thr=0.5, max_disp=25.0, orient_thr_deg=10.0):
        """One search for the three geometric stages: the (epipolar AND disparity) list + the orientation flag of every
        listed pair.  One call: the list is sized generously first and fetched again only if it did not fit."""
        L, R = _edges(L), _edges(R)
        lines = np.ascontiguousarray(lines, dtype=np.float64).reshape(-1, 3)
        assert len(lines) == len(L)
        row_ptr = np.zeros(len(L) + 1, dtype=np.int32)
        n = C.c_int64()
        cap = max(1024, 24 * len(L))
        for _ in range(2):
            col, ok = np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.uint8)
            rc = self.lib.ebvo_epi_candidates_staged(self._ctx, ptr(L), len(L), ptr(R), len(R), ptr(lines), epi_thr, max_disp,
                                                     orient_thr_deg, ptr(row_ptr), ptr(col), ptr(ok), cap, C.byref(n))
            if rc != _lib.EBVO_ERR_CAPACITY:
                break
            cap = int(n.value)
        self._check(rc, "ebvo_epi_candidates_staged")
        return row_ptr, col[: n.value].copy(), ok[: n.value].copy()

    # -- Stereo_Matches::apply_NCC_Filtering --------------------------------------------------
    def ncc_pairs(self, imgL, imgR, L, Rc, row_ptr, thr=0.6, want_left_patches=False):
        imgL, imgR = _u8(imgL), _u8(imgR)
        h, w = imgL.shape
        L, Rc = _edges(L), _edges(Rc)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        npairs = int(row_ptr[-1]) if len(row_ptr) else 0
        assert len(Rc) == npairs
        sims = np.zeros((npairs, 4), dtype=np.float64)
        best = np.zeros(npairs, dtype=np.float64)
        keep = np.zeros(npairs, dtype=np.uint8)
        lp = np.zeros((len(L), 2, 49), dtype=np.float32) if want_left_patches else None
        rc = self.lib.ebvo_ncc_pairs(self._ctx, ptr(imgL), ptr(imgR), h, w, imgL.strides[0], imgR.strides[0], ptr(L),
                                     len(L), ptr(Rc), ptr(row_ptr), thr, ptr(lp), ptr(sims), ptr(best), ptr(keep))
        self._check(rc, "ebvo_ncc_pairs")
        return sims, best, keep, lp

    # -- the resident stage-wise calls (what a stage produced stays on the device under a tag) ------------------------
    @staticmethod
    def _view(ptr_, count, dtype):
        """copy of `count` items of `dtype` at a page-locked address the library returned"""
        if not ptr_ or count == 0:
            return np.zeros(0, dtype=dtype)
        buf = (C.c_ubyte * (int(count) * np.dtype(dtype).itemsize)).from_address(ptr_)
        return np.frombuffer(buf, dtype=dtype, count=int(count)).copy()

    def toed_resident(self, img: np.ndarray, which: int, want_all: bool = False):
        """ebvo_toed_resident: (edges, n_total, all4 or None, tag)"""
        img = _u8(img)
        h, w = img.shape
        v = _lib.ToedView()
        self._check(self.lib.ebvo_toed_resident(self._ctx, which, ptr(img), h, w, img.strides[0], int(want_all), C.byref(v)),
                    "ebvo_toed_resident")
        all4 = self._view(v.all4, v.n_total * 4, np.float64).reshape(-1, 4) if want_all else None
        return self._view(v.edges, v.n_kept, EDGE_DTYPE), v.n_total, all4, int(v.tag)

    def epi_candidates_resident(self, tag_left, tag_right, lines, epi_thr=0.5, max_disp=25.0, orient_thr_deg=10.0,
                                stage_mask=_lib.STAGE_ALL, staged=False):
        """ebvo_epi_candidates_resident: (row_ptr, col_idx[, orient_ok]); staged = the (epipolar AND disparity) list + flags"""
        lines = np.ascontiguousarray(lines, dtype=np.float64).reshape(-1, 3)
        v = _lib.CandidatesView()
        mask = (_lib.STAGE_EPIPOLAR | _lib.STAGE_DISPARITY) if staged else stage_mask
        self._check(self.lib.ebvo_epi_candidates_resident(self._ctx, tag_left, tag_right, ptr(lines), epi_thr, max_disp,
                                                          orient_thr_deg, mask, int(staged), C.byref(v)),
                    "ebvo_epi_candidates_resident")
        rp = self._view(v.row_ptr, len(lines) + 1, np.int32)
        ci = self._view(v.col_idx, v.n_pairs, np.int32)
        if not staged:
            return rp, ci
        # the list the flags select (after apply_orientation_filter), formed on the device as well
        self.last_final_lists = (self._view(v.row_ptr_final, len(lines) + 1, np.int32), self._view(v.col_idx_final, v.n_final, np.int32))
        return rp, ci, self._view(v.orient_ok, v.n_pairs, np.uint8)

    def ncc_pairs_resident(self, tag_left, tag_right, imgL, imgR, row_ptr, col_idx, thr=0.6, want_left_patches=False,
                           want_sims=True):
        """ebvo_ncc_pairs_resident: (sims or None, best, keep, left_patches or None)"""
        imgL, imgR = _u8(imgL), _u8(imgR)
        h, w = imgL.shape
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        col_idx = np.ascontiguousarray(col_idx, dtype=np.int32)
        want = (_lib.NCC_WANT_LEFT_PATCHES if want_left_patches else 0) | (_lib.NCC_WANT_SIMS if want_sims else 0)
        v = _lib.NccView()
        self._check(self.lib.ebvo_ncc_pairs_resident(self._ctx, tag_left, tag_right, ptr(imgL), ptr(imgR), h, w, imgL.strides[0],
                                                     imgR.strides[0], ptr(row_ptr), ptr(col_idx), thr, want, C.byref(v)),
                    "ebvo_ncc_pairs_resident")
        sims = self._view(v.sims, v.n_pairs * 4, np.float64).reshape(-1, 4) if want_sims else None
        lp = self._view(v.left_patches, v.n_left * 98, np.float32).reshape(-1, 2, 49) if want_left_patches else None
        return sims, self._view(v.best, v.n_pairs, np.float64), self._view(v.keep, v.n_pairs, np.uint8), lp

    # -- cv::undistort (src/Pipeline.cpp:78-79) ---------------------------------------------------------
    def undistort(self, img, K, dist):
        img = _u8(img)
        h, w = img.shape
        K = np.ascontiguousarray(K, dtype=np.float64).reshape(4)
        dist = np.ascontiguousarray(dist, dtype=np.float64).reshape(-1)
        out = np.zeros((h, w), dtype=np.uint8)
        self._check(self.lib.ebvo_undistort(self._ctx, ptr(img), h, w, img.strides[0], ptr(K), ptr(dist), len(dist), ptr(out),
                                            out.strides[0]), "ebvo_undistort")
        return out

    def set_undistort(self, K_left=None, dist_left=None, K_right=None, dist_right=None):
        """Resident pipeline: undistort the uploaded pair (TOED / refinement on the result, NCC on the raw images).
        No arguments: off."""
        if K_left is None:
            self._check(self.lib.ebvo_stereo_set_undistort(self._ctx, None), "ebvo_stereo_set_undistort")
            return
        p = _lib.UndistortParams()
        n = len(dist_left)
        assert len(dist_right) == n and n in (4, 5)
        for k in range(4):
            p.K_left[k], p.K_right[k] = float(K_left[k]), float(K_right[k])
        for k in range(n):
            p.dist_left[k], p.dist_right[k] = float(dist_left[k]), float(dist_right[k])
        p.n_dist = n
        self._check(self.lib.ebvo_stereo_set_undistort(self._ctx, C.byref(p)), "ebvo_stereo_set_undistort")

    # -- util_compute_Img_Gradients (include/utility.h:131-141) -----------------------------------
    def sobel_gradients(self, img):
        img = _u8(img)
        h, w = img.shape
        gx = np.zeros((h, w), dtype=np.float32)
        gy = np.zeros((h, w), dtype=np.float32)
        self._check(self.lib.ebvo_sobel_gradients(self._ctx, ptr(img), h, w, img.strides[0], ptr(gx), ptr(gy)),
                    "ebvo_sobel_gradients")
        return gx, gy

    # -- Stereo_Matches::refine_edge_disparity (src/Stereo_Matches.cpp:1290-1358) ----------------
    def gn_refine_stereo(self, imgL, imgR, L, lines, row_ptr, cand_xy, max_iter=None, tol=None, huber_delta=None):
        """Photometric Gauss-Newton refinement of every (left edge, candidate) pair along the epipolar line.
        Returns dict(alpha, score, confidence, validity, iters, refined_xy)."""
        from ._lib import GnParams
        imgL, imgR = _u8(imgL), _u8(imgR)
        h, w = imgL.shape
        L = _edges(L)
        lines = np.ascontiguousarray(lines, dtype=np.float64).reshape(-1, 3)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        cand_xy = np.ascontiguousarray(cand_xy, dtype=np.float64).reshape(-1, 2)
        n = int(row_ptr[-1]) if len(row_ptr) else 0
        assert len(cand_xy) == n and len(lines) == len(L) and len(row_ptr) == len(L) + 1
        p = GnParams()
        self.lib.ebvo_gn_default_params(p)
        if max_iter is not None:
            p.max_iter = int(max_iter)
        if tol is not None:
            p.tol = float(tol)
        if huber_delta is not None:
            p.huber_delta = float(huber_delta)
        out = dict(alpha=np.zeros(n), score=np.zeros(n), confidence=np.zeros(n), validity=np.zeros(n, dtype=np.uint8),
                   iters=np.zeros(n, dtype=np.int32), refined_xy=np.zeros((n, 2)))
        rc = self.lib.ebvo_gn_refine_stereo(self._ctx, ptr(imgL), ptr(imgR), h, w, imgL.strides[0], imgR.strides[0],
                                            ptr(L), len(L), ptr(lines), ptr(row_ptr), ptr(cand_xy), C.byref(p),
                                            ptr(out["alpha"]), ptr(out["score"]), ptr(out["confidence"]),
                                            ptr(out["validity"]), ptr(out["iters"]), ptr(out["refined_xy"]))
        self._check(rc, "ebvo_gn_refine_stereo")
        return out

    def _gn_params(self, max_iter=None, tol=None, huber_delta=None):
        from ._lib import GnParams
        p = GnParams()
        self.lib.ebvo_gn_default_params(p)
        if max_iter is not None:
            p.max_iter = int(max_iter)
        if tol is not None:
            p.tol = float(tol)
        if huber_delta is not None:
            p.huber_delta = float(huber_delta)
        return p

    # -- Temporal_Matches::min_Edge_Photometric_Residual_by_Gauss_Newton (src/Temporal_Matches.cpp:735-851) ------
    def gn_refine_temporal(self, imgKF, imgCF, kf, cf, init_disp, **kw):
        imgKF, imgCF = _u8(imgKF), _u8(imgCF)
        h, w = imgKF.shape
        kf, cf = _edges(kf), _edges(cf)
        init_disp = np.ascontiguousarray(init_disp, dtype=np.float64).reshape(-1, 2)
        n = len(kf)
        assert len(cf) == n and len(init_disp) == n
        p = self._gn_params(**kw)
        out = dict(disp=np.zeros((n, 2)), score=np.zeros(n), validity=np.zeros(n, dtype=np.uint8),
                   iters=np.zeros(n, dtype=np.int32))
        rc = self.lib.ebvo_gn_refine_temporal(self._ctx, ptr(imgKF), ptr(imgCF), h, w, imgKF.strides[0], imgCF.strides[0],
                                              ptr(kf), ptr(cf), ptr(init_disp), n, C.byref(p), ptr(out["disp"]),
                                              ptr(out["score"]), ptr(out["validity"]), ptr(out["iters"]))
        self._check(rc, "ebvo_gn_refine_temporal")
        return out

    # -- stage glue: apply_Best_Nearly_Best_Test / apply_Lowe_Ratio_Test / shift_Edge_to_Epipolar_Line ---------------
    def bnb_test(self, row_ptr, scores, ratio_thr, higher_is_better=True):
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        nL = len(row_ptr) - 1
        cnt = np.zeros(nL, dtype=np.int32)
        order = np.full(len(scores), -1, dtype=np.int32)
        self._check(self.lib.ebvo_bnb_test(self._ctx, ptr(row_ptr), nL, ptr(scores), ratio_thr, int(higher_is_better),
                                           ptr(cnt), ptr(order)), "ebvo_bnb_test")
        return cnt, order

    def keep_best(self, row_ptr, scores):
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        scores = np.ascontiguousarray(scores, dtype=np.float64)
        nL = len(row_ptr) - 1
        cnt = np.zeros(nL, dtype=np.int32)
        order = np.full(len(scores), -1, dtype=np.int32)
        self._check(self.lib.ebvo_keep_best(self._ctx, ptr(row_ptr), nL, ptr(scores), ptr(cnt), ptr(order)),
                    "ebvo_keep_best")
        return cnt, order

    def epipolar_shift(self, cand, lines, row_ptr):
        cand = _edges(cand)
        lines = np.ascontiguousarray(lines, dtype=np.float64).reshape(-1, 3)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        out = np.zeros(len(cand), dtype=EDGE_DTYPE)
        self._check(self.lib.ebvo_epipolar_shift(self._ctx, ptr(cand), ptr(lines), ptr(row_ptr), len(row_ptr) - 1,
                                                 ptr(out)), "ebvo_epipolar_shift")
        return out

    def cluster_rows(self, cand, row_ptr, by_orientation=False, skip_single=True):
        """EdgeClusterer per row: (new_count, centres, cluster_of)."""
        cand = _edges(cand)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        nL = len(row_ptr) - 1
        cnt = np.zeros(nL, dtype=np.int32)
        centres = np.zeros(len(cand), dtype=EDGE_DTYPE)
        cluster_of = np.full(len(cand), -1, dtype=np.int32)
        self._check(self.lib.ebvo_cluster_rows(self._ctx, ptr(cand), ptr(row_ptr), nL, int(by_orientation), int(skip_single),
                                               ptr(cnt), ptr(centres), ptr(cluster_of)), "ebvo_cluster_rows")
        return cnt, centres, cluster_of

    # -- write_finalized_stereo_edge_pairs_to_file, numeric body (src/Stereo_Matches.cpp:1656-1699) -----------------
    def finalize_pairs(self, K_left, K_right, R21, T21, left, right) -> np.ndarray:
        cal = self._calib((K_left, K_right, R21, T21))
        left, right = _edges(left), _edges(right)
        assert len(left) == len(right)
        out = np.zeros((len(left), 16))
        self._check(self.lib.ebvo_finalize_pairs(self._ctx, C.byref(cal), ptr(left), ptr(right), len(left), ptr(out)),
                    "ebvo_finalize_pairs")
        return out

    # -- cv::SIFT::compute at the +-8 px points of every edge / apply_SIFT_filtering's score ---------------------------
    def sift_descriptors(self, img, edges) -> np.ndarray:
        img = _u8(img)
        h, w = img.shape
        edges = _edges(edges)
        out = np.zeros((len(edges), 2, 128), dtype=np.float32)
        self._check(self.lib.ebvo_sift_descriptors(self._ctx, ptr(img), h, w, img.strides[0], ptr(edges), len(edges), ptr(out)),
                    "ebvo_sift_descriptors")
        return out

    def sift_min_distances(self, left_desc, cand_desc, row_ptr) -> np.ndarray:
        left_desc = np.ascontiguousarray(left_desc, dtype=np.float32).reshape(-1, 2, 128)
        cand_desc = np.ascontiguousarray(cand_desc, dtype=np.float32).reshape(-1, 2, 128)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        assert len(row_ptr) == len(left_desc) + 1 and int(row_ptr[-1]) == len(cand_desc)
        out = np.zeros(len(cand_desc))
        self._check(self.lib.ebvo_sift_min_distances(self._ctx, ptr(left_desc), len(left_desc), ptr(cand_desc), ptr(row_ptr),
                                                     ptr(out)), "ebvo_sift_min_distances")
        return out

    def _finalize_args(self, calib, bnb_ratio, ncc_thr, use_sift, sift_thr, bnb_sift, gn):
        from ._lib import FinalizeParams
        p = FinalizeParams()
        p.bnb_ratio, p.ncc_thr, p.gn = bnb_ratio, ncc_thr, self._gn_params(**gn)
        p.use_sift, p.sift_thr, p.bnb_sift = int(bool(use_sift)), sift_thr, bnb_sift
        return p, None if calib is None else self._calib(calib)

    def stereo_finalize_submit(self, calib=None, slot=0, bnb_ratio=0.9, ncc_thr=0.6, use_sift=False, sift_thr=500.0,
                               bnb_sift=0.4, **gn):
        """Enqueue the chain after the first NCC pass on the slot's stream and return (ebvo_stereo_finalize_submit)."""
        p, cal = self._finalize_args(calib, bnb_ratio, ncc_thr, use_sift, sift_thr, bnb_sift, gn)
        self._check(self.lib.ebvo_stereo_finalize_submit(self._ctx, slot, C.byref(p), C.byref(cal) if cal is not None else None),
                    "ebvo_stereo_finalize_submit")
        self._fin_opts = getattr(self, "_fin_opts", {})
        self._fin_opts[slot] = (calib is not None, bool(use_sift))

    def stereo_finalize_wait(self, slot=0, fetch=True):
        """Wait for the chain of `slot`; returns (counts dict, dict(left_index, right, score[, rows]) or None)."""
        from ._lib import FinalizeCounts
        cnt = FinalizeCounts()
        self._check(self.lib.ebvo_stereo_finalize_wait(self._ctx, slot, C.byref(cnt)), "ebvo_stereo_finalize_wait")
        has_rows, use_sift = self._fin_opts.get(slot, (False, False))
        keys = ("n_sift",) * use_sift + ("n_ncc", "n_bnb", "n_clusters", "n_ncc2", "n_final")
        counts = {k: getattr(cnt, k) for k in keys}
        if not fetch:
            return counts, None
        n = cnt.n_final
        out = dict(left_index=np.zeros(n, dtype=np.int32), right=np.zeros(n, dtype=EDGE_DTYPE), score=np.zeros(n))
        rows = np.zeros((n, 16)) if has_rows else None
        self._check(self.lib.ebvo_stereo_fetch_final(self._ctx, slot, ptr(out["left_index"]), ptr(out["right"]),
                                                     ptr(out["score"]), ptr(rows)), "ebvo_stereo_fetch_final")
        if rows is not None:
            out["rows"] = rows
        return counts, out

    def stereo_finalize(self, calib=None, slot=0, bnb_ratio=0.9, ncc_thr=0.6, use_sift=False, sift_thr=500.0, bnb_sift=0.4,
                        **gn):
        """BNB -> shift -> refine -> cluster -> NCC -> best on the resident pair.  calib = (K_left, K_right, R21, T21) adds the
        output-file rows.  Returns (counts dict, dict(left_index, right, score[, rows]))."""
        self.stereo_finalize_submit(calib, slot, bnb_ratio, ncc_thr, use_sift, sift_thr, bnb_sift, **gn)
        return self.stereo_finalize_wait(slot)

    def stereo_refine(self, counts, slot=0, **kw):
        """Refine every kept match of the resident pair on the device; returns the per-pair outputs (n_pairs entries,
        validity 255 where the pair was not a kept match)."""
        p = self._gn_params(**kw)
        self._check(self.lib.ebvo_stereo_refine(self._ctx, slot, C.byref(p)), "ebvo_stereo_refine")
        n = int(counts.n_pairs)
        out = dict(alpha=np.zeros(n), score=np.zeros(n), confidence=np.zeros(n), validity=np.zeros(n, dtype=np.uint8),
                   iters=np.zeros(n, dtype=np.int32), refined_xy=np.zeros((n, 2)))
        self._check(self.lib.ebvo_stereo_fetch_refined(self._ctx, slot, ptr(out["alpha"]), ptr(out["score"]),
                                                       ptr(out["confidence"]), ptr(out["validity"]), ptr(out["iters"]),
                                                       ptr(out["refined_xy"])), "ebvo_stereo_fetch_refined")
        return out

    # -- Utility::get_edge_patches ------------------------------------------------------------
    def edge_patches(self, img, edges) -> np.ndarray:
        img = _u8(img)
        h, w = img.shape
        edges = _edges(edges)
        out = np.zeros((len(edges), 2, 49), dtype=np.float32)
        self._check(self.lib.ebvo_edge_patches(self._ctx, ptr(img), h, w, img.strides[0], ptr(edges), len(edges),
                                               ptr(out)), "ebvo_edge_patches")
        return out

    # -- Utility::get_patch_similarity / MatlabNCCComputer::computeNCC -----------------------
    def ncc_patches(self, A, B) -> np.ndarray:
        A = np.ascontiguousarray(A, dtype=np.float32).reshape(-1, 49)
        B = np.ascontiguousarray(B, dtype=np.float32).reshape(-1, 49)
        assert A.shape == B.shape
        sim = np.zeros(len(A), dtype=np.float64)
        self._check(self.lib.ebvo_ncc_patches(self._ctx, ptr(A), ptr(B), len(A), ptr(sim)), "ebvo_ncc_patches")
        return sim

    # -- Temporal_Matches::apply_NCC_filtering_quads ------------------------------------------
    def ncc_quads(self, kfL, kfR, cfL, cfR, thr=0.8):
        arrs = [np.ascontiguousarray(a, dtype=np.float32).reshape(-1, 98) for a in (kfL, kfR, cfL, cfR)]
        n = len(arrs[0])
        sl, sr = np.zeros(n), np.zeros(n)
        keep = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.ebvo_ncc_quads(self._ctx, *[ptr(a) for a in arrs], n, thr, ptr(sl), ptr(sr), ptr(keep)),
                    "ebvo_ncc_quads")
        return sl, sr, keep

    # -- device-resident pipeline --------------------------------------------------------------
    def default_params(self, F21=None) -> StereoParams:
        p = StereoParams()
        self.lib.ebvo_stereo_default_params(C.byref(p))
        if F21 is not None:
            F = np.ascontiguousarray(F21, dtype=np.float64).reshape(9)
            for k in range(9):
                p.F21[k] = float(F[k])
        return p

    def set_slots(self, n: int):
        self._check(self.lib.ebvo_stereo_set_slots(self._ctx, n), "ebvo_stereo_set_slots")

    def stereo_upload(self, left, right, slot: int = 0):
        left, right = _u8(left), _u8(right)
        h, w = left.shape
        assert right.shape == (h, w)
        self._check(self.lib.ebvo_stereo_upload_slot(self._ctx, slot, ptr(left), ptr(right), h, w, left.strides[0],
                                                     right.strides[0]), "ebvo_stereo_upload_slot")

    def stereo_upload_async(self, left, right, slot: int = 0):
        """ebvo_stereo_upload_async: returns once the copies are enqueued (page-locked sources: host_register); the slot's next
        submission waits for them on the device.  The arrays must stay alive and unchanged until the pair has been waited for."""
        assert left.dtype == np.uint8 and right.dtype == np.uint8 and left.flags.c_contiguous and right.flags.c_contiguous
        h, w = left.shape
        assert right.shape == (h, w)
        self._check(self.lib.ebvo_stereo_upload_async(self._ctx, slot, ptr(left), ptr(right), h, w, left.strides[0],
                                                      right.strides[0]), "ebvo_stereo_upload_async")

    def host_register(self, arr: np.ndarray):
        """page-lock a numpy array (a frame ring) for asynchronous uploads"""
        self._check(self.lib.ebvo_host_register(self._ctx, ptr(arr), arr.nbytes), "ebvo_host_register")

    def ingest_stats(self) -> dict:
        out = np.zeros(2, dtype=np.int64)
        self._check(self.lib.ebvo_ingest_stats(self._ctx, ptr(out)), "ebvo_ingest_stats")
        return {"pull_uploads": int(out[0]), "stream_uploads": int(out[1])}

    def host_unregister(self, arr: np.ndarray):
        self._check(self.lib.ebvo_host_unregister(self._ctx, ptr(arr)), "ebvo_host_unregister")

    def stereo_run(self, params: StereoParams) -> StereoCounts:
        c = StereoCounts()
        self._check(self.lib.ebvo_stereo_run(self._ctx, C.byref(params), C.byref(c)), "ebvo_stereo_run")
        return c

    def stereo_submit(self, params: StereoParams, slot: int = 0):
        self._check(self.lib.ebvo_stereo_submit(self._ctx, slot, C.byref(params)), "ebvo_stereo_submit")

    def stereo_wait(self, slot: int = 0) -> StereoCounts:
        c = StereoCounts()
        self._check(self.lib.ebvo_stereo_wait(self._ctx, slot, C.byref(c)), "ebvo_stereo_wait")
        return c

    def stereo_fetch(self, counts: StereoCounts, patches: bool = False, slot: int = 0):
        nL, nR, npairs = counts.n_left, counts.n_right, counts.n_pairs
        left = np.zeros(nL, dtype=EDGE_DTYPE)
        right = np.zeros(nR, dtype=EDGE_DTYPE)
        row_ptr = np.zeros(nL + 1, dtype=np.int32)
        col = np.zeros(npairs, dtype=np.int32)
        sims = np.zeros((npairs, 4))
        best = np.zeros(npairs)
        keep = np.zeros(npairs, dtype=np.uint8)
        lp = np.zeros((nL, 2, 49), dtype=np.float32) if patches else None
        self._check(self.lib.ebvo_stereo_fetch_slot(self._ctx, slot, ptr(left), ptr(right), ptr(row_ptr), ptr(col),
                                                    ptr(sims), ptr(best), ptr(keep), ptr(lp)), "ebvo_stereo_fetch_slot")
        return dict(left=left, right=right, row_ptr=row_ptr, col_idx=col, sims=sims, best=best, keep=keep,
                    left_patches=lp)

    # -- temporal quads against the keyframe (src/Temporal_Matches.cpp:335-469) -----------------------------------
    def temporal_set_keyframe(self, slot: int = 0):
        self._check(self.lib.ebvo_temporal_set_keyframe(self._ctx, slot), "ebvo_temporal_set_keyframe")

    def temporal_match_submit(self, slot: int = 0, **kw):
        """Enqueue the candidate + NCC stages of the slot's final mates against the keyframe (ebvo_temporal_match_submit).
        kw: fields of ebvo_temporal_params; max_iter / tol / huber_delta set the nested Gauss-Newton parameters."""
        p = _lib.TemporalParams()
        self.lib.ebvo_temporal_default_params(C.byref(p))
        fields = {name for name, _ in p._fields_} - {"gn"}
        for k, v in kw.items():
            if k in ("max_iter", "tol", "huber_delta"):
                setattr(p.gn, k, v)
            elif k in fields:
                setattr(p, k, v)
            else:
                raise TypeError(f"temporal_match: unknown parameter {k!r}")
        self._tq_n_kf.pop(slot, None)
        self._check(self.lib.ebvo_temporal_match_submit(self._ctx, slot, C.byref(p)), "ebvo_temporal_match_submit")
        self._tq_stages = getattr(self, "_tq_stages", {})
        self._tq_stages[slot] = int(p.stages)

    def temporal_match_wait(self, slot: int = 0, fetch: bool = True):
        c = _lib.TemporalCounts()
        self._check(self.lib.ebvo_temporal_match_wait(self._ctx, slot, C.byref(c)), "ebvo_temporal_match_wait")
        self._tq_n_kf[slot] = int(c.n_kf)
        return self._temporal_results(slot, c, self._tq_stages.get(slot, 0), fetch)

    def temporal_match(self, slot: int = 0, fetch: bool = True, **kw):
        self.temporal_match_submit(slot, **kw)
        return self.temporal_match_wait(slot, fetch)

    def _temporal_results(self, slot, c, stages, fetch):
        counts = dict(n_kf=c.n_kf, n_cf=c.n_cf, n_candidates=c.n_candidates, n_kept=c.n_kept)
        if stages:
            counts.update(n_sift=c.n_sift, n_bnb_ncc=c.n_bnb_ncc, n_bnb_sift=c.n_bnb_sift, n_refined_valid=c.n_refined_valid,
                          n_final=c.n_final)
        if not fetch:
            return counts, None
        n = c.n_candidates
        out = dict(row_ptr=np.zeros(c.n_kf + 1, dtype=np.int32), col_idx=np.zeros(n, dtype=np.int32), sim_left=np.zeros(n),
                   sim_right=np.zeros(n), keep=np.zeros(n, dtype=np.uint8))
        self._check(self.lib.ebvo_temporal_fetch(self._ctx, slot, ptr(out["row_ptr"]), ptr(out["col_idx"]), ptr(out["sim_left"]),
                                                 ptr(out["sim_right"]), ptr(out["keep"])), "ebvo_temporal_fetch")
        if stages:
            m = c.n_final
            fin = dict(row_ptr=np.zeros(c.n_kf + 1, dtype=np.int32), cf_index=np.zeros(m, dtype=np.int32),
                       left=np.zeros(m, dtype=EDGE_DTYPE), right=np.zeros(m, dtype=EDGE_DTYPE), ncc_left=np.zeros(m),
                       sift_left=np.zeros(m), score_left=np.zeros(m), score_right=np.zeros(m), valid=np.zeros(m, dtype=np.uint8))
            self._check(self.lib.ebvo_temporal_fetch_final(self._ctx, slot, *(ptr(fin[k]) for k in (
                "row_ptr", "cf_index", "left", "right", "ncc_left", "sift_left", "score_left", "score_right", "valid"))),
                "ebvo_temporal_fetch_final")
            out["final"] = fin
        return counts, out

    # -- relative pose from the final quads (MotionTracker::estimate_Relative_Pose_From_Quad_Pairs) -----------------------
    def pose_params(self, **kw) -> _lib.PoseParams:
        """ebvo_pose_params: the reference's defaults with `kw` (field names of the struct) applied."""
        p = _lib.PoseParams()
        self.lib.ebvo_pose_default_params(C.byref(p))
        fields = {name for name, _ in p._fields_}
        for k, v in kw.items():
            if k not in fields:
                raise TypeError(f"pose: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    @staticmethod
    def _calib(calib) -> _lib.StereoCalib:
        """(K_left, K_right, R21, T21) -> ebvo_stereo_calib (row-major 3x3 matrices, T21 of 3)"""
        cal = _lib.StereoCalib()
        for name, v, n in zip(("K_left", "K_right", "R21", "T21"), calib, (9, 9, 9, 3)):
            getattr(cal, name)[:] = np.ascontiguousarray(v, dtype=np.float64).reshape(n).tolist()
        return cal

    @staticmethod
    def _pose_dict(r) -> dict:
        out = {k: getattr(r, k) for k in ("status", "n_quads", "top_n", "iterations", "draws", "hypotheses", "best_inliers",
                                          "dynamic_max_iter", "inlier_ratio", "best_q1", "best_q2")}
        out["found"] = bool(r.found)
        out["R"] = np.array(r.R[:], dtype=np.float64).reshape(3, 3)
        out["t"] = np.array(r.t[:], dtype=np.float64)
        return out

    def temporal_estimate_pose(self, calib, slot: int = 0, **params) -> dict:
        """RANSAC relative pose on the slot's final quads (after temporal_match(stages=1)) and the keyframe mates
        (ebvo_temporal_estimate_pose).  calib = (K_left, K_right, R21, T21); params: fields of ebvo_pose_params.
        Returns the result fields, R (3x3), t and `inlier` (uint8 per final quad, CSR order of the final quads)."""
        p, cal, r = self.pose_params(**params), self._calib(calib), _lib.PoseResult()
        n_kf, n = C.c_int32(), C.c_int64()   # the slot's own count of final quads sizes the mask
        self._check(self.lib.ebvo_temporal_final_size(self._ctx, slot, C.byref(n_kf), C.byref(n)), "ebvo_temporal_final_size")
        inlier = np.zeros(n.value, dtype=np.uint8)
        self._check(self.lib.ebvo_temporal_estimate_pose(self._ctx, slot, C.byref(cal), C.byref(p), C.byref(r), ptr(inlier)),
                    "ebvo_temporal_estimate_pose")
        out = self._pose_dict(r)
        out["inlier"] = inlier
        return out

    def pose_from_quads(self, kf_left, kf_right, row_ptr, cf_left, cf_right, calib, **params) -> dict:
        """The same on host arrays (ebvo_pose_from_quads): KF mates per row, CSR row_ptr, CF left / right centres per quad.
        Also returns `quad_geom` (n x 12: Gamma, Gamma_bar, T, T_bar) and `rank_order` (CSR index per rank position); both
        stay zero when status = 1 (insufficient quads)."""
        kf_left, kf_right = _edges(kf_left), _edges(kf_right)
        cf_left, cf_right = _edges(cf_left), _edges(cf_right)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        assert len(kf_left) == len(kf_right) == len(row_ptr) - 1
        n = int(row_ptr[-1])
        assert len(cf_left) == len(cf_right) == n
        p, cal, r = self.pose_params(**params), self._calib(calib), _lib.PoseResult()
        inlier, geom, order = np.zeros(n, dtype=np.uint8), np.zeros((n, 12)), np.zeros(n, dtype=np.int32)
        self._check(self.lib.ebvo_pose_from_quads(self._ctx, ptr(kf_left), ptr(kf_right), len(kf_left), ptr(row_ptr), ptr(cf_left),
                                                  ptr(cf_right), C.byref(cal), C.byref(p), C.byref(r), ptr(inlier), ptr(geom),
                                                  ptr(order)), "ebvo_pose_from_quads")
        out = self._pose_dict(r)
        out.update(inlier=inlier, quad_geom=geom, rank_order=order)
        return out

    # -- the pose stage under ground truth (get_Quad_for_Pose_Solution's has_gt() branch, Solution_Constraints_Application) --
    @staticmethod
    def _row_mask(a, n_kf, what):
        if a is None:
            return None
        a = np.ascontiguousarray(a, dtype=np.uint8)
        if a.shape != (n_kf,):
            raise ValueError(f"{what}: one byte per keyframe mate")
        return a

    def _gt_quads(self, kf_left, kf_right, row_ptr, cf_left, cf_right, row_listed, kf_is_tp):
        kf_left, kf_right = _edges(kf_left), _edges(kf_right)
        cf_left, cf_right = _edges(cf_left), _edges(cf_right)
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        assert len(kf_left) == len(kf_right) == len(row_ptr) - 1
        assert len(cf_left) == len(cf_right) == int(row_ptr[-1])
        n_kf = len(kf_left)
        return (kf_left, kf_right, row_ptr, cf_left, cf_right, self._row_mask(row_listed, n_kf, "row_listed"),
                self._row_mask(kf_is_tp, n_kf, "kf_is_tp"))

    def pose_from_quads_gt(self, kf_left, kf_right, row_ptr, cf_left, cf_right, calib, row_listed=None, kf_is_tp=None,
                           **params) -> dict:
        """pose_from_quads over the quads of the rows that are listed and TP (ebvo_pose_from_quads_gt); row_listed / kf_is_tp:
        one byte per keyframe mate or None (all set).  n_quads is the selected count; `inlier` and `quad_geom` are in the full
        CSR order (zero on quads not selected), `rank_order` holds full-CSR indices, -1 beyond the selected count."""
        kfL, kfR, rp, cfL, cfR, listed, tp = self._gt_quads(kf_left, kf_right, row_ptr, cf_left, cf_right, row_listed, kf_is_tp)
        n = int(rp[-1])
        p, cal, r = self.pose_params(**params), self._calib(calib), _lib.PoseResult()
        inlier, geom, order = np.zeros(n, dtype=np.uint8), np.zeros((n, 12)), np.zeros(n, dtype=np.int32)
        self._check(self.lib.ebvo_pose_from_quads_gt(self._ctx, ptr(kfL), ptr(kfR), len(kfL), ptr(rp), ptr(cfL), ptr(cfR), ptr(listed),
                                                     ptr(tp), C.byref(cal), C.byref(p), C.byref(r), ptr(inlier), ptr(geom),
                                                     ptr(order)), "ebvo_pose_from_quads_gt")
        out = self._pose_dict(r)
        out.update(inlier=inlier, quad_geom=geom, rank_order=order)
        return out

    def temporal_estimate_pose_gt(self, calib, slot: int = 0, **params) -> dict:
        """temporal_estimate_pose over the ground-truth rows of a slot armed by temporal_set_gt after temporal_match(stages=1)
        (ebvo_temporal_estimate_pose_gt)."""
        p, cal, r = self.pose_params(**params), self._calib(calib), _lib.PoseResult()
        n_kf, n = C.c_int32(), C.c_int64()
        self._check(self.lib.ebvo_temporal_final_size(self._ctx, slot, C.byref(n_kf), C.byref(n)), "ebvo_temporal_final_size")
        inlier = np.zeros(n.value, dtype=np.uint8)
        self._check(self.lib.ebvo_temporal_estimate_pose_gt(self._ctx, slot, C.byref(cal), C.byref(p), C.byref(r), ptr(inlier)),
                    "ebvo_temporal_estimate_pose_gt")
        out = self._pose_dict(r)
        out["inlier"] = inlier
        return out

    @staticmethod
    def _cascade_runs(runs, draw_idx, draw_stage, details):
        out = []
        for r in runs:
            stages = [dict(name=_lib.PC_STAGE_NAMES[g.stage], stage=g.stage, surviving=g.surviving, veridical=g.veridical,
                           recall=g.recall, precision=g.precision) for g in r.stages]
            out.append(_CascadeRun(stages, status=r.status, n_quads=r.n_quads, top_n=r.top_n, draws=r.draws))
        return (out, draw_idx, draw_stage) if details else out

    @staticmethod
    def _cascade_buffers(p, n_runs, details):
        """the run records and, for details, the draw arrays; sizes the library refuses are left to it (nothing is allocated
        for them)"""
        n_runs = int(n_runs)
        runs = (_lib.PoseCascadeRun * max(n_runs, 0))()
        ok = n_runs >= 1 and 0 <= p.max_iterations and n_runs * p.max_iterations <= _lib.PC_MAX_DRAWS
        idx = np.zeros((n_runs, p.max_iterations, 2), dtype=np.int32) if details and ok else None
        stage = np.zeros((n_runs, p.max_iterations), dtype=np.uint8) if details and ok else None
        return n_runs, runs, idx, stage

    def pose_constraint_metrics(self, kf_left, kf_right, row_ptr, cf_left, cf_right, calib, row_listed=None, kf_is_tp=None,
                                quad_is_tp=None, n_runs: int = 1, details: bool = False, **params):
        """Solution_Constraints_Application on host arrays (ebvo_pose_constraint_metrics): n_runs runs of max_iterations
        sampled quad pairs each.  quad_is_tp: b_is_veridical per quad in CSR order or None (none veridical).  Returns a list
        of runs; a run is a list of five stage dicts (name, stage, surviving, veridical, recall, precision) under the
        reference's names and carries status, n_quads, top_n and draws as attributes.  details=True: also draw_idx
        (n_runs x max_iterations x 2 rank positions) and draw_stage (bits 0-2: constraints passed, bit 7: both veridical)."""
        kfL, kfR, rp, cfL, cfR, listed, tp = self._gt_quads(kf_left, kf_right, row_ptr, cf_left, cf_right, row_listed, kf_is_tp)
        if quad_is_tp is not None:
            quad_is_tp = np.ascontiguousarray(quad_is_tp, dtype=np.uint8)
            if quad_is_tp.shape != (int(rp[-1]),):
                raise ValueError("quad_is_tp: one byte per quad")
        p, cal = self.pose_params(**params), self._calib(calib)
        n_runs, runs, idx, stage = self._cascade_buffers(p, n_runs, details)
        self._check(self.lib.ebvo_pose_constraint_metrics(self._ctx, ptr(kfL), ptr(kfR), len(kfL), ptr(rp), ptr(cfL), ptr(cfR),
                                                          ptr(listed), ptr(tp), ptr(quad_is_tp), C.byref(cal), C.byref(p), n_runs, runs,
                                                          ptr(idx), ptr(stage)), "ebvo_pose_constraint_metrics")
        return self._cascade_runs(runs, idx, stage, details)

    def temporal_pose_constraint_metrics(self, calib, slot: int = 0, n_runs: int = 1, details: bool = False, **params):
        """The same on a slot armed by temporal_set_gt after temporal_match(stages=1)
        (ebvo_temporal_pose_constraint_metrics): b_is_veridical is the slot's Edge Clustering flag."""
        p, cal = self.pose_params(**params), self._calib(calib)
        n_runs, runs, idx, stage = self._cascade_buffers(p, n_runs, details)
        self._check(self.lib.ebvo_temporal_pose_constraint_metrics(self._ctx, slot, C.byref(cal), C.byref(p), n_runs, runs, ptr(idx),
                                                                   ptr(stage)), "ebvo_temporal_pose_constraint_metrics")
        return self._cascade_runs(runs, idx, stage, details)

    # -- inlier refit of the relative pose (Gauss-Newton over both cameras; the contract is in ebvo_hip.h) ----------------
    def _refine_params(self, params):
        """splits **params into ebvo_pose_params (only max_reproj_error is read) and ebvo_pose_refine_params"""
        rp = _lib.PoseRefineParams()
        self.lib.ebvo_pose_refine_default_params(C.byref(rp))
        mine = {name for name, _ in rp._fields_}
        for k in [k for k in params if k in mine]:
            setattr(rp, k, params.pop(k))
        return self.pose_params(**params), rp

    @staticmethod
    def _start_pose(R, t):
        R = np.ascontiguousarray(R, dtype=np.float64).reshape(9)
        t = np.ascontiguousarray(t, dtype=np.float64).reshape(3)
        return R, t

    @staticmethod
    def _refined_dict(r, inlier) -> dict:
        out = {k: getattr(r, k) for k in ("status", "stop_reason", "rounds_run", "steps_kept", "n_quads", "fit_quads", "inliers",
                                          "cost_first", "cost_last")}
        out["R"] = np.array(r.R[:], dtype=np.float64).reshape(3, 3)
        out["t"] = np.array(r.t[:], dtype=np.float64)
        out["inlier"] = inlier
        return out

    def pose_refine_from_quads(self, kf_left, kf_right, row_ptr, cf_left, cf_right, calib, R, t, row_listed=None, kf_is_tp=None,
                               **params) -> dict:
        """Refit of the start pose (R, t) on its inliers among the host quads (ebvo_pose_refine_from_quads); row_listed /
        kf_is_tp select rows as in pose_from_quads_gt.  params: max_reproj_error and the fields of ebvo_pose_refine_params
        (rounds, iterations, huber_px, step_eps, block_threads).  Returns the fields of ebvo_pose_refined, R (3x3), t and
        `inlier` (uint8 per quad in the full CSR order, under the returned pose)."""
        kfL, kfR, rp_, cfL, cfR, listed, tp = self._gt_quads(kf_left, kf_right, row_ptr, cf_left, cf_right, row_listed, kf_is_tp)
        p, rp = self._refine_params(dict(params))
        cal, r = self._calib(calib), _lib.PoseRefined()
        R, t = self._start_pose(R, t)
        inlier = np.zeros(int(rp_[-1]), dtype=np.uint8)
        self._check(self.lib.ebvo_pose_refine_from_quads(self._ctx, ptr(kfL), ptr(kfR), len(kfL), ptr(rp_), ptr(cfL), ptr(cfR),
                                                         ptr(listed), ptr(tp), C.byref(cal), C.byref(p), C.byref(rp), ptr(R), ptr(t),
                                                         C.byref(r), ptr(inlier)), "ebvo_pose_refine_from_quads")
        return self._refined_dict(r, inlier)

    def temporal_refine_pose(self, calib, R, t, slot: int = 0, gt_rows: bool = False, **params) -> dict:
        """The same on the slot's final quads (ebvo_temporal_refine_pose); gt_rows: over the ground-truth rows of an armed
        slot, as temporal_estimate_pose_gt selects them."""
        p, rp = self._refine_params(dict(params))
        cal, r = self._calib(calib), _lib.PoseRefined()
        R, t = self._start_pose(R, t)
        n_kf, n = C.c_int32(), C.c_int64()
        self._check(self.lib.ebvo_temporal_final_size(self._ctx, slot, C.byref(n_kf), C.byref(n)), "ebvo_temporal_final_size")
        inlier = np.zeros(n.value, dtype=np.uint8)
        self._check(self.lib.ebvo_temporal_refine_pose(self._ctx, slot, C.byref(cal), C.byref(p), C.byref(rp), ptr(R), ptr(t),
                                                       1 if gt_rows else 0, C.byref(r), ptr(inlier)), "ebvo_temporal_refine_pose")
        return self._refined_dict(r, inlier)

    # -- alignment of the pose to the current frame's TOED edges by normal distance (the contract is in ebvo_hip.h) --------
    def align_params(self, **kw) -> _lib.AlignParams:
        """ebvo_align_params: the defaults of ebvo_align_default_params with `kw` applied."""
        p = _lib.AlignParams()
        self.lib.ebvo_align_default_params(C.byref(p))
        fields = {name for name, _ in p._fields_}
        for k, v in kw.items():
            if k not in fields:
                raise TypeError(f"align: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    @staticmethod
    def _aligned_dict(r, assoc_left, assoc_right) -> dict:
        out = {k: getattr(r, k) for k in ("status", "stop_reason", "rounds_run", "steps_kept", "n_kf", "fit_terms", "inliers",
                                          "cost_first", "cost_last", "rms_normal")}
        out["n_assoc"] = (int(r.n_assoc[0]), int(r.n_assoc[1]))
        out["R"] = np.array(r.R[:], dtype=np.float64).reshape(3, 3)
        out["t"] = np.array(r.t[:], dtype=np.float64)
        out["assoc_left"], out["assoc_right"] = assoc_left, assoc_right
        return out

    def pose_align_edges(self, kf_left, kf_right, cf_edges_left, cf_edges_right, img_w: int, img_h: int, calib, R, t, lambda_=None,
                         **params) -> dict:
        """Alignment of the start pose (R, t) to the current frame's TOED edges on host arrays (ebvo_pose_align_edges):
        cf_edges_right may be None with cameras=1.  params: the fields of ebvo_align_params.  lambda_ (one double per keyframe
        mate): the alignment on Gamma / lambda (ebvo_pose_align_edges_depth).  Returns the fields of ebvo_aligned_pose, R (3x3),
        t, and assoc_left / assoc_right (int32 per keyframe mate: edge index or -1)."""
        kfL, kfR, E0 = _edges(kf_left), _edges(kf_right), _edges(cf_edges_left)
        E1 = _edges(cf_edges_right) if cf_edges_right is not None else np.zeros(0, dtype=EDGE_DTYPE)
        if len(kfL) != len(kfR):
            raise ValueError("kf_left and kf_right differ in length")
        p, cal, r = self.align_params(**params), self._calib(calib), _lib.AlignedPose()
        R, t = self._start_pose(R, t)
        aL, aR = np.full(len(kfL), -1, dtype=np.int32), np.full(len(kfL), -1, dtype=np.int32)
        tail = (ptr(E0), len(E0), ptr(E1) if cf_edges_right is not None else None, len(E1), int(img_w), int(img_h), C.byref(cal),
                C.byref(p), ptr(R), ptr(t), C.byref(r), ptr(aL), ptr(aR))
        if lambda_ is None:
            self._check(self.lib.ebvo_pose_align_edges(self._ctx, ptr(kfL), ptr(kfR), len(kfL), *tail), "ebvo_pose_align_edges")
        else:
            lam = np.ascontiguousarray(lambda_, dtype=np.float64)
            if lam.shape != (len(kfL),):
                raise ValueError("lambda_ needs one value per keyframe mate")
            self._check(self.lib.ebvo_pose_align_edges_depth(self._ctx, ptr(kfL), ptr(kfR), ptr(lam), len(kfL), *tail),
                        "ebvo_pose_align_edges_depth")
        return self._aligned_dict(r, aL, aR)

    def temporal_align_pose(self, calib, R, t, slot: int = 0, **params) -> dict:
        """The same with the context's keyframe mates against the kept TOED edge lists the slot's pair left resident
        (ebvo_temporal_align_pose): needs a keyframe and a waited pair, neither finalisation nor a temporal match."""
        p, cal, r = self.align_params(**params), self._calib(calib), _lib.AlignedPose()
        R, t = self._start_pose(R, t)
        n_kf, n0, n1 = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.ebvo_temporal_align_size(self._ctx, slot, C.byref(n_kf), C.byref(n0), C.byref(n1)),
                    "ebvo_temporal_align_size")
        aL, aR = np.full(n_kf.value, -1, dtype=np.int32), np.full(n_kf.value, -1, dtype=np.int32)
        self._check(self.lib.ebvo_temporal_align_pose(self._ctx, slot, C.byref(cal), C.byref(p), ptr(R), ptr(t), C.byref(r), ptr(aL),
                                                      ptr(aR)), "ebvo_temporal_align_pose")
        return self._aligned_dict(r, aL, aR)

    # -- inverse-depth filter of the keyframe mates, fed by aligned frames (the contract is in ebvo_hip.h) --------------------
    def depth_params(self, **kw) -> _lib.DepthParams:
        """ebvo_depth_params: the defaults of ebvo_depth_default_params with `kw` applied."""
        p = _lib.DepthParams()
        self.lib.ebvo_depth_default_params(C.byref(p))
        fields = {name for name, _ in p._fields_}
        for k, v in kw.items():
            if k not in fields:
                raise TypeError(f"depth: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    @staticmethod
    def _depth_dict(r) -> dict:
        out = {k: getattr(r, k) for k in ("n_kf", "n_dead", "n_updated", "n_restored", "rms_before", "rms_after")}
        out["n_terms"] = (int(r.n_terms[0]), int(r.n_terms[1]))
        out["n_gated"] = (int(r.n_gated[0]), int(r.n_gated[1]))
        return out

    def depth_refine_edges(self, kf_left, kf_right, cf_edges_left, cf_edges_right, assoc_left, assoc_right, img_w: int, img_h: int,
                           calib, R, t, state=None, **params) -> dict:
        """One update of the mates' inverse-depth state on host arrays (ebvo_depth_refine_edges).  assoc_*: what
        pose_align_edges returned (None: no term in that camera).  state: None (the prior) or (lambda, info, n_obs).  params:
        the fields of ebvo_depth_params.  Returns the fields of ebvo_depth_refined and the new lambda, info, n_obs, flags."""
        kfL, kfR, E0 = _edges(kf_left), _edges(kf_right), _edges(cf_edges_left)
        E1 = _edges(cf_edges_right) if cf_edges_right is not None else np.zeros(0, dtype=EDGE_DTYPE)
        n = len(kfL)
        if len(kfR) != n:
            raise ValueError("kf_left and kf_right differ in length")
        assoc = []
        for a in (assoc_left, assoc_right):
            a = None if a is None else np.ascontiguousarray(a, dtype=np.int32)
            if a is not None and a.shape != (n,):
                raise ValueError("an association array needs one value per keyframe mate")
            assoc.append(a)
        p, cal, r = self.depth_params(**params), self._calib(calib), _lib.DepthRefined()
        R, t = self._start_pose(R, t)
        lam, info, nobs, flags = np.ones(n), np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
        if state is not None:
            lam = np.array(state[0], dtype=np.float64)
            info = np.array(state[1], dtype=np.float64)
            nobs = np.array(state[2], dtype=np.int32)
            if not (lam.shape == info.shape == nobs.shape == (n,)):
                raise ValueError("the state needs one value per keyframe mate")
        sin = (ptr(lam), ptr(info), ptr(nobs)) if state is not None else (None, None, None)
        self._check(self.lib.ebvo_depth_refine_edges(self._ctx, ptr(kfL), ptr(kfR), n, ptr(E0), len(E0),
                                                     ptr(E1) if cf_edges_right is not None else None, len(E1),
                                                     None if assoc[0] is None else ptr(assoc[0]), None if assoc[1] is None else ptr(assoc[1]),
                                                     int(img_w), int(img_h), C.byref(cal), C.byref(p), ptr(R), ptr(t), *sin, ptr(lam),
                                                     ptr(info), ptr(nobs), ptr(flags), C.byref(r)), "ebvo_depth_refine_edges")
        return dict(self._depth_dict(r), lambda_=lam, info=info, n_obs=nobs, flags=flags)

    def temporal_refine_depth(self, calib, R, t, slot: int = 0, align=None, **params) -> dict:
        """One update of the keyframe's resident state from the slot's resident pair under (R, t)
        (ebvo_temporal_refine_depth).  align: a dict of ebvo_align_params fields (radius, cell_size, orient_thr_deg) for the
        association; params: the fields of ebvo_depth_params."""
        ap, dp, cal, r = self.align_params(**(align or {})), self.depth_params(**params), self._calib(calib), _lib.DepthRefined()
        R, t = self._start_pose(R, t)
        self._check(self.lib.ebvo_temporal_refine_depth(self._ctx, slot, C.byref(cal), C.byref(ap), C.byref(dp), ptr(R), ptr(t),
                                                        C.byref(r)), "ebvo_temporal_refine_depth")
        return self._depth_dict(r)

    def temporal_depth_fetch(self, slot: int = 0) -> dict:
        """lambda_, info, n_obs, flags of the keyframe's mates (ebvo_temporal_depth_fetch)."""
        n_kf, n0, n1 = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.ebvo_temporal_align_size(self._ctx, slot, C.byref(n_kf), C.byref(n0), C.byref(n1)),
                    "ebvo_temporal_align_size")
        n = n_kf.value
        lam, info, nobs, flags = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.uint8)
        self._check(self.lib.ebvo_temporal_depth_fetch(self._ctx, ptr(lam), ptr(info), ptr(nobs), ptr(flags)), "ebvo_temporal_depth_fetch")
        return dict(lambda_=lam, info=info, n_obs=nobs, flags=flags)

    def temporal_depth_reset(self) -> None:
        """The keyframe's state back to the prior (ebvo_temporal_depth_reset)."""
        self._check(self.lib.ebvo_temporal_depth_reset(self._ctx), "ebvo_temporal_depth_reset")

    def temporal_use_depth(self, on: bool) -> None:
        """temporal_align_pose works on Gamma / lambda while on (ebvo_temporal_use_depth); default off."""
        self._check(self.lib.ebvo_temporal_use_depth(self._ctx, 1 if on else 0), "ebvo_temporal_use_depth")

    # -- handover of the refined depths to the next keyframe on promotion (the contract is in ebvo_hip.h) ---------------------
    def depth_carry_params(self, **kw) -> _lib.DepthCarryParams:
        """ebvo_depth_carry_params: the defaults of ebvo_depth_carry_default_params with `kw` applied."""
        p = _lib.DepthCarryParams()
        self.lib.ebvo_depth_carry_default_params(C.byref(p))
        fields = {name for name, _ in p._fields_}
        for k, v in kw.items():
            if k not in fields:
                raise TypeError(f"depth carry: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    @staticmethod
    def _carried_dict(r) -> dict:
        return {k: int(getattr(r, k)) for k, _ in r._fields_}

    def depth_carry(self, kf_left, kf_right, new_left, new_right, img_w: int, img_h: int, calib, R, t, state=None, **params) -> dict:
        """The old keyframe's depths carried to the new mates on host arrays (ebvo_depth_carry).  state: None (nothing to carry:
        every live new mate at its prior) or the old mates' (lambda, info, n_obs).  (R, t): old keyframe -> new frame.  params:
        the fields of ebvo_depth_carry_params.  Returns the fields of ebvo_depth_carried and lambda_, info, n_obs, flags,
        src_index of the new mates."""
        oL, oR, nL, nR = _edges(kf_left), _edges(kf_right), _edges(new_left), _edges(new_right)
        no, nn = len(oL), len(nL)
        if len(oR) != no or len(nR) != nn:
            raise ValueError("left and right mates differ in length")
        p, cal, r = self.depth_carry_params(**params), self._calib(calib), _lib.DepthCarried()
        R, t = self._start_pose(R, t)
        sin = (None, None, None)
        if state is not None:
            lam_in = np.ascontiguousarray(state[0], dtype=np.float64)
            info_in = np.ascontiguousarray(state[1], dtype=np.float64)
            nobs_in = np.ascontiguousarray(state[2], dtype=np.int32)
            if not (lam_in.shape == info_in.shape == nobs_in.shape == (no,)):
                raise ValueError("the state needs one value per old keyframe mate")
            sin = (ptr(lam_in), ptr(info_in), ptr(nobs_in))
        lam, info, nobs = np.ones(nn), np.zeros(nn), np.zeros(nn, dtype=np.int32)
        flags, src = np.zeros(nn, dtype=np.uint8), np.full(nn, -1, dtype=np.int32)
        self._check(self.lib.ebvo_depth_carry(self._ctx, ptr(oL), ptr(oR), no, *sin, ptr(nL), ptr(nR), nn, int(img_w), int(img_h),
                                              C.byref(cal), C.byref(p), ptr(R), ptr(t), ptr(lam), ptr(info), ptr(nobs), ptr(flags), ptr(src),
                                              C.byref(r)), "ebvo_depth_carry")
        return dict(self._carried_dict(r), lambda_=lam, info=info, n_obs=nobs, flags=flags, src_index=src)

    def temporal_promote_keyframe(self, calib, R, t, slot: int = 0, **params) -> dict:
        """The slot's finalised pair becomes the keyframe and inherits the old keyframe's refined depths through (R, t), old
        keyframe -> this frame (ebvo_temporal_promote_keyframe).  Returns the fields of ebvo_depth_carried."""
        p, cal, r = self.depth_carry_params(**params), self._calib(calib), _lib.DepthCarried()
        R, t = self._start_pose(R, t)
        self._check(self.lib.ebvo_temporal_promote_keyframe(self._ctx, slot, C.byref(cal), C.byref(p), ptr(R), ptr(t), C.byref(r)),
                    "ebvo_temporal_promote_keyframe")
        return self._carried_dict(r)

    def temporal_depth_source(self, slot: int = 0) -> np.ndarray:
        """src_index of the last promotion: per keyframe mate the old keyframe's mate it took its depth from, or -1
        (ebvo_temporal_depth_source)."""
        n_kf, n0, n1 = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self.lib.ebvo_temporal_align_size(self._ctx, slot, C.byref(n_kf), C.byref(n0), C.byref(n1)),
                    "ebvo_temporal_align_size")
        src = np.full(n_kf.value, -1, dtype=np.int32)
        self._check(self.lib.ebvo_temporal_depth_source(self._ctx, ptr(src)), "ebvo_temporal_depth_source")
        return src

    # -- keyframe coverage, the switch policy and the frame step (the contract is in ebvo_hip.h) -------------------------------
    @staticmethod
    def _with(p, what: str, kw: dict):
        fields = {name for name, _ in p._fields_}
        for k, v in kw.items():
            if k not in fields:
                raise TypeError(f"{what}: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    def cover_params(self, **kw) -> _lib.CoverParams:
        """ebvo_cover_params: the defaults of ebvo_cover_default_params with `kw` applied."""
        p = _lib.CoverParams()
        self.lib.ebvo_cover_default_params(C.byref(p))
        return self._with(p, "cover", kw)

    def keyframe_policy(self, **kw) -> _lib.KeyframePolicy:
        """ebvo_keyframe_policy: the defaults of ebvo_keyframe_policy_default with `kw` applied."""
        p = _lib.KeyframePolicy()
        self.lib.ebvo_keyframe_policy_default(C.byref(p))
        return self._with(p, "keyframe policy", kw)

    @staticmethod
    def _cover_dict(r) -> dict:
        out = {k: int(getattr(r, k)) for k, _ in r._fields_ if k != "hist"}
        out["hist"] = np.array(r.hist[:], dtype=np.int32)
        return out

    @staticmethod
    def _cover_record(cover) -> _lib.KeyframeCover:
        r = _lib.KeyframeCover()
        for k, _ in r._fields_:
            if k == "hist":
                for b, v in enumerate(np.asarray(cover.get("hist", np.zeros(_lib.COVER_BINS)), dtype=np.int64)):
                    r.hist[b] = int(v)
            else:
                setattr(r, k, int(cover[k]))
        return r

    @staticmethod
    def _cover_outputs(n_kf: int, n0: int, w: int, h: int, cover_cell: int, arrays: bool):
        if not arrays:
            return [None] * 6
        nc = ((w + cover_cell - 1) // cover_cell) * ((h + cover_cell - 1) // cover_cell)
        return [np.zeros(n_kf, dtype=np.uint8), np.full(n_kf, -1, dtype=np.int32), np.full(n_kf, np.nan), np.zeros(n0, dtype=np.uint8),
                np.zeros(nc, dtype=np.int32), np.zeros(nc, dtype=np.int32)]

    _COVER_ARRAYS = ("flags", "assoc", "disp", "explained", "cell_edges", "cell_explained")

    def keyframe_cover_edges(self, kf_left, kf_right, cf_edges_left, img_w: int, img_h: int, calib, R, t, lambda_=None, arrays=True,
                             **params) -> dict:
        """How much of the keyframe explains the current frame's kept left edges under (R, t), on host arrays
        (ebvo_keyframe_cover_edges).  lambda_: one double per mate (None: the triangulated depths).  params: the fields of
        ebvo_cover_params.  Returns the fields of ebvo_keyframe_cover and, with arrays, flags / assoc / disp per mate, explained
        per edge and the two cell planes (cw * ch)."""
        kfL, kfR, E0 = _edges(kf_left), _edges(kf_right), _edges(cf_edges_left)
        n = len(kfL)
        if len(kfR) != n:
            raise ValueError("kf_left and kf_right differ in length")
        p, cal, r = self.cover_params(**params), self._calib(calib), _lib.KeyframeCover()
        R, t = self._start_pose(R, t)
        lam = None
        if lambda_ is not None:
            lam = np.ascontiguousarray(lambda_, dtype=np.float64)
            if lam.shape != (n,):
                raise ValueError("lambda_ needs one value per keyframe mate")
        outs = self._cover_outputs(n, len(E0), int(img_w), int(img_h), max(int(p.cover_cell), 1), arrays)
        self._check(self.lib.ebvo_keyframe_cover_edges(self._ctx, ptr(kfL), ptr(kfR), ptr(lam), n, ptr(E0), len(E0), int(img_w), int(img_h),
                                                       C.byref(cal), C.byref(p), ptr(R), ptr(t), C.byref(r), *[ptr(a) for a in outs]),
                    "ebvo_keyframe_cover_edges")
        out = self._cover_dict(r)
        if arrays:
            out.update(zip(self._COVER_ARRAYS, outs))
        return out

    def temporal_keyframe_cover(self, calib, R, t, slot: int = 0, arrays=True, **params) -> dict:
        """The same with the context's keyframe mates (on Gamma / lambda while temporal_use_depth is on) against the kept left
        edge list the slot's pair left resident (ebvo_temporal_keyframe_cover)."""
        p, cal, r = self.cover_params(**params), self._calib(calib), _lib.KeyframeCover()
        R, t = self._start_pose(R, t)
        outs = [None] * 6
        if arrays:
            n_kf, n0 = C.c_int32(), C.c_int32()
            cw, ch = C.c_int32(), C.c_int32()
            self._check(self.lib.ebvo_temporal_cover_size(self._ctx, slot, C.byref(p), C.byref(n_kf), C.byref(n0), C.byref(cw), C.byref(ch)),
                        "ebvo_temporal_cover_size")
            outs = self._cover_outputs(n_kf.value, n0.value, cw.value, ch.value, 1, True)
        self._check(self.lib.ebvo_temporal_keyframe_cover(self._ctx, slot, C.byref(cal), C.byref(p), ptr(R), ptr(t), C.byref(r),
                                                          *[ptr(a) for a in outs]), "ebvo_temporal_keyframe_cover")
        out = self._cover_dict(r)
        if arrays:
            out.update(zip(self._COVER_ARRAYS, outs))
        return out

    def keyframe_decide(self, cover: dict, **policy):
        """(decision, reasons) of ebvo_keyframe_decide on a cover record (a dict of its fields): 0 keep, 1 switch, 2 lost."""
        p, r, reasons = self.keyframe_policy(**policy), self._cover_record(cover), C.c_uint32()
        d = self.lib.ebvo_keyframe_decide(C.byref(r), C.byref(p), C.byref(reasons))
        self._check(min(d, 0), "ebvo_keyframe_decide")
        return int(d), int(reasons.value)

    def temporal_keyframe_pose(self):
        """(Rk, tk): the keyframe's pose in the sequence frame, X_kf = Rk X_seq + tk (ebvo_temporal_keyframe_pose)."""
        R, t = np.zeros(9), np.zeros(3)
        self._check(self.lib.ebvo_temporal_keyframe_pose(self._ctx, ptr(R), ptr(t)), "ebvo_temporal_keyframe_pose")
        return R.reshape(3, 3), t

    def track_params(self, align=None, depth=None, cover=None, carry=None, finalize=None, policy=None, refine_depth=True) -> _lib.TrackParams:
        """ebvo_track_params: the defaults of ebvo_track_default_params with a dict of fields applied per stage (finalize: the
        fields of ebvo_finalize_params, `gn` a dict of ebvo_gn_params fields)."""
        p = _lib.TrackParams()
        self.lib.ebvo_track_default_params(C.byref(p))
        for name, kw in (("align", align), ("depth", depth), ("cover", cover), ("carry", carry), ("policy", policy)):
            self._with(getattr(p, name), name, dict(kw or {}))
        fin = dict(finalize or {})
        self._with(p.finalize.gn, "finalize gn", dict(fin.pop("gn", {})))
        self._with(p.finalize, "finalize", fin)
        p.refine_depth = 1 if refine_depth else 0
        return p

    def temporal_track_frame(self, calib, R, t, slot: int = 0, **stages) -> dict:
        """One frame step on a waited slot (ebvo_temporal_track_frame): align from (R, t), refine the keyframe's depths, measure
        the coverage, decide and -- on decision 1 -- finalise the slot and promote it.  stages: the arguments of track_params.
        Returns pose / depth / cover / carried / finalized (dicts of the records), reasons, decision, switched, tracked,
        failed_stage, R_seq (3x3), t_seq.  A refusal raises EbvoError; its `stage` names the stage."""
        p, cal, r = self.track_params(**stages), self._calib(calib), _lib.TrackedFrame()
        R, t = self._start_pose(R, t)
        rc = self.lib.ebvo_temporal_track_frame(self._ctx, slot, C.byref(cal), C.byref(p), ptr(R), ptr(t), C.byref(r))
        if rc:
            try:
                self._check(rc, f"ebvo_temporal_track_frame (stage {r.failed_stage})")
            except _lib.EbvoError as e:
                e.stage = int(r.failed_stage)
                raise
        out = dict(pose=self._aligned_dict(r.pose, None, None), depth=self._depth_dict(r.depth), cover=self._cover_dict(r.cover),
                   carried=self._carried_dict(r.carried), finalized={k: int(getattr(r.finalized, k)) for k, _ in r.finalized._fields_},
                   reasons=int(r.reasons), decision=int(r.decision), switched=int(r.switched), tracked=int(r.tracked),
                   failed_stage=int(r.failed_stage), R_seq=np.array(r.R_seq[:], dtype=np.float64).reshape(3, 3),
                   t_seq=np.array(r.t_seq[:], dtype=np.float64))
        return out

    # -- ground-truth evaluation from a disparity map (Find_Stereo_GT_Locations, get_Stereo_Edge_GT_Pairs,
    # -- Evaluate_Stereo_Edge_Correspondences) ---------------------------------------------------------------
    def gt_params(self, **kw) -> _lib.GtParams:
        """ebvo_gt_params: the reference's constants (4.0, 0.5, 1.0, 5.0, DIST_TO_GT_THRESH 1.0) with `kw` applied."""
        p = _lib.GtParams()
        self.lib.ebvo_gt_default_params(C.byref(p))
        fields = {name for name, _ in p._fields_}
        for k, v in kw.items():
            if k not in fields:
                raise TypeError(f"gt: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    @staticmethod
    def _disp(disp) -> np.ndarray:
        disp = np.asarray(disp)
        if disp.ndim != 2 or disp.dtype != np.float32:
            raise TypeError("the disparity map is a 2-D float32 array (disp0GT.pfm as the reference reads it)")
        if disp.strides[1] != 4 or disp.strides[0] % 4 or disp.strides[0] < 4 * disp.shape[1]:
            disp = np.ascontiguousarray(disp)
        return disp

    def stereo_set_gt(self, disp, calib, slot: int = 0, **params) -> dict:
        """Arm `slot` (its pair has run) with the left disparity map: GT locations, veridical pool and the metrics of the
        stages the run formed (ebvo_stereo_set_gt).  Returns dict(n_valid, n_focused, n_pool)."""
        disp = self._disp(disp)
        p, cal = self.gt_params(**params), self._calib(calib)
        self._check(self.lib.ebvo_stereo_set_gt(self._ctx, slot, ptr(disp), disp.shape[0], disp.shape[1], disp.strides[0] // 4,
                                                C.byref(cal), C.byref(p)), "ebvo_stereo_set_gt")
        return self.stereo_gt_size(slot)

    def stereo_gt_size(self, slot: int = 0) -> dict:
        nv, nf, npool = C.c_int32(), C.c_int32(), C.c_int64()
        self._check(self.lib.ebvo_stereo_gt_size(self._ctx, slot, C.byref(nv), C.byref(nf), C.byref(npool)), "ebvo_stereo_gt_size")
        return dict(n_valid=nv.value, n_focused=nf.value, n_pool=npool.value)

    def stereo_gt_fetch(self, slot: int = 0) -> dict:
        """What Stereo_Edge_Pairs holds after get_Stereo_Edge_GT_Pairs, per focused left edge in index order."""
        sz = self.stereo_gt_size(slot)
        nf, npool = sz["n_focused"], sz["n_pool"]
        out = dict(focused_index=np.zeros(nf, dtype=np.int32), gt_xy=np.zeros((nf, 2)), gamma_left=np.zeros((nf, 3)),
                   gamma_right=np.zeros((nf, 3)), pool_row_ptr=np.zeros(nf + 1, dtype=np.int32),
                   pool_idx=np.zeros(npool, dtype=np.int32))
        self._check(self.lib.ebvo_stereo_gt_fetch(self._ctx, slot, ptr(out["focused_index"]), ptr(out["gt_xy"]),
                                                  ptr(out["gamma_left"]), ptr(out["gamma_right"]), ptr(out["pool_row_ptr"]),
                                                  ptr(out["pool_idx"])), "ebvo_stereo_gt_fetch")
        out.update(sz)
        return out

    @staticmethod
    def _gt_stage_dict(g) -> dict:
        d = {k: getattr(g, k) for k in ("stage", "rows", "nonempty", "rows_with_tp", "sum_tp", "sum_n", "recall", "precision",
                                        "precision_pair", "ambiguity")}
        d["name"] = _lib.GT_STAGE_NAMES[g.stage]
        d["present"] = bool(g.present)
        return d

    def stereo_gt_metrics(self, slot: int = 0) -> list:
        """One dict per stage of get_Stereo_Edge_Pairs, in the reference's order and under its names; `present` False for a
        stage the chain did not run (SIFT stages without use_sift, the later stages before stereo_finalize)."""
        arr = (_lib.GtStage * _lib.GT_NUM_STAGES)()
        rc = self.lib.ebvo_stereo_gt_metrics(self._ctx, slot, arr)
        if rc < 0:
            self._check(rc, "ebvo_stereo_gt_metrics")
        return [self._gt_stage_dict(arr[k]) for k in range(rc)]

    def stereo_gt_stage_rows(self, stage: int, n_left: int, slot: int = 0) -> np.ndarray:
        """(n, tp) of every left edge at `stage` ([n_left, 2] int32, zero on rows that are not focused).  n_left: the run's
        counts.n_left; a smaller value raises EbvoError(EBVO_ERR_CAPACITY), nothing is written."""
        out = np.zeros((n_left, 2), dtype=np.int32)   # the library refuses an array shorter than the slot's edge list
        self._check(self.lib.ebvo_stereo_gt_stage_rows(self._ctx, slot, stage, ptr(out), n_left), "ebvo_stereo_gt_stage_rows")
        return out

    def gt_locate(self, edges, disp, calib, **params) -> dict:
        """Find_Stereo_GT_Locations on host arrays (ebvo_gt_locate): valid, gt_xy, gamma_left, gamma_right per edge."""
        edges, disp = _edges(edges), self._disp(disp)
        p, cal = self.gt_params(**params), self._calib(calib)
        n = len(edges)
        out = dict(valid=np.zeros(n, dtype=np.uint8), gt_xy=np.zeros((n, 2)), gamma_left=np.zeros((n, 3)),
                   gamma_right=np.zeros((n, 3)))
        self._check(self.lib.ebvo_gt_locate(self._ctx, ptr(edges), n, ptr(disp), disp.shape[0], disp.shape[1], disp.strides[0] // 4,
                                            C.byref(cal), C.byref(p), ptr(out["valid"]), ptr(out["gt_xy"]), ptr(out["gamma_left"]),
                                            ptr(out["gamma_right"])), "ebvo_gt_locate")
        return out

    def gt_evaluate_rows(self, row_ptr, cand_edges, focused, gt_xy, tp_dist: float = 1.0):
        """Evaluate_Stereo_Edge_Correspondences on a CSR list of candidate edges per left edge (ebvo_gt_evaluate_rows).
        Returns (n_tp [nL, 2] int32, stage dict)."""
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        nL = len(row_ptr) - 1
        cand, focused = _edges(cand_edges), np.ascontiguousarray(focused, dtype=np.uint8)
        gt_xy = np.ascontiguousarray(gt_xy, dtype=np.float64).reshape(-1, 2)
        if nL < 0 or len(focused) != nL or len(gt_xy) != nL or (nL >= 0 and len(cand) != int(row_ptr[-1])):
            raise ValueError("gt_evaluate_rows: row_ptr, cand_edges, focused and gt_xy do not describe the same rows")
        n_tp, g = np.zeros((nL, 2), dtype=np.int32), _lib.GtStage()
        self._check(self.lib.ebvo_gt_evaluate_rows(self._ctx, ptr(row_ptr), ptr(cand), nL, ptr(focused), ptr(gt_xy), float(tp_dist),
                                                   ptr(n_tp), C.byref(g)), "ebvo_gt_evaluate_rows")
        d = self._gt_stage_dict(g)
        d.pop("name")
        return n_tp, d

    # -- temporal ground truth from a relative pose (build_Veridical_Quads, Evaluate_Temporal_Edge_Pairs_on_Quads) -------
    def tgt_params(self, **kw) -> _lib.TgtParams:
        """ebvo_tgt_params: the reference's constants (10 degrees, 2 px, 20 px, 10 px) with `kw` applied."""
        p = _lib.TgtParams()
        self.lib.ebvo_tgt_default_params(C.byref(p))
        fields = {name for name, _ in p._fields_}
        for k, v in kw.items():
            if k not in fields:
                raise TypeError(f"tgt: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    @staticmethod
    def _pose(R, t):
        return np.ascontiguousarray(R, dtype=np.float64).reshape(9), np.ascontiguousarray(t, dtype=np.float64).reshape(3)

    def temporal_set_gt(self, R, t, calib, slot: int = 0, kf_gamma=None, kf_is_tp=None, **params) -> dict:
        """Arm `slot` (its temporal match has completed) with the relative pose keyframe -> current frame
        (ebvo_temporal_set_gt).  kf_gamma: n_kf x 3 GT points of the keyframe mates or None (their triangulated points);
        kf_is_tp: n_kf flags or None (all true).  Returns dict(n_kf, n_rows, n_veridical)."""
        R, t = self._pose(R, t)
        p, cal = self.tgt_params(**params), self._calib(calib)
        if kf_gamma is not None:
            kf_gamma = np.ascontiguousarray(kf_gamma, dtype=np.float64).reshape(-1, 3)
        if kf_is_tp is not None:
            kf_is_tp = np.ascontiguousarray(kf_is_tp, dtype=np.uint8)
        for a in (kf_gamma, kf_is_tp):
            # every match of this context goes through temporal_match_wait, so a slot without a count has no match to arm
            if a is not None and len(a) != self._tq_n_kf.get(slot, -1):
                raise ValueError("temporal_set_gt: kf_gamma / kf_is_tp need one entry per keyframe mate of the slot's "
                                 "completed temporal match")
        self._check(self.lib.ebvo_temporal_set_gt(self._ctx, slot, ptr(R), ptr(t), C.byref(cal), C.byref(p), ptr(kf_gamma),
                                                  ptr(kf_is_tp)), "ebvo_temporal_set_gt")
        return self.temporal_gt_size(slot)

    def temporal_gt_size(self, slot: int = 0) -> dict:
        n_kf, n_rows, n_ver = C.c_int32(), C.c_int32(), C.c_int64()
        self._check(self.lib.ebvo_temporal_gt_size(self._ctx, slot, C.byref(n_kf), C.byref(n_rows), C.byref(n_ver)),
                    "ebvo_temporal_gt_size")
        return dict(n_kf=n_kf.value, n_rows=n_rows.value, n_veridical=n_ver.value)

    def temporal_gt_fetch(self, slot: int = 0) -> dict:
        """Per keyframe mate: in_image, proj_left / proj_right, orient_left / orient_right, and the veridical quads as a CSR
        (ver_row_ptr, ver_idx: current-frame mate indices)."""
        sz = self.temporal_gt_size(slot)
        n, m = sz["n_kf"], sz["n_veridical"]
        out = dict(in_image=np.zeros(n, dtype=np.uint8), proj_left=np.zeros((n, 2)), proj_right=np.zeros((n, 2)),
                   orient_left=np.zeros(n), orient_right=np.zeros(n), ver_row_ptr=np.zeros(n + 1, dtype=np.int32),
                   ver_idx=np.zeros(m, dtype=np.int32))
        self._check(self.lib.ebvo_temporal_gt_fetch(self._ctx, slot, *(ptr(out[k]) for k in (
            "in_image", "proj_left", "proj_right", "orient_left", "orient_right", "ver_row_ptr", "ver_idx"))),
            "ebvo_temporal_gt_fetch")
        out.update(sz)
        return out

    @staticmethod
    def _tgt_stage_dict(g) -> dict:
        d = {k: getattr(g, k) for k in ("stage", "rows", "nonempty", "rows_with_tp", "sum_tp", "sum_n", "recall", "precision",
                                        "precision_pair", "ambiguity")}
        d["name"] = _lib.TGT_STAGE_NAMES[g.stage]
        d["present"] = bool(g.present)
        return d

    def temporal_gt_metrics(self, slot: int = 0) -> list:
        """One dict per stage of get_Temporal_Edge_Pairs_from_Quads under the reference's names; `present` for Orientation,
        NCC and (after stages = 1) Edge Clustering, and after temporal_keep_stages for Location Proximity and (stages = 1)
        the four interior stages as well."""
        arr = (_lib.GtStage * _lib.TGT_NUM_STAGES)()
        rc = self.lib.ebvo_temporal_gt_metrics(self._ctx, slot, arr)
        if rc < 0:
            self._check(rc, "ebvo_temporal_gt_metrics")
        return [self._tgt_stage_dict(arr[k]) for k in range(rc)]

    def temporal_gt_flags(self, stage: int, n: int, slot: int = 0) -> np.ndarray:
        """b_is_TP per quad of a present stage, in the stage's CSR order; n: the stage's quad count (n_candidates, n_kept
        or n_final of the match; n_sift, n_bnb_ncc, n_bnb_sift, n_bnb_sift for the interior stages of a kept trail)."""
        out = np.zeros(n, dtype=np.uint8)
        self._check(self.lib.ebvo_temporal_gt_flags(self._ctx, slot, stage, ptr(out)), "ebvo_temporal_gt_flags")
        return out

    def temporal_keep_stages(self, on: bool = True, slot: int = 0):
        """Per-slot switch read by the slot's NEXT temporal match (ebvo_temporal_keep_stages): that match leaves its interior
        stage lists behind, and temporal_set_gt then evaluates every stage the match ran instead of three."""
        self._check(self.lib.ebvo_temporal_keep_stages(self._ctx, slot, int(bool(on))), "ebvo_temporal_keep_stages")

    def temporal_fetch_stage(self, stage: int, slot: int = 0) -> dict:
        """The list after the SIFT filter, after either best-nearly-best test or after the refinement (stage = the EBVO_TGT_*
        id) of a match that kept its trail with stages = 1: row_ptr over the keyframe mates, cf_index, and the centres the
        evaluation reads (left, right: the mate's edges before the refinement, the refined centres at it)."""
        n = C.c_int64()
        self._check(self.lib.ebvo_temporal_stage_size(self._ctx, slot, stage, C.byref(n)), "ebvo_temporal_stage_size")
        n_kf = self._tq_n_kf[slot]
        out = dict(row_ptr=np.zeros(n_kf + 1, dtype=np.int32), cf_index=np.zeros(n.value, dtype=np.int32),
                   left=np.zeros(n.value, dtype=EDGE_DTYPE), right=np.zeros(n.value, dtype=EDGE_DTYPE))
        self._check(self.lib.ebvo_temporal_fetch_stage(self._ctx, slot, stage, *(ptr(out[k]) for k in (
            "row_ptr", "cf_index", "left", "right"))), "ebvo_temporal_fetch_stage")
        return out

    def temporal_gt_stage_rows(self, stage: int, slot: int = 0) -> np.ndarray:
        """(n, tp) of every keyframe mate at a present stage of the armed slot ([n_kf, 2] int32, zero on rows outside the
        evaluation)."""
        n_kf = self.temporal_gt_size(slot)["n_kf"]
        out = np.zeros((n_kf, 2), dtype=np.int32)
        self._check(self.lib.ebvo_temporal_gt_stage_rows(self._ctx, slot, stage, ptr(out), n_kf), "ebvo_temporal_gt_stage_rows")
        return out

    def tgt_grid_rows(self, kf_left, kf_right, cf_left, cf_right, img_w, img_h, row_on, proj_left, proj_right, cell_size=15,
                      grid_radius: float = 30.0, tp_dist: float = 2.0):
        """The grid stage ("Location Proximity") evaluated on host arrays without forming its list (ebvo_tgt_grid_rows).
        Returns (n_tp [n_kf, 2] int32, stage dict)."""
        kf_left, kf_right, cf_left, cf_right = (_edges(a) for a in (kf_left, kf_right, cf_left, cf_right))
        n_kf, n_cf = len(kf_left), len(cf_left)
        pl = np.ascontiguousarray(proj_left, dtype=np.float64).reshape(-1, 2)
        pr = np.ascontiguousarray(proj_right, dtype=np.float64).reshape(-1, 2)
        if row_on is not None:
            row_on = np.ascontiguousarray(row_on, dtype=np.uint8)
        if len(kf_right) != n_kf or len(cf_right) != n_cf or len(pl) != n_kf or len(pr) != n_kf or \
                (row_on is not None and len(row_on) != n_kf):
            raise ValueError("tgt_grid_rows: the arrays do not describe the same mates")
        n_tp, g = np.zeros((n_kf, 2), dtype=np.int32), _lib.GtStage()
        self._check(self.lib.ebvo_tgt_grid_rows(self._ctx, ptr(kf_left), ptr(kf_right), n_kf, ptr(cf_left), ptr(cf_right), n_cf,
                                                int(img_w), int(img_h), int(cell_size), float(grid_radius), ptr(row_on), ptr(pl),
                                                ptr(pr), float(tp_dist), ptr(n_tp), C.byref(g)), "ebvo_tgt_grid_rows")
        d = self._tgt_stage_dict(g)
        d.pop("name")
        d.pop("stage")
        return n_tp, d

    def tgt_veridical(self, kf_left, kf_right, cf_left, cf_right, img_w, img_h, R, t, calib, kf_gamma=None, cell_size=15,
                      **params) -> dict:
        """build_Veridical_Quads on host arrays (ebvo_tgt_veridical): the arrays of temporal_gt_fetch."""
        kf_left, kf_right, cf_left, cf_right = (_edges(a) for a in (kf_left, kf_right, cf_left, cf_right))
        assert len(kf_left) == len(kf_right) and len(cf_left) == len(cf_right)
        R, t = self._pose(R, t)
        p, cal = self.tgt_params(**params), self._calib(calib)
        n, n_cf = len(kf_left), len(cf_left)
        if kf_gamma is not None:
            kf_gamma = np.ascontiguousarray(kf_gamma, dtype=np.float64).reshape(-1, 3)
            assert len(kf_gamma) == n
        out = dict(in_image=np.zeros(n, dtype=np.uint8), proj_left=np.zeros((n, 2)), proj_right=np.zeros((n, 2)),
                   orient_left=np.zeros(n), orient_right=np.zeros(n), ver_row_ptr=np.zeros(n + 1, dtype=np.int32))
        names = ("in_image", "proj_left", "proj_right", "orient_left", "orient_right", "ver_row_ptr")
        head = (self._ctx, ptr(kf_left), ptr(kf_right), ptr(kf_gamma), n, ptr(cf_left), ptr(cf_right), n_cf, img_w, img_h, cell_size,
                ptr(R), ptr(t), C.byref(cal), C.byref(p))
        n_ver = C.c_int64()
        self._check(self.lib.ebvo_tgt_veridical(*head, *(ptr(out[k]) for k in names), None, 0, C.byref(n_ver)), "ebvo_tgt_veridical")
        out["ver_idx"] = np.zeros(n_ver.value, dtype=np.int32)
        if n_ver.value:
            self._check(self.lib.ebvo_tgt_veridical(*head, *(ptr(out[k]) for k in names), ptr(out["ver_idx"]), n_ver.value,
                                                    C.byref(n_ver)), "ebvo_tgt_veridical")
        out["n_veridical"] = n_ver.value
        return out

    # -- temporal matching under a pose prior (this project's own stage: the search is centred on the predicted projections) --
    def tprior_params(self, **kw) -> _lib.TpriorParams:
        """ebvo_tprior_params: img_margin = 0, use_orientation = 1, with `kw` applied."""
        p = _lib.TpriorParams()
        self.lib.ebvo_tprior_default_params(C.byref(p))
        fields = {name for name, _ in p._fields_}
        for k, v in kw.items():
            if k not in fields:
                raise TypeError(f"tprior: unknown parameter {k!r}")
            setattr(p, k, v)
        return p

    def temporal_set_prior(self, R, t, calib, slot: int = 0, **params):
        """Give the slot's NEXT temporal match the relative pose keyframe -> current frame it is expected to find
        (ebvo_temporal_set_prior; the convention of temporal_set_gt and of temporal_estimate_pose's result).  One-shot: the
        next successful match consumes it; temporal_set_keyframe drops it.  params: img_margin, use_orientation."""
        R, t = self._pose(R, t)
        p, cal = self.tprior_params(**params), self._calib(calib)
        self._check(self.lib.ebvo_temporal_set_prior(self._ctx, slot, ptr(R), ptr(t), C.byref(cal), C.byref(p)),
                    "ebvo_temporal_set_prior")

    def temporal_clear_prior(self, slot: int = 0):
        self._check(self.lib.ebvo_temporal_clear_prior(self._ctx, slot), "ebvo_temporal_clear_prior")

    def temporal_prior_fetch(self, slot: int = 0) -> dict:
        """Per keyframe mate of a match made under a prior: live, proj_left / proj_right [n, 2], orient_left / orient_right."""
        n = self._tq_n_kf.get(slot, 0)
        out = dict(live=np.zeros(n, dtype=np.uint8), proj_left=np.zeros((n, 2)), proj_right=np.zeros((n, 2)),
                   orient_left=np.zeros(n), orient_right=np.zeros(n))
        self._check(self.lib.ebvo_temporal_prior_fetch(self._ctx, slot, *(ptr(out[k]) for k in (
            "live", "proj_left", "proj_right", "orient_left", "orient_right"))), "ebvo_temporal_prior_fetch")
        return out

    def tprior_candidates(self, kf_left, kf_right, cf_left, cf_right, img_w, img_h, R, t, calib, cell_size=15,
                          grid_radius: float = 30.0, orient_thr_deg: float = 10.0, cap=None, **params) -> dict:
        """The candidate stage under a pose prior on host arrays (ebvo_tprior_candidates): the arrays of temporal_prior_fetch
        plus the candidate lists row_ptr / col_idx and n_candidates.  cap: room of col_idx (None: sized by a first call)."""
        kf_left, kf_right, cf_left, cf_right = (_edges(a) for a in (kf_left, kf_right, cf_left, cf_right))
        if len(kf_left) != len(kf_right) or len(cf_left) != len(cf_right):
            raise ValueError("tprior_candidates: the arrays do not describe the same mates")
        R, t = self._pose(R, t)
        p, cal = self.tprior_params(**params), self._calib(calib)
        n, n_cf = len(kf_left), len(cf_left)
        out = dict(live=np.zeros(n, dtype=np.uint8), proj_left=np.zeros((n, 2)), proj_right=np.zeros((n, 2)),
                   orient_left=np.zeros(n), orient_right=np.zeros(n), row_ptr=np.zeros(n + 1, dtype=np.int32))
        names = ("live", "proj_left", "proj_right", "orient_left", "orient_right", "row_ptr")
        head = (self._ctx, ptr(kf_left), ptr(kf_right), n, ptr(cf_left), ptr(cf_right), n_cf, int(img_w), int(img_h), int(cell_size),
                float(grid_radius), float(orient_thr_deg), ptr(R), ptr(t), C.byref(cal), C.byref(p))
        n_cand = C.c_int64()
        if cap is None:
            self._check(self.lib.ebvo_tprior_candidates(*head, *(ptr(out[k]) for k in names), None, 0, C.byref(n_cand)),
                        "ebvo_tprior_candidates")
            cap = n_cand.value
        out["col_idx"] = np.zeros(cap, dtype=np.int32)
        rc = self.lib.ebvo_tprior_candidates(*head, *(ptr(out[k]) for k in names), ptr(out["col_idx"]), cap, C.byref(n_cand))
        out["n_candidates"] = n_cand.value
        if rc == _lib.EBVO_ERR_CAPACITY:
            err = _lib.EbvoError(rc, "ebvo_tprior_candidates", f"{n_cand.value} candidates, room for {cap}")
            err.n_candidates = n_cand.value
            raise err
        self._check(rc, "ebvo_tprior_candidates")
        out["col_idx"] = out["col_idx"][:n_cand.value]
        return out

    def tgt_evaluate_rows(self, row_ptr, left_centres, right_centres, row_on, proj_left, proj_right, tp_dist: float = 2.0):
        """Evaluate_Temporal_Edge_Pairs_on_Quads on a CSR list of quad centres per keyframe mate (ebvo_tgt_evaluate_rows).
        Returns (n_tp [n_kf, 2] int32, is_tp per quad, stage dict)."""
        row_ptr = np.ascontiguousarray(row_ptr, dtype=np.int32)
        n_kf = len(row_ptr) - 1
        L, Rr = _edges(left_centres), _edges(right_centres)
        pl = np.ascontiguousarray(proj_left, dtype=np.float64).reshape(-1, 2)
        pr = np.ascontiguousarray(proj_right, dtype=np.float64).reshape(-1, 2)
        if row_on is not None:
            row_on = np.ascontiguousarray(row_on, dtype=np.uint8)
        if n_kf < 0 or len(pl) != n_kf or len(pr) != n_kf or len(L) != int(row_ptr[-1]) or len(Rr) != len(L) or \
                (row_on is not None and len(row_on) != n_kf):
            raise ValueError("tgt_evaluate_rows: the arrays do not describe the same rows")
        n_tp, is_tp, g = np.zeros((n_kf, 2), dtype=np.int32), np.zeros(len(L), dtype=np.uint8), _lib.GtStage()
        self._check(self.lib.ebvo_tgt_evaluate_rows(self._ctx, ptr(row_ptr), ptr(L), ptr(Rr), n_kf, ptr(row_on), ptr(pl), ptr(pr),
                                                    float(tp_dist), ptr(n_tp), ptr(is_tp), C.byref(g)), "ebvo_tgt_evaluate_rows")
        d = {k: getattr(g, k) for k in ("rows", "nonempty", "rows_with_tp", "sum_tp", "sum_n", "recall", "precision",
                                        "precision_pair", "ambiguity")}
        d["present"] = bool(g.present)
        return n_tp, is_tp, d

    def stereo_fetch_begin(self, slot: int = 0, what: int = _lib.FETCH_DEFAULT):
        """Enqueue the device-to-host copies of a finished pair's results into the slot's page-locked staging."""
        self._check(self.lib.ebvo_stereo_fetch_begin(self._ctx, slot, what), "ebvo_stereo_fetch_begin")

    def stereo_fetch_end(self, slot: int = 0) -> dict:
        """Wait for the copies and return numpy VIEWS of the page-locked arrays (valid until the slot is reused)."""
        v = _lib.StereoView()
        self._check(self.lib.ebvo_stereo_fetch_end(self._ctx, slot, C.byref(v)), "ebvo_stereo_fetch_end")

        def view(ptr_, count, dtype):
            if not ptr_ or count == 0:
                return None if not ptr_ else np.zeros(0, dtype=dtype)
            nbytes = int(count) * np.dtype(dtype).itemsize
            buf = (C.c_ubyte * nbytes).from_address(ptr_)
            return np.frombuffer(buf, dtype=dtype, count=int(count))

        sims = view(v.sims, v.n_pairs * 4, np.float64)
        return dict(left=view(v.left, v.n_left, EDGE_DTYPE), right=view(v.right, v.n_right, EDGE_DTYPE),
                    row_ptr=view(v.row_ptr, v.n_left + 1, np.int32), col_idx=view(v.col_idx, v.n_pairs, np.int32),
                    sims=None if sims is None else sims.reshape(-1, 4), best=view(v.best, v.n_pairs, np.float64),
                    keep=view(v.keep, v.n_pairs, np.uint8))

    def stereo_fetch_compact_begin(self, slot: int = 0, what: int = _lib.COMPACT_DEFAULT):
        self._check(self.lib.ebvo_stereo_fetch_compact_begin(self._ctx, slot, what), "ebvo_stereo_fetch_compact_begin")

    def stereo_pushed_view(self, slot: int = 0) -> dict:
        """the compact results a pair submitted with PAIR_PUSH left in the slot's page-locked arena (no copy, no wait)"""
        v = _lib.CompactView()
        self._check(self.lib.ebvo_stereo_pushed_view(self._ctx, slot, C.byref(v)), "ebvo_stereo_pushed_view")
        return self._compact_dict(v)

    def stereo_fetch_compact_end(self, slot: int = 0) -> dict:
        """numpy VIEWS of the compact arrays: (x, y) pairs, orientations, CSR, best, keep as a bit mask (bit k & 31 of word k >> 5)"""
        v = _lib.CompactView()
        self._check(self.lib.ebvo_stereo_fetch_compact_end(self._ctx, slot, C.byref(v)), "ebvo_stereo_fetch_compact_end")
        return self._compact_dict(v)

    @staticmethod
    def _compact_dict(v) -> dict:

        def view(ptr_, count, dtype):
            if not ptr_:
                return None
            nbytes = int(count) * np.dtype(dtype).itemsize
            if nbytes == 0:
                return np.zeros(0, dtype=dtype)
            return np.frombuffer((C.c_ubyte * nbytes).from_address(ptr_), dtype=dtype, count=int(count))

        lxy, rxy = view(v.left_xy, 2 * v.n_left, np.float64), view(v.right_xy, 2 * v.n_right, np.float64)
        return dict(left_xy=None if lxy is None else lxy.reshape(-1, 2), right_xy=None if rxy is None else rxy.reshape(-1, 2),
                    left_theta=view(v.left_theta, v.n_left, np.float64), right_theta=view(v.right_theta, v.n_right, np.float64),
                    row_ptr=view(v.row_ptr, v.n_left + 1, np.int32), col_idx=view(v.col_idx, v.n_pairs, np.int32),
                    best=view(v.best, v.n_pairs, np.float64), keep_bits=view(v.keep_bits, 2 * ((v.n_pairs + 63) // 64), np.uint32),
                    n_pairs=int(v.n_pairs), n_matches=int(v.n_matches))

    def debug_set(self, key: int, value: int):
        """Test hooks (ebvo_debug_set): 0 = attempts of the regrow loop, 1 = force N overflowed results, 2 = number of
        lanes (streams the submitted pairs are dealt to when more slots are in use; 0 = one stream per slot), 3 = the
        profiler instruments one stage alone (index in profile_get()'s order + 1; 0 = every stage), 4 / 5 = launch layout
        of the refinements (1 = one thread per pair always / threshold of the eight-lanes layout); 10 = pair chain as a
        hipGraph; 11 / 12 / 17 = grids of the exact centre / mags / NCC tile kernels in blocks; 13 / 14 / 18 = A/B switches;
        15 = bit mask of kernels launched twice, 16 = the chain ends after stage N (measurement only), 20 = draws per batch
        of the pose search, 21 = most blocks of the ground-truth kernels, 22 / 23 = most blocks of every grid-stride launch
        of the temporal path / of the stereo finalize chain (same bits for any value): include/ebvo_hip.h.
        A value outside the key's range raises EbvoError(EBVO_ERR_ARG) and changes nothing."""
        self._check(self.lib.ebvo_debug_set(self._ctx, key, value), "ebvo_debug_set")

    # -- profiling -----------------------------------------------------------------------------
    def profile_enable(self, on: bool = True, every: int = 1):
        """every = N > 1: bracket only every N-th pair submitted to the device pipeline."""
        self._check(self.lib.ebvo_profile_enable(self._ctx, (max(1, every) if on else 0)), "ebvo_profile_enable")

    def profile_reset(self):
        self._check(self.lib.ebvo_profile_reset(self._ctx), "ebvo_profile_reset")

    def profile_get(self) -> dict:
        arr = (_lib.KernelTime * _lib.MAX_KERNELS)()
        n = C.c_int()
        self._check(self.lib.ebvo_profile_get(self._ctx, arr, C.byref(n)), "ebvo_profile_get")
        return {arr[k].name.decode(): (arr[k].ms, arr[k].launches) for k in range(n.value)}

    def fp64_peak(self, iters: int = 20):
        a, b = C.c_double(), C.c_double()
        self._check(self.lib.ebvo_fp64_peak(self._ctx, iters, C.byref(a), C.byref(b)), "ebvo_fp64_peak")
        return a.value, b.value
