"""CPU restatement of MotionTracker::estimate_Relative_Pose_From_Quad_Pairs (src/MotionTracker.cpp:28-253) -- the checker of
ebvo_temporal_estimate_pose / ebvo_pose_from_quads (test infrastructure).

- glibc's rand() (TYPE_3 additive generator) in Python;
- quad geometry = columns 6-11 of the oracle's finalize_pairs with K_right := K_left (MotionTracker's own arithmetic,
  get_left_calib_matrix() for both cameras);
- the rank order (:90-103);
- the loop, literally, with Python floats for the constraints and the pose and one numpy ufunc per operation for the scores
  (IEEE double, no FMA), glibc's log / ceil through the math module.
Also synthetic quads of a known motion for the tests.
"""
from __future__ import annotations

import math

import numpy as np

from tests import oracle as orc

EDGE_DTYPE = orc.EDGE_DTYPE

DEFAULTS = dict(max_iterations=5000, min_iterations=1000, dyn_num_trials_mult=3.0, success_prob=0.97, max_reproj_error=1.5,
                top_rank_fraction=0.7, tau_length=0.13, tau_t1=0.12, tau_t2=0.12, tau_tangent=0.32, rand_seed=1,
                continue_stream=0, max_draws=1 << 22)


class GlibcRand:
    """srand(seed) / rand() of glibc (random_r.c, TYPE_3: degree 31, separation 3)."""

    def __init__(self, seed: int = 1):
        seed &= 0xFFFFFFFF
        if seed == 0:
            seed = 1
        word = seed - (1 << 32) if seed >= 1 << 31 else seed   # int32_t
        r = [word & 0xFFFFFFFF]
        for _ in range(1, 31):
            hi = abs(word) // 127773 * (1 if word >= 0 else -1)  # C division: truncation toward zero
            lo = word - hi * 127773
            word = 16807 * lo - 2836 * hi
            if word < 0:
                word += 2147483647
            r.append(word & 0xFFFFFFFF)
        self.r, self.pos = r, 3
        for _ in range(310):
            self.rand()

    def rand(self) -> int:
        a, b = self.pos, (self.pos + 28) % 31
        v = (self.r[a] + self.r[b]) & 0xFFFFFFFF
        self.r[a] = v
        self.pos = (self.pos + 1) % 31
        return v >> 1


def _kmat(K):
    K = np.asarray(K, dtype=np.float64)
    if K.size == 4:
        fx, fy, cx, cy = K
        K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    return K.reshape(3, 3)


def quad_geometry(kf_left, kf_right, row_ptr, cf_left, cf_right, K_left, R21, T21):
    """n x 12: Gamma, Gamma_bar, T, T_bar per quad in CSR order (get_Gammas_and_Tangents_From_Quads :28-66)."""
    K = _kmat(K_left)
    rows = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    a = orc.finalize_pairs(K, K, R21, T21, np.asarray(kf_left)[rows], np.asarray(kf_right)[rows])
    b = orc.finalize_pairs(K, K, R21, T21, cf_left, cf_right)
    return np.concatenate([a[:, 6:9], b[:, 6:9], a[:, 9:12], b[:, 9:12]], axis=1)


def rank_order(row_ptr):
    """CSR index per rank position: ascending row length, then KF index, then candidate index (:90-103)."""
    row_ptr = np.asarray(row_ptr)
    lens = np.diff(row_ptr)
    rows = np.repeat(np.arange(len(lens)), lens)
    n = int(row_ptr[-1])
    return np.lexsort((np.arange(n), rows, lens[rows])).astype(np.int32)


def _div(a, b):
    """IEEE a / b of two Python floats (Python raises on a zero divisor)."""
    if b != 0.0:
        return a / b
    if a == 0.0 or math.isnan(a):
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _normalized(v):
    z = _dot(v, v)
    if z > 0:
        s = math.sqrt(z)
        return (v[0] / s, v[1] / s, v[2] / s)
    return v


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _mv(M, v):
    return tuple((M[i * 3] * v[0] + M[i * 3 + 1] * v[1]) + M[i * 3 + 2] * v[2] for i in range(3))


def constraints(q1, q2, tau):
    """Apply_Normalized_Length / T1 / T2 / Tangent_Angle_Similarity_Constraint (:108-134) in order"""
    G1, Gb1, T1, Tb1 = q1[0:3], q1[3:6], q1[6:9], q1[9:12]
    G2, Gb2, T2, Tb2 = q2[0:3], q2[3:6], q2[6:9], q2[9:12]
    d12, d12b = _sub(G1, G2), _sub(Gb1, Gb2)
    lG, lGb = math.sqrt(_dot(d12, d12)), math.sqrt(_dot(d12b, d12b))
    if not (_div(abs(lG - lGb), lG) < tau[0]):
        return False
    d21, d21b = _sub(G2, G1), _sub(Gb2, Gb1)
    n21, n21b = math.sqrt(_dot(d21, d21)), math.sqrt(_dot(d21b, d21b))
    c, cb = _div(_dot(d21, T1), n21), _div(_dot(d21b, Tb1), n21b)
    if not (abs(abs(c) - abs(cb)) < tau[1]):
        return False
    c, cb = _div(_dot(d21, T2), n21), _div(_dot(d21b, Tb2), n21b)
    if not (abs(abs(c) - abs(cb)) < tau[2]):
        return False
    c, cb = _dot(T1, T2), _dot(Tb1, Tb2)
    return abs(abs(c) - abs(cb)) < tau[3]


def pose_from_pair(q1, q2):
    """estimate_Pose_From_a_Quad_Pair (:136-153): R (row-major, 9), t"""
    G1, Gb1, T1, Tb1 = q1[0:3], q1[3:6], q1[6:9], q1[9:12]
    e1 = _normalized(_sub(q2[0:3], G1))
    e1b = _normalized(_sub(q2[3:6], Gb1))
    s, sb = _dot(e1, T1), _dot(e1b, Tb1)
    e2 = _normalized(tuple(T1[i] - s * e1[i] for i in range(3)))
    e2b = _normalized(tuple(Tb1[i] - sb * e1b[i] for i in range(3)))
    e3, e3b = _cross(e1, e2), _cross(e1b, e2b)
    R = tuple((e1b[i] * e1[j] + e2b[i] * e2[j]) + e3b[i] * e3[j] for i in range(3) for j in range(3))
    RG = _mv(R, G1)
    t = tuple(Gb1[i] - RG[i] for i in range(3))
    return R, t


def inliers(R, t, G, cf_xy, K, thr):
    """score_Pose_Hypothesis (:155-173) over every quad: one numpy ufunc per operation"""
    with np.errstate(all="ignore"):
        h = [np.add(np.add(R[i * 3] * G[:, 0], R[i * 3 + 1] * G[:, 1]), R[i * 3 + 2] * G[:, 2]) + t[i] for i in range(3)]
        p = [np.add(np.add(K[i * 3] * h[0], K[i * 3 + 1] * h[1]), K[i * 3 + 2] * h[2]) for i in range(3)]
        dx = p[0] / p[2] - cf_xy[:, 0]
        dy = p[1] / p[2] - cf_xy[:, 1]
        return np.sqrt(dx * dx + dy * dy) < thr


def estimate_pose(kf_left, kf_right, row_ptr, cf_left, cf_right, K_left, R21, T21, rng=None, **params):
    """The whole search.  rng: a GlibcRand to continue (continue_stream), else one seeded with rand_seed.  Returns the
    fields of ebvo_pose_result plus inlier, quad_geom, rank_order and the generator."""
    p = dict(DEFAULTS, **params)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    n = int(row_ptr[-1])
    if rng is None:
        rng = GlibcRand(p["rand_seed"])
    top_n = int(p["top_rank_fraction"] * float(n))
    out = dict(status=0, found=False, n_quads=n, top_n=top_n, iterations=0, draws=0, hypotheses=0, best_inliers=0,
               dynamic_max_iter=p["max_iterations"], inlier_ratio=0.0, best_q1=-1, best_q2=-1, R=np.eye(3), t=np.zeros(3),
               inlier=np.zeros(n, dtype=np.uint8), quad_geom=None, rank_order=None, rng=rng)
    if n < 2 or top_n < 2:
        out["status"] = 1
        return out
    K = tuple(_kmat(K_left).reshape(9).tolist())
    geom = quad_geometry(kf_left, kf_right, row_ptr, cf_left, cf_right, K_left, R21, T21)
    order = rank_order(row_ptr)
    out.update(quad_geom=geom, rank_order=order)
    G = np.ascontiguousarray(geom[:, 0:3])
    cf_xy = np.stack([np.asarray(cf_left)["x"], np.asarray(cf_left)["y"]], axis=1)
    rows = [tuple(r) for r in geom.tolist()]
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
        while True:
            i1 = rng.rand() % top_n
            i2 = rng.rand() % top_n
            if i1 != i2:
                break
        draws += 1
        q1, q2 = rows[order[i1]], rows[order[i2]]
        if not constraints(q1, q2, tau):
            it = it - 1 if it > 0 else 0
            it += 1
            continue
        hyps += 1
        R, t = pose_from_pair(q1, q2)
        c = int(inliers(R, t, G, cf_xy, K, thr).sum())
        if c > best:
            best, ratio, best_rt = c, c / n, (R, t)
            out["best_q1"], out["best_q2"] = i1, i2
        if ratio >= 0.95:
            dyn = min_it
        elif ratio <= 0.05:
            dyn = max_it
        else:
            prob_outlier = 1.0 - ratio * ratio       # std::pow(ratio, 2) compiles to ratio * ratio
            v = log_prob_missing_model / math.log(prob_outlier) * p["dyn_num_trials_mult"]
            v = 0 if not (v > 0) else min(math.ceil(v), 1 << 62) if math.isfinite(v) else 1 << 62
            dyn = v
        it += 1
    out.update(status=status, iterations=it, draws=draws, hypotheses=hyps, best_inliers=best, dynamic_max_iter=dyn,
               inlier_ratio=ratio, found=best > 0)
    if best > 0:
        R, t = best_rt
        out["R"], out["t"] = np.array(R).reshape(3, 3), np.array(t)
        out["inlier"] = inliers(R, t, G, cf_xy, K, thr).astype(np.uint8)
    return out


# ---- synthetic quads of a known motion ---------------------------------------------------------------------------------

def rot(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(angle) * k + (1 - math.cos(angle)) * (k @ k)


def _edge(K, X, D):
    """image edge of the 3-D point X with tangent D (camera frame): location and orientation of the projected tangent"""
    x = K[0, 0] * X[:, 0] / X[:, 2] + K[0, 2]
    y = K[1, 1] * X[:, 1] / X[:, 2] + K[1, 2]
    tx = K[0, 0] * (D[:, 0] * X[:, 2] - X[:, 0] * D[:, 2])
    ty = K[1, 1] * (D[:, 1] * X[:, 2] - X[:, 1] * D[:, 2])
    e = np.zeros(len(X), dtype=EDGE_DTYPE)
    e["x"], e["y"], e["theta"] = x, y, np.arctan2(ty, tx)
    return e


def synthetic_quads(n_quads, outlier_frac, calib, R_gt, t_gt, seed=0, multi=0.2):
    """Quads of a known motion X_cf = R_gt X_kf + t_gt.  calib = (K_left 3x3, R21, T21); K_right := K_left.  Rows (KF mates)
    hold one or two quads (a share `multi` of the rows holds two); int(outlier_frac * n) quads have their CF left and right
    centres moved by 5-12 px.  Only points whose reconstructed tangent keeps its sign under the motion are used (tangents
    away from the epipolar planes).  Returns (kf_left, kf_right, row_ptr, cf_left, cf_right, inlier mask in CSR order)."""
    K, R21, T21 = _kmat(calib[0]), np.asarray(calib[1], dtype=np.float64).reshape(3, 3), np.asarray(calib[2], dtype=np.float64)
    rng = np.random.default_rng(seed)
    w, h = 2 * K[0, 2], 2 * K[1, 2]
    # row lengths: first the rows, then which quads are outliers
    lens = []
    while sum(lens) < n_quads:
        lens.append(2 if rng.random() < multi and sum(lens) + 2 <= n_quads else 1)
    n_kf = len(lens)
    Xs, Ds = [], []
    while sum(len(x) for x in Xs) < n_kf:
        m = 4 * n_kf + 16
        z = rng.uniform(4.0, 30.0, m)
        u, v = rng.uniform(0.05 * w, 0.95 * w, m), rng.uniform(0.05 * h, 0.95 * h, m)
        X = np.stack([(u - K[0, 2]) * z / K[0, 0], (v - K[1, 2]) * z / K[1, 1], z], axis=1)
        D = rng.normal(size=(m, 3))
        D[:, 1] += 2.0 * np.sign(D[:, 1])          # mostly vertical: away from the (horizontal) epipolar planes
        D /= np.linalg.norm(D, axis=1, keepdims=True)
        Xc, Dc = X @ R_gt.T + t_gt, D @ R_gt.T
        ok = Xc[:, 2] > 1.0
        kfL, kfR = _edge(K, X, D), _edge(K, X @ R21.T + T21, D @ R21.T)
        cfL, cfR = _edge(K, Xc, Dc), _edge(K, Xc @ R21.T + T21, Dc @ R21.T)
        a = orc.finalize_pairs(K, K, R21, T21, kfL, kfR)
        b = orc.finalize_pairs(K, K, R21, T21, cfL, cfR)
        same = np.einsum("ij,ij->i", a[:, 9:12] @ R_gt.T, b[:, 9:12]) > 0.999
        good = ok & same & (np.abs(a[:, 6:9] - X).max(axis=1) < 1e-6)
        Xs.append(X[good])
        Ds.append(D[good])
    X, D = np.concatenate(Xs)[:n_kf], np.concatenate(Ds)[:n_kf]
    Xc, Dc = X @ R_gt.T + t_gt, D @ R_gt.T
    kfL, kfR = _edge(K, X, D), _edge(K, X @ R21.T + T21, D @ R21.T)
    cfL0, cfR0 = _edge(K, Xc, Dc), _edge(K, Xc @ R21.T + T21, Dc @ R21.T)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    rows = np.repeat(np.arange(n_kf), lens)
    cfL, cfR = cfL0[rows].copy(), cfR0[rows].copy()
    n = len(rows)
    inl = np.ones(n, dtype=np.uint8)
    # the second quad of a two-quad row is an outlier first (its KF mate has its true match), then random ones
    second = np.flatnonzero(np.concatenate([[False], rows[1:] == rows[:-1]]))
    n_out = int(outlier_frac * n)
    pool = np.concatenate([rng.permutation(second), rng.permutation(np.setdiff1d(np.arange(n), second))])
    out_idx = pool[:n_out]
    # rows whose every quad would be an outlier are fine: the KF mate simply has no true match
    inl[out_idx] = 0
    ang = rng.uniform(0, 2 * math.pi, len(out_idx))
    r = rng.uniform(5.0, 12.0, len(out_idx))
    for e in (cfL, cfR):
        e["x"][out_idx] += r * np.cos(ang)
        e["y"][out_idx] += r * np.sin(ang)
    # a plain inlier in a two-quad row: the outlier twin differs, nothing else to do; an inlier twin of an inlier would be
    # a duplicate quad (zero length: every pair of them is rejected), so twins that stayed inliers are moved off as well
    twin_in = second[inl[second] == 1]
    if len(twin_in):
        inl[twin_in] = 0
        ang = rng.uniform(0, 2 * math.pi, len(twin_in))
        for e in (cfL, cfR):
            e["x"][twin_in] += 7.0 * np.cos(ang)
            e["y"][twin_in] += 7.0 * np.sin(ang)
    return kfL, kfR, row_ptr, cfL, cfR, inl
