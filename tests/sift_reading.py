"""A second reading of the fixed-scale SIFT descriptor (OpenCV 4.x: createInitialImage / GaussianBlur for the base level,
sift.simd.hpp calcSIFTDescriptor for the descriptor; the +-8 px keypoints of src/Stereo_Matches.cpp:655-689 and the
min-of-four distance of :736-740), written from the published algorithm in numpy float32 and sharing no code with
oracle/ebvo_oracle.c or csrc/ebvo_math.h:

  - base level: float image, 13-tap Gaussian of sigma sqrt(1.6^2 - 0.5^2), row pass with the taps in ascending order,
    column pass centre first and then the symmetric pairs, reflect-101 borders;
  - descriptor: OpenCV's flat (d + 2)(d + 2)(n + 2) histogram addressed by its flat index; the reference's orientations of
    -180 .. 180 degrees leave o0 negative after the single `+= n`, and OpenCV then indexes the previous cell -- kept; a
    NEGATIVE flat index (in front of the array) is dropped explicitly, never through Python's negative indexing;
  - expf and fastAtan2 restated in np.float32 from their formulas; sin / cos from the oracle's correctly rounded pair.

Every float32 operation below is one numpy float32 operation (one rounding, no contraction), applied to all keypoints at
once; the loop over the 11 x 11 samples and the eight votes of a sample is sequential, so every histogram bin receives its
addends in sample order."""
import math

import numpy as np

from tests import oracle as orc

F = np.float32
D, N = 4, 8
FLT_EPS = F(1.1920928955078125e-07)


def expf(x):
    """exp(x) by Cody-Waite reduction (ln 2 = 0.693359375 - 2.12194440e-4) and the degree-6 Taylor polynomial"""
    x = np.asarray(x, dtype=F)
    with np.errstate(all="ignore"):
        fk = x * F(1.44269504088896341)
        half = np.where(fk >= F(0), F(0.5), F(-0.5)).astype(F)
        k = np.trunc(np.where(np.isfinite(fk), fk + half, F(0))).astype(np.int32)
        dk = k.astype(F)
        r = (x - dk * F(0.693359375)) - dk * F(-2.12194440e-4)
        p = F(1) / F(720)
        p = p * r + F(1) / F(120)
        p = p * r + F(1) / F(24)
        p = p * r + F(1) / F(6)
        p = p * r + F(0.5)
        p = p * r + F(1)
        p = p * r + F(1)
        v = np.ldexp(p.astype(F), k).astype(F)
        v = np.where(x < F(-87), F(0), v)
        v = np.where(x > F(88), F(np.inf), v)
        return np.where(x != x, x, v).astype(F)


def fast_atan2_deg(y, x):
    """OpenCV's fastAtan2 (modules/core/src/mathfuncs_core.simd.hpp: atan_f32), degrees"""
    y, x = np.asarray(y, dtype=F), np.asarray(x, dtype=F)
    scale = F(180 / math.pi)
    p1, p3 = F(0.9997878412794807) * scale, F(-0.3258083974640975) * scale
    p5, p7 = F(0.1555786518463281) * scale, F(-0.04432655554792128) * scale
    eps = F(2.2204460492503131e-16)
    with np.errstate(all="ignore"):
        ax, ay = np.abs(x), np.abs(y)
        xs = ax >= ay
        c = np.where(xs, ay, ax) / (np.where(xs, ax, ay) + eps)
        c2 = c * c
        t = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
        a = np.where(xs, t, F(90) - t)
        a = np.where(x < 0, F(180) - a, a)
        a = np.where(y < 0, F(360) - a, a)
    return a.astype(F)


def kernel13():
    sigma = F(1.6)
    v = sigma * sigma - F(0.5) * F(0.5)
    sd = np.sqrt(v if v > F(0.01) else F(0.01))
    assert sd.dtype == F
    sigma_x = float(sd)
    scale2x = -0.5 / (sigma_x * sigma_x)
    kd = [math.exp(scale2x * (i - 6.0) * (i - 6.0)) for i in range(13)]
    total = 0.0
    for t in kd:
        total += t
    total = 1.0 / total
    return np.array([t * total for t in kd]).astype(F)


def reflect101(p, n):
    if n == 1:
        return 0
    while p < 0 or p >= n:
        p = -p if p < 0 else 2 * (n - 1) - p
    return p


def base_level(img):
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape
    k = kernel13()
    f = img.astype(F)
    cols = [np.array([reflect101(x - 6 + t, w) for x in range(w)]) for t in range(13)]
    tmp = f[:, cols[0]] * k[0]
    for t in range(1, 13):
        tmp = tmp + f[:, cols[t]] * k[t]
    out = k[6] * tmp
    for t in range(1, 7):
        dn = np.array([reflect101(y + t, h) for y in range(h)])
        up = np.array([reflect101(y - t, h) for y in range(h)])
        out = out + k[6 + t] * (tmp[dn] + tmp[up])
    assert out.dtype == F
    return out


COUNTERS = ("samples", "o0_negative", "dropped_in_front", "clipped", "saturated", "equal_255", "all_zero")


def descriptors(img, edges):
    """((n, 2, 128) float32, counters)"""
    img = np.asarray(img, dtype=np.uint8)
    rows, cols = img.shape
    base = base_level(img)
    e = np.asarray(edges, dtype=orc.EDGE_DTYPE)
    n_e = len(e)
    cnt = dict.fromkeys(COUNTERS, 0)
    if n_e == 0:
        return np.zeros((0, 2, 128), dtype=F), cnt
    theta = e["theta"].astype(np.float64)
    sn, cs = orc.sincos_v(theta, orc.PORTABLE)
    # the two points 8 px along the normal: (x + 8 sin, y - 8 cos), then (x - 8 sin, y + 8 cos); cv::KeyPoint holds floats
    px_d = np.stack([e["x"] + 8 * sn, e["x"] + 8 * (-sn)], 1).reshape(-1)
    py_d = np.stack([e["y"] + 8 * (-cs), e["y"] + 8 * cs], 1).reshape(-1)
    with np.errstate(all="ignore"):
        ptx, pty = px_d.astype(F), py_d.astype(F)
        kp_angle = np.repeat((180 / math.pi * theta).astype(F), 2)
        ori = F(360) - kp_angle
        ori = np.where(np.abs(ori - F(360)) < FLT_EPS, F(0), ori).astype(F)
        px, py = np.rint(ptx).astype(np.int64), np.rint(pty).astype(np.int64)
        arg = ori * F(math.pi / 180)
        s64, c64 = orc.sincos_v(arg.astype(np.float64), orc.PORTABLE)
        cos_t, sin_t = c64.astype(F), s64.astype(F)
        bins_per_rad = F(N) / F(360)
        exp_scale = F(-1) / (F(D * D) * F(0.5))
        hist_width = F(3) * F(0.5)
        radius = int(np.rint(hist_width * F(1.4142135623730951) * F(D + 1) * F(0.5)))
        radius = min(radius, int(math.sqrt(float(cols) * cols + float(rows) * rows)))
        cos_t = cos_t / hist_width
        sin_t = sin_t / hist_width
        n_kp = 2 * n_e
        hist = np.zeros((n_kp, (D + 2) * (D + 2) * (N + 2)), dtype=F)
        for i in range(-radius, radius + 1):
            for j in range(-radius, radius + 1):
                c_rot = F(j) * cos_t - F(i) * sin_t
                r_rot = F(j) * sin_t + F(i) * cos_t
                rbin = r_rot + F(D // 2) - F(0.5)
                cbin = c_rot + F(D // 2) - F(0.5)
                r, c = py + i, px + j
                ok = ((rbin > -1) & (rbin < D) & (cbin > -1) & (cbin < D) & (r > 0) & (r < rows - 1) & (c > 0) &
                      (c < cols - 1))
                sel = np.flatnonzero(ok)
                if len(sel) == 0:
                    continue
                r, c, rbin, cbin, c_rot, r_rot = r[sel], c[sel], rbin[sel], cbin[sel], c_rot[sel], r_rot[sel]
                dx = base[r, c + 1] - base[r, c - 1]
                dy = base[r - 1, c] - base[r + 1, c]
                wexp = (c_rot * c_rot + r_rot * r_rot) * exp_scale
                Ori = fast_atan2_deg(dy, dx)
                Mag = np.sqrt(dx * dx + dy * dy)
                W = expf(wexp)
                obin = (Ori - ori[sel]) * bins_per_rad
                mag = Mag * W
                r0, c0, o0 = (np.floor(v).astype(np.int64) for v in (rbin, cbin, obin))
                rbin = rbin - r0.astype(F)
                cbin = cbin - c0.astype(F)
                obin = obin - o0.astype(F)
                o0 = np.where(o0 < 0, o0 + N, o0)
                o0 = np.where(o0 >= N, o0 - N, o0)
                v_r1 = mag * rbin
                v_r0 = mag - v_r1
                v_rc11 = v_r1 * cbin
                v_rc10 = v_r1 - v_rc11
                v_rc01 = v_r0 * cbin
                v_rc00 = v_r0 - v_rc01
                v_rco111 = v_rc11 * obin
                v_rco110 = v_rc11 - v_rco111
                v_rco101 = v_rc10 * obin
                v_rco100 = v_rc10 - v_rco101
                v_rco011 = v_rc01 * obin
                v_rco010 = v_rc01 - v_rco011
                v_rco001 = v_rc00 * obin
                v_rco000 = v_rc00 - v_rco001
                assert v_rco000.dtype == F and obin.dtype == F and mag.dtype == F
                idx = ((r0 + 1) * (D + 2) + c0 + 1) * (N + 2) + o0
                cnt["samples"] += len(sel)
                cnt["o0_negative"] += int((o0 < 0).sum())
                for off, val in ((0, v_rco000), (1, v_rco001), (N + 2, v_rco010), (N + 3, v_rco011),
                                 ((D + 2) * (N + 2), v_rco100), ((D + 2) * (N + 2) + 1, v_rco101),
                                 ((D + 3) * (N + 2), v_rco110), ((D + 3) * (N + 2) + 1, v_rco111)):
                    at = idx + off
                    keep = at >= 0                       # in front of the array: dropped, explicitly
                    cnt["dropped_in_front"] += int((~keep).sum())
                    assert (at[keep] < hist.shape[1]).all()
                    hist[sel[keep], at[keep]] += val[keep]
        # circular orientation histogram, then the d x d x n interior
        raw = np.zeros((n_kp, D * D * N), dtype=F)
        for i in range(D):
            for j in range(D):
                idx = ((i + 1) * (D + 2) + (j + 1)) * (N + 2)
                hist[:, idx] += hist[:, idx + N]
                hist[:, idx + 1] += hist[:, idx + N + 1]
                for k in range(N):
                    raw[:, (i * D + j) * N + k] = hist[:, idx + k]
        nrm2 = np.zeros(n_kp, dtype=F)
        for k in range(D * D * N):
            nrm2 = nrm2 + raw[:, k] * raw[:, k]
        thr = np.sqrt(nrm2) * F(0.2)
        nrm2 = np.zeros(n_kp, dtype=F)
        for k in range(D * D * N):
            val = np.where(raw[:, k] < thr, raw[:, k], thr)
            cnt["clipped"] += int((raw[:, k] > thr).sum())
            raw[:, k] = val
            nrm2 = nrm2 + val * val
        sq = np.sqrt(nrm2)
        scale = F(512) / np.where(sq > FLT_EPS, sq, FLT_EPS)
        assert scale.dtype == F
        v = np.rint(raw * scale[:, None]).astype(np.int64)
        cnt["saturated"] = int((v > 255).sum())
        out = np.clip(v, 0, 255)
        cnt["equal_255"] = int((out == 255).sum())
        cnt["all_zero"] = int((out == 0).all(axis=1).sum())
    return out.astype(F).reshape(n_e, 2, 128), cnt


def min_distances(left_desc, cand_desc, row_ptr):
    """min of the four L2 distances (L1,R1), (L2,R1), (L1,R2), (L2,R2): float differences, squares summed in double"""
    left = np.asarray(left_desc, dtype=F).reshape(-1, 2, 128)
    cand = np.asarray(cand_desc, dtype=F).reshape(-1, 2, 128)
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    row = np.repeat(np.arange(len(row_ptr) - 1), np.diff(row_ptr))
    best = np.zeros(len(cand))
    for t in range(4):
        a, b = left[row, t & 1], cand[:, t >> 1]
        s = np.zeros(len(cand))
        for q in range(128):
            v = (a[:, q] - b[:, q]).astype(np.float64)
            s = s + v * v
        dd = np.sqrt(s)
        best = dd if t == 0 else np.where(dd < best, dd, best)
    return best
