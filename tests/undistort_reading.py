"""A second reading of cv::undistort (OpenCV 4.x: modules/calib3d/src/undistort.dispatch.cpp cv::undistort + the scalar loop
of initUndistortRectifyMap with CV_16SC2 maps, modules/imgproc/src/imgwarp.cpp remapBilinear, 8-bit, BORDER_CONSTANT 0), as
DESIGN.md section 2 and the header of oracle/ebvo_oracle.c: orc_undistort describe it -- written from that description, in
Python doubles (IEEE binary64, one rounding per operation, no contraction), sharing no code with the C restatement:

  - stripes of max(1, 4096 / cols) rows, clipped to the image; every stripe has its own camera matrix (cy - y0), inverted
    with the closed 3 x 3 form of cv::invert;
  - along a row (_x, _y, _w) advance by SEQUENTIAL ADDITION of the inverse's first column (a plain loop: the running sum is
    not j * step);
  - the distortion polynomial in the written operation order (k4 .. k6, s1 .. s4 and the tilt are zero / identity and stay
    in the expressions, as in the source);
  - u, v -> cvRound(u * 32) with saturation, `>> 5` and `& 31` on the two's complement value, the (short) cast of the
    CV_16SC2 map;
  - integer bilinear weights (exact, sum 2^15), taps outside the image read 0, (acc + 2^14) >> 15.

Besides the image it returns how many pixels fall in each class of source position, so that a test case can state which
branch it reaches (tests/undistort_cases.py)."""
import numpy as np

INT_MIN, INT_MAX = -2147483648, 2147483647


def inv3x3(a):
    d = a[0] * (a[4] * a[8] - a[5] * a[7]) - a[1] * (a[3] * a[8] - a[5] * a[6]) + a[2] * (a[3] * a[7] - a[4] * a[6])
    d = 1.0 / d
    return [(a[4] * a[8] - a[5] * a[7]) * d, (a[2] * a[7] - a[1] * a[8]) * d, (a[1] * a[5] - a[2] * a[4]) * d,
            (a[5] * a[6] - a[3] * a[8]) * d, (a[0] * a[8] - a[2] * a[6]) * d, (a[2] * a[3] - a[0] * a[5]) * d,
            (a[3] * a[7] - a[4] * a[6]) * d, (a[1] * a[6] - a[0] * a[7]) * d, (a[0] * a[4] - a[1] * a[3]) * d]


def cv_round_sat(v):
    """saturate_cast<int>(double): round half to even inside the int range, the nearest end outside it (NaN -> INT_MIN).
    Returns (values as int64, saturated flags)."""
    low = ~(v > -2147483648.0)
    high = ~low & ~(v < 2147483647.0)
    safe = np.where(low | high, 0.0, v)
    r = np.rint(safe).astype(np.int64)
    r[low] = INT_MIN
    r[high] = INT_MAX
    return r, low | high


def to_short(v):
    return ((v + 32768) & 0xFFFF) - 32768


def stripe_height(h, w):
    return min(max(1, 4096 // max(w, 1)), h)


def undistort(img, K, dist):
    """(image, counts).  K = (fx, fy, cx, cy), dist = k1 k2 p1 p2 [k3]."""
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape
    fx, fy, u0, v0 = (float(v) for v in K)
    d = [float(v) for v in dist] + [0.0] * (5 - len(dist))
    k1, k2, p1, p2, k3 = d
    k4 = k5 = k6 = s1 = s2 = s3 = s4 = 0.0
    ss0 = stripe_height(h, w)
    out = np.zeros((h, w), dtype=np.uint8)
    src = img.astype(np.int64)
    names = ("inside", "left", "right", "top", "bottom", "none", "wrapped", "saturated", "wrapped_reading")
    counts = dict.fromkeys(names, 0)
    row_y = np.zeros(h)
    none_mask = np.zeros((h, w), dtype=bool)
    stripes = []
    with np.errstate(all="ignore"):
        for y0 in range(0, h, ss0):
            ss = min(ss0, h - y0)
            stripes.append(ss)
            ir = inv3x3([fx, 0.0, u0, 0.0, fy, v0 - y0, 0.0, 0.0, 1.0])
            for i in range(ss):
                _x, _y, _w = i * ir[1] + ir[2], i * ir[4] + ir[5], i * ir[7] + ir[8]
                row_y[y0 + i] = _y
                xs, ys, ws = np.empty(w), np.empty(w), np.empty(w)
                for j in range(w):
                    xs[j], ys[j], ws[j] = _x, _y, _w
                    _x += ir[0]
                    _y += ir[3]
                    _w += ir[6]
                ww = 1.0 / ws
                x, y = xs * ww, ys * ww
                x2, y2 = x * x, y * y
                r2, _2xy = x2 + y2, 2 * x * y
                kr = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
                xd = x * kr + p1 * _2xy + p2 * (r2 + 2 * x2) + s1 * r2 + s2 * r2 * r2
                yd = y * kr + p1 * (r2 + 2 * y2) + p2 * _2xy + s3 * r2 + s4 * r2 * r2
                t0 = 1.0 * xd + 0.0 * yd + 0.0 * 1.0
                t1 = 0.0 * xd + 1.0 * yd + 0.0 * 1.0
                t2 = 0.0 * xd + 0.0 * yd + 1.0 * 1.0
                inv_proj = np.where(t2 != 0, 1.0 / t2, 1.0)
                u = fx * inv_proj * t0 + u0
                v = fy * inv_proj * t1 + v0
                iu, su = cv_round_sat(u * 32)
                iv, sv = cv_round_sat(v * 32)
                qx, qy = iu >> 5, iv >> 5
                sx, sy = to_short(qx), to_short(qy)
                fxi, fyi = iu & 31, iv & 31
                w00, w01 = (32 - fyi) * (32 - fxi) * 32, (32 - fyi) * fxi * 32
                w10, w11 = fyi * (32 - fxi) * 32, fyi * fxi * 32
                cx0, cx1 = (sx >= 0) & (sx < w), (sx + 1 >= 0) & (sx + 1 < w)
                ry0, ry1 = (sy >= 0) & (sy < h), (sy + 1 >= 0) & (sy + 1 < h)

                def tap(yy, xx, ok):
                    return np.where(ok, src[np.where(ok, yy, 0), np.where(ok, xx, 0)], 0)

                acc = (tap(sy, sx, cx0 & ry0) * w00 + tap(sy, sx + 1, cx1 & ry0) * w01 +
                       tap(sy + 1, sx, cx0 & ry1) * w10 + tap(sy + 1, sx + 1, cx1 & ry1) * w11)
                out[y0 + i] = np.clip((acc + (1 << 14)) >> 15, 0, 255).astype(np.uint8)
                anyx, anyy = cx0 | cx1, ry0 | ry1
                some = anyx & anyy
                sat = su | sv
                wrapped = ~sat & ((qx != sx) | (qy != sy))
                none_mask[y0 + i] = ~some
                counts["inside"] += int((cx0 & cx1 & ry0 & ry1).sum())
                counts["none"] += int((~some).sum())
                counts["left"] += int((some & cx1 & ~cx0).sum())
                counts["right"] += int((some & cx0 & ~cx1).sum())
                counts["top"] += int((some & ry1 & ~ry0).sum())
                counts["bottom"] += int((some & ry0 & ~ry1).sum())
                counts["saturated"] += int(sat.sum())
                counts["wrapped"] += int(wrapped.sum())
                counts["wrapped_reading"] += int((wrapped & some).sum())
                if sat.any():
                    counts.setdefault("saturated_sx", set()).update(int(t) for t in np.unique(sx[su]))
                    counts.setdefault("saturated_sy", set()).update(int(t) for t in np.unique(sy[sv]))
    counts["ss0"] = ss0
    counts["stripes"] = stripes
    counts["row_y"] = row_y
    counts["none_mask"] = none_mask
    return out, counts
