"""Synthetic edge lists for the chunk marks of the candidate walk (match_kernels.hip: candidates_kernel, step 3), and the
marks themselves recomputed in numpy.

A left edge marks the staged chunks of right edges it has to walk either by testing the chunk box against its own region
box (the fast mark: both the epipolar and the disparity stage enabled and the edge `flat`) or against the line itself
(box_may_match).  Neither may lose a chunk that holds a passing pair, and the CSR must not depend on which one ran.  A
case is one list of 130 left edges (three tiles of 64, the last one partial) whose epipolar lines cycle through eight
kinds -- so that every wave of the walk, which takes eight consecutive left edges per round, holds all of them --, and
about 1,100 right edges (three groups of 64 chunks) in raster order: a dense grid around the lines, so that the first
tile's union of regions selects more than 64 chunks (two staging batches), plus, for the first edges of every kind, points
at |dx| = max_disp exactly and one ulp either side, at distance epi_thr from the line and one ulp either side, and on the
boundary of the edge's region box.  Two parameter sets: the defaults, and a wide one whose rows pass 64 candidates (the
fill pass redoes the tile).

The numpy functions follow the device code operation for operation in binary64 (no contraction on either side), so the
flags and marks computed here are the kernel's; the tests only rely on them being conservative.
"""
import functools

import numpy as np

from edge_based_visual_odometry_amd._lib import EDGE_DTYPE

CHUNK, GROUP, TILE, STAGE = 8, 64, 64, 64
BOX_SLACK = 1e-6
FLAT_BANDS = 4.0
EPI, DISP, ORIENT = 1, 2, 4
MASKS = (1, 2, 3, 4, 5, 6, 7)
N_LEFT = 130
KINDS = ("a=0", "below flat", "above flat", "45 deg", "b=0", "NaN", "a=b=0", "steep below flat")
PARAMS = {
    "default": dict(epi_thr=0.5, max_disp=25.0, orient_thr_deg=10.0),
    "wide": dict(epi_thr=2.0, max_disp=100.0, orient_thr_deg=10.0),
}


def slacked(p):
    return p["max_disp"] + BOX_SLACK, p["epi_thr"] + BOX_SLACK


def flat_slope(p):
    """tan of the tilt at which an edge stops being flat"""
    D, band = slacked(p)
    return FLAT_BANDS * band / (2.0 * D)


# --- the device code in numpy ----------------------------------------------------------------------------------------
def left_ctx(lines):
    a, b, c = lines[:, 0], lines[:, 1], lines[:, 2]
    with np.errstate(all="ignore"):
        nrm = np.sqrt(a * a + b * b)
        return a / nrm, b / nrm, c / nrm


def region_boxes(L, lines, p, mask):
    """region_box: x0, x1, y0, y1 per left edge"""
    D, band = slacked(p)
    ah, bh, ch = left_ctx(lines)
    n = len(L)
    x0, x1 = np.full(n, -np.inf), np.full(n, np.inf)
    y0, y1 = np.full(n, -np.inf), np.full(n, np.inf)
    if mask & DISP:
        x0, x1, y0, y1 = L["x"] - D, L["x"] + D, L["y"] - D, L["y"] + D
    if (mask & EPI) and (mask & DISP):
        ok = (ah == ah) & (bh == bh) & (ch == ch)
        with np.errstate(all="ignore"):
            m = 1e-9
            s = ok & (np.abs(bh) > m)
            ya, yb = -(ah * x0 + ch) / bh, -(ah * x1 + ch) / bh
            e = band / np.abs(bh) + BOX_SLACK
            y0 = np.where(s, np.fmax(y0, np.fmin(ya, yb) - e), y0)
            y1 = np.where(s, np.fmin(y1, np.fmax(ya, yb) + e), y1)
            s = ok & (np.abs(ah) > m)
            xa, xb = -(bh * y0 + ch) / ah, -(bh * y1 + ch) / ah
            e = band / np.abs(ah) + BOX_SLACK
            x0 = np.where(s, np.fmax(x0, np.fmin(xa, xb) - e), x0)
            x1 = np.where(s, np.fmin(x1, np.fmax(xa, xb) + e), x1)
    return x0, x1, y0, y1


def flat_flags(lines, p, mask):
    """region_is_flat AND both stages enabled: the edges that take the fast mark"""
    if not ((mask & EPI) and (mask & DISP)):
        return np.zeros(len(lines), dtype=bool)
    D, band = slacked(p)
    ah, bh, _ = left_ctx(lines)
    pq = np.abs(ah), np.abs(bh)
    with np.errstate(all="ignore"):
        return 2.0 * D * np.fmin(*pq) <= FLAT_BANDS * band * np.fmax(*pq)


def chunk_boxes(R):
    nch = (len(R) + CHUNK - 1) // CHUNK
    out = np.zeros((4, nch))
    for c in range(nch):
        x, y = R["x"][c * CHUNK:(c + 1) * CHUNK], R["y"][c * CHUNK:(c + 1) * CHUNK]
        out[:, c] = np.fmin.reduce(x), np.fmax.reduce(x), np.fmin.reduce(y), np.fmax.reduce(y)
    return out


def fast_marks(boxes, regions):
    """box_meets_region for every (left edge, chunk)"""
    bx0, bx1, by0, by1 = (b[None, :] for b in boxes)
    rx0, rx1, ry0, ry1 = (r[:, None] for r in regions)
    return ~((bx0 > rx1) | (bx1 < rx0) | (by0 > ry1) | (by1 < ry0))


def line_marks(boxes, L, lines, p, mask):
    """box_may_match for every (left edge, chunk)"""
    D, band = slacked(p)
    ah, bh, ch = (v[:, None] for v in left_ctx(lines))
    xl, yl = L["x"][:, None], L["y"][:, None]
    n = len(L)
    x0, x1, y0, y1 = (np.broadcast_to(b[None, :], (n, boxes.shape[1])) for b in boxes)
    may = np.ones((n, boxes.shape[1]), dtype=bool)
    with np.errstate(all="ignore"):
        if mask & DISP:
            x0, x1, y0, y1 = np.fmax(x0, xl - D), np.fmin(x1, xl + D), np.fmax(y0, yl - D), np.fmin(y1, yl + D)
            may &= ~((x0 > x1) | (y0 > y1))
        if mask & EPI:
            gx0, gx1, gy0, gy1 = ah * x0, ah * x1, bh * y0, bh * y1
            gmin = np.fmin(gx0, gx1) + np.fmin(gy0, gy1) + ch
            gmax = np.fmax(gx0, gx1) + np.fmax(gy0, gy1) + ch
            may &= ~((gmin > band) | (gmax < -band))
    return may


def chunks_of_tile_union(boxes, regions, tile):
    """how many chunks the tile's union of region boxes selects (staged BATCH = 64 at a time)"""
    s = slice(tile * TILE, (tile + 1) * TILE)
    ux0, ux1, uy0, uy1 = regions[0][s].min(), regions[1][s].max(), regions[2][s].min(), regions[3][s].max()
    return int((~((boxes[0] > ux1) | (boxes[1] < ux0) | (boxes[2] > uy1) | (boxes[3] < uy0))).sum())


# --- the cases -------------------------------------------------------------------------------------------------------
def _line(kind, px, py, p, scale):
    """(a, b, c) of the given kind through (px, py)"""
    t = flat_slope(p)
    if kind == "NaN":
        return np.nan, 1.0, -py
    if kind == "a=b=0":
        return 0.0, 0.0, 0.25
    if kind == "a=0":
        return 0.0, scale, -scale * py                     # exact: py is a multiple of 1/8, scale a power of two
    if kind == "b=0":
        return scale, 0.0, -scale * px
    a, b = {"below flat": (t * (1.0 - 1e-6), 1.0), "above flat": (t * (1.0 + 1e-6), 1.0), "45 deg": (1.0, 1.0),
            "steep below flat": (1.0, -t * (1.0 - 1e-6))}[kind]
    a, b = a * scale, b * scale
    return a, b, -(a * px + b * py)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(L, R, lines, kinds, special): `special` lists (left index, what, right index) of the placed boundary points"""
    p = PARAMS[name]
    D0, thr = p["max_disp"], p["epi_thr"]
    L = np.zeros(N_LEFT, dtype=EDGE_DTYPE)
    i = np.arange(N_LEFT)
    L["x"] = 120.0 + 2.5 * i                               # multiples of 0.5: lx - max_disp is exact
    L["y"] = 100.0 + 0.125 * (i % 5)
    L["theta"] = 0.3
    L["index"] = i
    kinds = [KINDS[k % len(KINDS)] for k in range(N_LEFT)]
    lines = np.zeros((N_LEFT, 3))
    for k in range(N_LEFT):
        lines[k] = _line(kinds[k], L["x"][k] - 6.0, L["y"][k] + 0.125, p, 0.0078125)
    pts = []                                               # (x, y, left index or -1, what)
    # the grid: 8 rows one pixel apart around the lines, 120 columns
    for gy in range(8):
        for gx in range(120):
            pts.append((40.0 + gx * 3.75 + 0.25 * (gy % 3), 97.125 + gy, -1, "grid"))
    # boundary points for the first two edges of every kind, under every mask's own region box
    ah, bh, ch = left_ctx(lines)
    reg = {m: region_boxes(L, lines, p, m) for m in (2, 3)}
    for k in range(2 * len(KINDS)):
        lx, ly = L["x"][k], L["y"][k]
        u = np.spacing(max(lx, D0))                        # the ulp of the coarsest of lx, rx and max_disp: lx - rx is exact
        for rx in (lx - D0, lx - D0 + u, lx - D0 - u):
            pts.append((rx, ly, k, "disparity"))           # dy = 0: max_disp exactly, one ulp less, one ulp more
        if np.isfinite(ah[k]) and np.isfinite(bh[k]) and np.isfinite(ch[k]):
            # the foot of the line near the edge, moved along the normal by epi_thr
            d = ah[k] * (lx - 6.0) + bh[k] * ly + ch[k]
            fx, fy = (lx - 6.0) - d * ah[k], ly - d * bh[k]
            qx, qy = fx + thr * ah[k], fy + thr * bh[k]
            for s in (0, -1, 1):
                if abs(bh[k]) >= abs(ah[k]):
                    pts.append((qx, qy if s == 0 else np.nextafter(qy, s * np.inf), k, "band"))
                else:
                    pts.append((qx if s == 0 else np.nextafter(qx, s * np.inf), qy, k, "band"))
        for m, (x0, x1, y0, y1) in reg.items():
            xm, ym = 0.5 * (x0[k] + x1[k]), 0.5 * (y0[k] + y1[k])
            for q in ((x0[k], ym), (x1[k], ym), (xm, y0[k]), (xm, y1[k]), (x0[k], y0[k]), (x1[k], y1[k])):
                if np.isfinite(q[0]) and np.isfinite(q[1]):
                    pts.append((q[0], q[1], k, "region"))
    # raster order, as TOED lists its edges: by pixel row, then by x
    pts.sort(key=lambda q: (np.floor(q[1]), q[0], q[1]))
    R = np.zeros(len(pts), dtype=EDGE_DTYPE)
    R["x"] = [q[0] for q in pts]
    R["y"] = [q[1] for q in pts]
    k = np.arange(len(pts))
    R["theta"] = np.where(k % 5 == 4, 1.5, 0.3 + 0.05 * (k % 3 - 1))   # every fifth fails the orientation gate
    R["index"] = k
    special = [(q[2], q[3], j) for j, q in enumerate(pts) if q[2] >= 0]
    return dict(L=L, R=R, lines=lines, kinds=kinds, special=special, params=p)


@functools.lru_cache(maxsize=None)
def reference(name, mask):
    """the oracle's CSR of a case under a stage mask: computed once, shared, read-only"""
    from tests import oracle as orc
    c = case(name)
    rp, ci = orc.epi_candidates(c["L"], c["R"], c["lines"], stage_mask=mask, **c["params"])
    rp.setflags(write=False)
    ci.setflags(write=False)
    return rp, ci
