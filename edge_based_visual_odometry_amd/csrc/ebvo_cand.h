// ebvo_cand.h -- the pair predicates of the candidate search and the index-range boxes that pre-filter them, shared by
// match_kernels.hip (candidates_kernel) and gt_kernels.hip (veridical pool, per-stage census): one statement of the
// reference's tests (src/Stereo_Matches.cpp:99-101, :545-546, :887-901), so both walks decide every pair alike.
#ifndef EBVO_CAND_H
#define EBVO_CAND_H

#include "ebvo_internal.h"

#ifdef __HIPCC__
namespace
{

constexpr int CHUNK = 8;         // edges per chunk box = lanes per left edge in the candidate walk
constexpr int GROUP = 64;        // chunks per group box (512 edges)
constexpr double BOX_SLACK = 1e-6;

struct Box
{
    double x0, x1, y0, y1;
};

// A size that is either known on the host (dev == nullptr) or lives in device memory: the device-resident
// pipeline never reads a count back before the last kernel of a pair, so every kernel takes its sizes this way
// and runs grid-stride over whatever the count turns out to be.
struct DevN
{
    int host;
    const int32_t *dev;
};
__device__ inline int devn(const DevN &d) { return d.dev ? *d.dev : d.host; }

struct CandParams
{
    double epi_thr, max_disp, orient_thr;
    int mask;
    DevN nL, nR;
    int64_t cap;        // capacity of col_idx (FILL)
    int32_t *stage;     // [nL][STAGE] first STAGE candidates of every left edge, written by the counting pass
    int32_t *tile_flag; // [tiles] 1: some row of the tile has more than STAGE candidates -> the fill pass redoes the tile
    int32_t *tile_tot;  // [tiles] candidates of the tile's rows (int32, wraps like the row offsets), written by the counting pass
};

// Can any point of the box satisfy the enabled epipolar / disparity predicates?  Conservative.
__device__ inline bool box_may_match(const Box &bx, double xl, double yl, double ah, double bh, double ch,
                                     double D, double band, int mask)
{
    double x0 = bx.x0, x1 = bx.x1, y0 = bx.y0, y1 = bx.y1;
    if (mask & EBVO_STAGE_DISPARITY)
    {
        x0 = fmax(x0, xl - D);
        x1 = fmin(x1, xl + D);
        y0 = fmax(y0, yl - D);
        y1 = fmin(y1, yl + D);
        if (x0 > x1 || y0 > y1)
            return false;
    }
    if (mask & EBVO_STAGE_EPIPOLAR)
    {
        const double gx0 = ah * x0, gx1 = ah * x1, gy0 = bh * y0, gy1 = bh * y1;
        const double gmin = fmin(gx0, gx1) + fmin(gy0, gy1) + ch;
        const double gmax = fmax(gx0, gx1) + fmax(gy0, gy1) + ch;
        if (gmin > band || gmax < -band)
            return false;
    }
    return true;
}

// Per-left-edge constants of the predicates.
struct LeftCtx
{
    double lx, ly, lth;
    double a, b, c, nrm;    // epipolar line and sqrt(a*a + b*b) (src/Stereo_Matches.cpp:99)
    double ah, bh, ch;      // normalised line, for the conservative box tests only
    double t_lo, t_hi;      // epi_thr * nrm * (1 -+ 2^-50)
    double s_lo, s_hi;      // max_disp^2 * (1 -+ 2^-50)
};

// The reference's predicates, bit-exact.
//   epipolar (:99-101):  fl(|a x + b y + c| / nrm) < thr.   With t = fl(thr*nrm): |num| < t(1-2^-50) implies the
//     rounded quotient is < thr, |num| > t(1+2^-50) implies it is >= thr (division is monotone and correctly rounded,
//     all roundings involved are <= 2^-53 relative); only inside that sliver is the division evaluated.
//   disparity (:545-546): fl(sqrt(fl(dx*dx + dy*dy))) <= D, same argument on s = fl(dx*dx + dy*dy) against D^2.
//   orientation (:887-901): as written.
// Straight-line form: the three quantities are always evaluated and compared against both margins; only a lane inside
// a 2^-50 sliver (practically never) takes the branch with the division / square root.  One lane = one pair in the
// candidate walk, so an early exit saves nothing unless all 64 lanes take it, while every nested exit costs
// exec-mask bookkeeping.
__device__ inline bool pair_passes(const LeftCtx &l, double rx, double ry, double rth, const CandParams &P)
{
    bool e_fast = true, e_maybe = true, d_fast = true, d_maybe = true, o_ok = true;
    double num = 0.0, s = 0.0;
    if (P.mask & EBVO_STAGE_EPIPOLAR)
    {
        num = fabs(l.a * rx + l.b * ry + l.c);
        e_fast = num < l.t_lo;
        e_maybe = num <= l.t_hi; // false for NaN
    }
    if (P.mask & EBVO_STAGE_DISPARITY)
    {
        const double dx = l.lx - rx, dy = l.ly - ry;
        s = dx * dx + dy * dy;
        d_fast = s < l.s_lo;
        d_maybe = s <= l.s_hi;
    }
    if (P.mask & EBVO_STAGE_ORIENTATION)
    {
        double od = fabs((l.lth - rth) * 0x1.ca5dc1a63c1f8p+5 /* 180.0 / M_PI */);
        if (od > 180.0)
            od = 360.0 - od;
        o_ok = od < P.orient_thr || fabs(od - 180.0) < P.orient_thr;
    }
    bool ok = o_ok && e_maybe && d_maybe;
    if (ok && !(e_fast && d_fast))
    {
        asm volatile("" : "+v"(num), "+v"(s)); // keeps the division and the square root inside the rare branch
        if (!e_fast)
            ok = num / l.nrm < P.epi_thr;
        if (ok && !d_fast)
            ok = sqrt(s) <= P.max_disp;
    }
    return ok;
}

__device__ inline double wave_min(double v)
{
    for (int d = 32; d > 0; d >>= 1)
        v = fmin(v, __shfl_xor(v, d));
    return v;
}
__device__ inline double wave_max(double v)
{
    for (int d = 32; d > 0; d >>= 1)
        v = fmax(v, __shfl_xor(v, d));
    return v;
}

// Bounding boxes of the index ranges: one thread per chunk (CHUNK edges), one wave per group (64 chunks), so the group
// box is a wave reduction of the chunk boxes it has just produced.
__device__ inline void boxes_body(const ebvo_edge *__restrict__ R, int nR, Box *__restrict__ cb, Box *__restrict__ gb,
                                  int32_t *__restrict__ tile_flag, int ntiles, int vb, int vg)
{
    static_assert(GROUP == 64, "one wave per group");
    // the tile flags of the counting pass that follows (round 4: zeroed here instead of by a launch of their own)
    for (int t = vb * blockDim.x + threadIdx.x; t < ntiles; t += vg * blockDim.x)
        tile_flag[t] = 0;
    const int nchunks = (nR + CHUNK - 1) / CHUNK, ngroups = (nchunks + GROUP - 1) / GROUP;
    const int lane = threadIdx.x & 63;
    const double inf = __builtin_inf();
    for (int g = vb * 4 + (threadIdx.x >> 6); g < ngroups; g += vg * 4)
    {
        const int c = g * GROUP + lane;
        Box b;
        b.x0 = inf; b.x1 = -inf; b.y0 = inf; b.y1 = -inf;
        if (c < nchunks)
        {
            const int k0 = c * CHUNK, k1 = min(nR, k0 + CHUNK);
            b.x0 = b.x1 = R[k0].x;
            b.y0 = b.y1 = R[k0].y;
            for (int k = k0 + 1; k < k1; ++k)
            {
                const double x = R[k].x, y = R[k].y;
                b.x0 = fmin(b.x0, x);
                b.x1 = fmax(b.x1, x);
                b.y0 = fmin(b.y0, y);
                b.y1 = fmax(b.y1, y);
            }
            cb[c] = b;
        }
        Box u;
        u.x0 = wave_min(b.x0); u.x1 = wave_max(b.x1); u.y0 = wave_min(b.y0); u.y1 = wave_max(b.y1);
        if (lane == 0)
            gb[g] = u;
    }
}

// the constants of one left edge: its location, orientation and epipolar line (a, b, c); d2 = max_disp * max_disp
__device__ inline LeftCtx left_ctx_make(double lx, double ly, double lth, double a, double b, double c, double epi_thr, double d2)
{
    LeftCtx l;
    l.lx = lx; l.ly = ly; l.lth = lth;
    l.a = a; l.b = b; l.c = c;
    l.nrm = sqrt((l.a * l.a) + (l.b * l.b));
    l.ah = l.a / l.nrm; l.bh = l.b / l.nrm; l.ch = l.c / l.nrm;
    const double t = epi_thr * l.nrm;
    l.t_lo = t * (1.0 - 0x1p-50); l.t_hi = t * (1.0 + 0x1p-50);
    l.s_lo = d2 * (1.0 - 0x1p-50); l.s_hi = d2 * (1.0 + 0x1p-50);
    return l;
}

} // namespace
#endif

#endif /* EBVO_CAND_H */
