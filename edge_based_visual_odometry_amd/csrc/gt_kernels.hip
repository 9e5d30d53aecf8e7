// gt_kernels.hip -- ground-truth evaluation of the stereo chain from a disparity map, on gfx950.
//
// Replaces, in the reference (the has_gt() == true branch, is_left = true):
//   Stereo_Matches::Find_Stereo_GT_Locations                   src/Stereo_Matches.cpp:133-200
//   Bilinear_Interpolation<float>                              include/utility.h:81-104
//   get_Stereo_Edge_GT_Pairs / get_right_edge_indices_close_to_GT_location / extract_Epipolar_Edge_Indices
//                                                              src/Stereo_Matches.cpp:202-268, :111-131, :91-109
//   Evaluate_Stereo_Edge_Correspondences (per-row counts)      src/Stereo_Matches.cpp:270-379
//
// gt_locate: one thread per left edge.  gt_pool / gt_census: one WAVE per left edge walks the right edges through the
// two levels of index-range bounding boxes of the candidate search (chunks of 8 edges, groups of 64 chunks): the 64 lanes
// test 64 group boxes, then the 64 chunk boxes of every marked group, then take the marked chunks eight at a time, one
// pair per lane, in ascending right index; a ballot gives the hit mask, popcounts give the counts and the ranks.  The
// boxes only pre-filter: every decision is the exact predicate of ebvo_cand.h / of the reference text.  gt_rows: eight
// lanes per row of a CSR list.  No floating-point value is ever accumulated on the device: the kernels produce integer
// (n, tp) per row, the integer stage totals are integer atomics, and the four doubles of a stage are summed on the host
// in row order (ebvo_capi.hip: gt_stage_doubles).
//
// Compiled with -ffp-contract=off like the rest.
#include "ebvo_cand.h"
#include "ebvo_geom.h"
#include "ebvo_internal.h"
#include "ebvo_math.h"

namespace
{

constexpr double RAD_TO_DEG = 0x1.ca5dc1a63c1f8p+5; // 180.0 / M_PI (include/utility.h:290)

// Bilinear_Interpolation<float> (include/utility.h:81-104) in the reference's expression order.  At an integer x or y the
// weights are 0 / 0: the result is NaN, as there.  (A NaN coordinate, which the reference would index the map with, is
// out of bounds here.)
__device__ inline double bilinear_f32_nan(const float *__restrict__ m, int rows, int cols, int stride, double x, double y)
{
    const double fx = floor(x), cx = ceil(x), fy = floor(y), cy = ceil(y);
    if (!(fx >= 0 && fy >= 0 && cx < cols && cy < rows)) // Q11 = (fx, cy), Q21 = (cx, cy), Q12 = (fx, fy), Q22 = (cx, fy)
        return __builtin_nan("");
    const int ifx = (int)fx, icx = (int)cx, ify = (int)fy, icy = (int)cy;
    const double q11 = m[(size_t)icy * stride + ifx], q21 = m[(size_t)icy * stride + icx];
    const double q12 = m[(size_t)ify * stride + ifx], q22 = m[(size_t)ify * stride + icx];
    const double f_x_y1 = ((cx - x) / (cx - fx)) * q11 + ((x - fx) / (cx - fx)) * q21;
    const double f_x_y2 = ((cx - x) / (cx - fx)) * q12 + ((x - fx) / (cx - fx)) * q22;
    return ((fy - y) / (fy - cy)) * f_x_y1 + ((y - cy) / (fy - cy)) * f_x_y2;
}

struct GtCalib
{
    double Kli[9], R21[9], T21[3];
};

// Find_Stereo_GT_Locations (:133-200).  Both rays use the LEFT calibration inverse (:179-180).
__global__ __launch_bounds__(256) void gt_locate_kernel(const ebvo_edge *__restrict__ E, int n, const float *__restrict__ disp,
                                                        int h, int w, int stride, GtCalib C, double gate_deg,
                                                        uint8_t *__restrict__ valid, double *__restrict__ gt_xy,
                                                        double *__restrict__ gl, double *__restrict__ gr)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        const double x = E[i].x, y = E[i].y, deg = E[i].theta * RAD_TO_DEG;
        bool ok = !(fabs(deg) < gate_deg || fabs(deg - 180.0) < gate_deg || fabs(deg + 180.0) < gate_deg); // :146
        double d = 0.0;
        if (ok)
        {
            d = bilinear_f32_nan(disp, h, w, stride, x, y);
            ok = !(d != d || isinf(d) || d < 0); // :154
        }
        double gx = -1.0, gy = -1.0, G[3] = {-1.0, -1.0, -1.0}, Gr[3] = {-1.0, -1.0, -1.0};
        if (ok)
        {
            gx = x - d;
            gy = y;
            const double e1[3] = {x, y, 1.0}, e2[3] = {gx, gy, 1.0};
            double g1[3], g2[3], Rg1[3];
            mv3(C.Kli, e1, g1);
            mv3(C.Kli, e2, g2);
            mv3(C.R21, g1, Rg1);
            // Utility::backproject_2D_point_to_3D_point_using_rays (src/utility.cpp:95-102), as ebvo_geom.h states it
            const double numerator = C.T21[0] - C.T21[2] * g2[0];
            const double denominator = Rg1[2] * g2[0] - Rg1[0];
            const double rho1 = numerator / denominator;
            G[0] = rho1 * g1[0];
            G[1] = rho1 * g1[1];
            G[2] = rho1 * g1[2];
            mv3(C.R21, G, Gr); // :189
            Gr[0] += C.T21[0];
            Gr[1] += C.T21[1];
            Gr[2] += C.T21[2];
        }
        valid[i] = ok ? 1 : 0;
        gt_xy[(size_t)i * 2] = gx;
        gt_xy[(size_t)i * 2 + 1] = gy;
#pragma unroll
        for (int k = 0; k < 3; ++k)
        {
            gl[(size_t)i * 3 + k] = G[k];
            gr[(size_t)i * 3 + k] = Gr[k];
        }
    }
}

// chunk and group boxes of the right edges (pre-filter only): the candidate search's construction, ebvo_cand.h
__global__ __launch_bounds__(256) void gt_boxes_kernel(const ebvo_edge *__restrict__ R, int nR, Box *__restrict__ cb,
                                                       Box *__restrict__ gb)
{
    boxes_body(R, nR, cb, gb, nullptr, 0, blockIdx.x, gridDim.x);
}

// What a box must meet for one left edge: box_may_match's arguments.
struct WalkRegion
{
    double xc, yc, ah, bh, ch, D, band;
    int mask;
};

// One wave visits, in ascending right index, every right edge of every chunk whose box meets the region: visit(act, k,
// x, y, theta) is called by all 64 lanes together (it may ballot); act = this lane holds right edge k.
template <class F>
__device__ inline void walk_right_edges(const Box *__restrict__ cb, const Box *__restrict__ gb, const ebvo_edge *__restrict__ R,
                                        int nR, const WalkRegion &g, F &&visit)
{
    const int lane = threadIdx.x & 63, sub = lane >> 3, e = lane & 7;
    const int nchunks = (nR + CHUNK - 1) / CHUNK, ngroups = (nchunks + GROUP - 1) / GROUP;
    for (int g0 = 0; g0 < ngroups; g0 += 64)
    {
        const int gi = g0 + lane;
        unsigned long long gm =
            __ballot(gi < ngroups && box_may_match(gb[gi < ngroups ? gi : 0], g.xc, g.yc, g.ah, g.bh, g.ch, g.D, g.band, g.mask));
        while (gm)
        {
            const int grp = g0 + __ffsll((long long)gm) - 1;
            gm &= gm - 1;
            const int c = grp * GROUP + lane;
            unsigned long long cm =
                __ballot(c < nchunks && box_may_match(cb[c < nchunks ? c : 0], g.xc, g.yc, g.ah, g.bh, g.ch, g.D, g.band, g.mask));
            while (cm)
            {
                // lanes 8 s .. 8 s + 7 take the s-th marked chunk
                unsigned long long m = cm;
                for (int t = 0; t < sub; ++t)
                    m &= m - 1; // 0 stays 0
                const int k = m ? (grp * GROUP + __ffsll((long long)m) - 1) * CHUNK + e : nR;
                const bool act = k < nR;
                double x = 0.0, y = 0.0, th = 0.0;
                if (act)
                {
                    x = R[k].x;
                    y = R[k].y;
                    th = R[k].theta;
                }
                visit(act, k, x, y, th);
#pragma unroll
                for (int t = 0; t < 8; ++t)
                    cm &= cm - 1;
            }
        }
    }
}

struct PoolArgs
{
    const ebvo_edge *L, *R;
    const double *lines, *gt_xy;
    const uint8_t *valid;
    const Box *cb, *gb;
    int nL, nR;
    double epi_thr, dist_tol, orient_tol;
};

// get_Stereo_Edge_GT_Pairs (:202-268): right edge k joins row i if extract_Epipolar_Edge_Indices(line, right, epi_thr)
// holds (:99-101, the candidate search's predicate and its exact-branch treatment), cv::norm(GT - loc) < dist_tol (:120)
// and |deg(theta_R) - deg(theta_L)| < orient_tol, no wrap-around (:124).  FILL = false: cnt[i]; FILL = true: the indices
// at row_ptr[i] and focused[i] = valid[i] && cnt > 0.
template <bool FILL>
__global__ __launch_bounds__(256) void gt_pool_kernel(PoolArgs A, int32_t *__restrict__ cnt, const int32_t *__restrict__ row_ptr,
                                                      int32_t *__restrict__ pool_idx, uint8_t *__restrict__ focused)
{
    const int lane = threadIdx.x & 63;
    CandParams P{};
    P.epi_thr = A.epi_thr;
    P.mask = EBVO_STAGE_EPIPOLAR;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < A.nL; i += gridDim.x * 4)
    {
        int n = 0;
        if (A.valid[i])
        {
            const LeftCtx l = left_ctx_make(A.L[i].x, A.L[i].y, A.L[i].theta, A.lines[(size_t)i * 3], A.lines[(size_t)i * 3 + 1],
                                            A.lines[(size_t)i * 3 + 2], A.epi_thr, 0.0);
            const double gx = A.gt_xy[(size_t)i * 2], gy = A.gt_xy[(size_t)i * 2 + 1];
            const double degL = l.lth * RAD_TO_DEG;
            WalkRegion g{gx, gy, l.ah, l.bh, l.ch, A.dist_tol + BOX_SLACK, A.epi_thr + BOX_SLACK,
                         EBVO_STAGE_EPIPOLAR | EBVO_STAGE_DISPARITY};
            const int64_t o = FILL ? (int64_t)row_ptr[i] : 0;
            walk_right_edges(A.cb, A.gb, A.R, A.nR, g, [&](bool act, int k, double x, double y, double th) {
                const double dx = gx - x, dy = gy - y;
                const bool ok = act && pair_passes(l, x, y, th, P) && sqrt(dx * dx + dy * dy) < A.dist_tol &&
                                fabs(th * RAD_TO_DEG - degL) < A.orient_tol;
                const unsigned long long hits = __ballot(ok);
                if (FILL && ok)
                    pool_idx[o + n + __popcll(hits & ((1ull << lane) - 1ull))] = k;
                n += __popcll(hits);
            });
        }
        if (lane == 0)
        {
            if (FILL)
                focused[i] = n > 0 ? 1 : 0;
            else
                cnt[i] = n;
        }
    }
}

struct CensusArgs
{
    const ebvo_edge *L, *R;
    const double *lines, *gt_xy;
    const uint8_t *focused;
    const Box *cb, *gb;
    int nL, nR;
    double epi_thr, max_disp, orient_thr, tp_dist;
    int mask;
    int32_t *rows[3]; // [nL][2] (n, tp) under epi, epi & disp, epi & disp & orient
};

// The three geometric stages (:1374-1408), whose lists the chain never forms: per focused row one walk of the boxes under
// the first enabled predicate, the candidate search's predicates on every visited pair, and a TP test (:305, <=).
__global__ __launch_bounds__(256) void gt_census_kernel(CensusArgs A)
{
    const int lane = threadIdx.x & 63;
    CandParams Pe{}, Pd{}, Po{};
    Pe.epi_thr = Pd.epi_thr = Po.epi_thr = A.epi_thr;
    Pe.max_disp = Pd.max_disp = Po.max_disp = A.max_disp;
    Pe.orient_thr = Pd.orient_thr = Po.orient_thr = A.orient_thr;
    Pe.mask = A.mask & EBVO_STAGE_EPIPOLAR;
    Pd.mask = A.mask & EBVO_STAGE_DISPARITY;
    Po.mask = A.mask & EBVO_STAGE_ORIENTATION;
    const double d2 = A.max_disp * A.max_disp;
    for (int i = blockIdx.x * 4 + (threadIdx.x >> 6); i < A.nL; i += gridDim.x * 4)
    {
        int n0 = 0, n1 = 0, n2 = 0, t0 = 0, t1 = 0, t2 = 0;
        if (A.focused[i])
        {
            const LeftCtx l = left_ctx_make(A.L[i].x, A.L[i].y, A.L[i].theta, A.lines[(size_t)i * 3], A.lines[(size_t)i * 3 + 1],
                                            A.lines[(size_t)i * 3 + 2], A.epi_thr, d2);
            const double gx = A.gt_xy[(size_t)i * 2], gy = A.gt_xy[(size_t)i * 2 + 1];
            WalkRegion g{l.lx, l.ly, l.ah, l.bh, l.ch, A.max_disp + BOX_SLACK, A.epi_thr + BOX_SLACK, Pe.mask};
            walk_right_edges(A.cb, A.gb, A.R, A.nR, g, [&](bool act, int, double x, double y, double th) {
                const double dx = x - gx, dy = y - gy;
                const bool tp = sqrt(dx * dx + dy * dy) <= A.tp_dist;
                const bool pe = act && pair_passes(l, x, y, th, Pe);
                const bool pd = pe && pair_passes(l, x, y, th, Pd);
                const bool po = pd && pair_passes(l, x, y, th, Po);
                n0 += __popcll(__ballot(pe));
                t0 += __popcll(__ballot(pe && tp));
                n1 += __popcll(__ballot(pd));
                t1 += __popcll(__ballot(pd && tp));
                n2 += __popcll(__ballot(po));
                t2 += __popcll(__ballot(po && tp));
            });
        }
        if (lane == 0)
        {
            A.rows[0][(size_t)i * 2] = n0;
            A.rows[0][(size_t)i * 2 + 1] = t0;
            A.rows[1][(size_t)i * 2] = n1;
            A.rows[1][(size_t)i * 2 + 1] = t1;
            A.rows[2][(size_t)i * 2] = n2;
            A.rows[2][(size_t)i * 2 + 1] = t2;
        }
    }
}

// Evaluate_Stereo_Edge_Correspondences' inner loop (:296-331) on a CSR list: eight lanes per row.  A candidate is
// cand[k], or R[col_idx[k]]; flags (optional): only candidates with flags[k] != 0 are in the list.
__global__ __launch_bounds__(256) void gt_rows_kernel(const int32_t *__restrict__ row_ptr, const ebvo_edge *__restrict__ cand,
                                                      const int32_t *__restrict__ col_idx, const ebvo_edge *__restrict__ R,
                                                      const uint8_t *__restrict__ flags, const double *__restrict__ gt_xy,
                                                      const uint8_t *__restrict__ focused, int nL, double tp_dist,
                                                      int32_t *__restrict__ out)
{
    const int lane = threadIdx.x & 63, e = lane & 7, gshift = lane & ~7;
    const int rows_per_pass = (gridDim.x * blockDim.x) >> 3;
    const int first = (blockIdx.x * blockDim.x + threadIdx.x) >> 3;
    // every lane of a wave runs the same number of passes (the ballots below need the whole wave)
    for (int base = 0; base < nL; base += rows_per_pass)
    {
        const int i = base + first;
        const bool live = i < nL && focused[i];
        const int b = live ? row_ptr[i] : 0, len = live ? row_ptr[i + 1] - b : 0;
        const double gx = live ? gt_xy[(size_t)i * 2] : 0.0, gy = live ? gt_xy[(size_t)i * 2 + 1] : 0.0;
        int n = 0, tp = 0;
        int maxlen = len;
        for (int d = 32; d > 0; d >>= 1)
            maxlen = max(maxlen, __shfl_xor(maxlen, d));
        for (int k0 = 0; k0 < maxlen; k0 += 8)
        {
            const int k = k0 + e;
            bool in = k < len;
            if (in && flags)
                in = flags[b + k] != 0;
            bool hit = false;
            if (in)
            {
                const ebvo_edge &c = cand ? cand[b + k] : R[col_idx[b + k]];
                const double dx = c.x - gx, dy = c.y - gy;
                hit = sqrt(dx * dx + dy * dy) <= tp_dist; // :305
            }
            n += __popcll((__ballot(in) >> gshift) & 0xffull);
            tp += __popcll((__ballot(hit) >> gshift) & 0xffull);
        }
        if (e == 0 && i < nL)
        {
            out[(size_t)i * 2] = n;
            out[(size_t)i * 2 + 1] = tp;
        }
    }
}

// integer totals of one stage: focused rows, non-empty rows, rows with a TP, sum of tp, sum of n (tot zeroed beforehand)
__global__ __launch_bounds__(256) void gt_totals_kernel(const int32_t *__restrict__ rows, const uint8_t *__restrict__ focused, int nL,
                                                        unsigned long long *__restrict__ tot)
{
    unsigned long long v[5] = {0, 0, 0, 0, 0};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nL; i += gridDim.x * blockDim.x)
        if (focused[i])
        {
            const int n = rows[(size_t)i * 2], tp = rows[(size_t)i * 2 + 1];
            v[0] += 1;
            v[1] += n > 0;
            v[2] += tp > 0;
            v[3] += (unsigned long long)tp;
            v[4] += (unsigned long long)n;
        }
#pragma unroll
    for (int k = 0; k < 5; ++k)
    {
        for (int d = 32; d > 0; d >>= 1)
            v[k] += __shfl_xor(v[k], d);
        if ((threadIdx.x & 63) == 0 && v[k])
            atomicAdd(&tot[k], v[k]);
    }
}

int gt_grid(const ebvo_ctx *ctx, int64_t items, int per_block)
{
    int64_t g = (items + per_block - 1) / per_block;
    const int64_t most = ctx->gt_blocks > 0 ? ctx->gt_blocks : 8192;
    g = g < 1 ? 1 : g;
    return (int)(g < most ? g : most);
}

} // namespace

int gt_locate_enqueue(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_E, int n, const float *d_disp, int h, int w, int stride,
                      const ebvo_stereo_calib *calib, double gate_deg, uint8_t *d_valid, double *d_gt_xy, double *d_gl, double *d_gr)
{
    if (n <= 0)
        return EBVO_OK;
    GtCalib C;
    inverse3_host(calib->K_left, C.Kli);
    for (int k = 0; k < 9; ++k)
        C.R21[k] = calib->R21[k];
    for (int k = 0; k < 3; ++k)
        C.T21[k] = calib->T21[k];
    ProfScope ps(ctx, s, K_GT_MISC);
    hipLaunchKernelGGL(gt_locate_kernel, dim3(gt_grid(ctx, n, 256)), dim3(256), 0, s.stream, d_E, n, d_disp, h, w, stride, C, gate_deg,
                       d_valid, d_gt_xy, d_gl, d_gr);
    EBVO_HIP(ctx, hipGetLastError());
    return EBVO_OK;
}

size_t gt_boxes_bytes(int nR)
{
    const size_t nchunks = ((size_t)nR + CHUNK - 1) / CHUNK, ngroups = (nchunks + GROUP - 1) / GROUP;
    return sizeof(Box) * (nchunks + ngroups + 2);
}

int gt_boxes_enqueue(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_R, int nR, void *d_boxes)
{
    if (nR <= 0)
        return EBVO_OK;
    const size_t nchunks = ((size_t)nR + CHUNK - 1) / CHUNK, ngroups = (nchunks + GROUP - 1) / GROUP;
    Box *cb = (Box *)d_boxes, *gb = cb + nchunks + 1;
    ProfScope ps(ctx, s, K_GT_MISC);
    hipLaunchKernelGGL(gt_boxes_kernel, dim3(gt_grid(ctx, (int64_t)ngroups, 4)), dim3(256), 0, s.stream, d_R, nR, cb, gb);
    EBVO_HIP(ctx, hipGetLastError());
    return EBVO_OK;
}

int gt_pool_enqueue(ebvo_ctx *ctx, Slot &s, bool fill, const ebvo_edge *d_L, int nL, const ebvo_edge *d_R, int nR,
                    const double *d_lines, const double *d_gt_xy, const uint8_t *d_valid, const void *d_boxes,
                    const ebvo_gt_params *p, int32_t *d_cnt, const int32_t *d_row_ptr, int32_t *d_pool_idx, uint8_t *d_focused)
{
    if (nL <= 0)
        return EBVO_OK;
    const size_t nchunks = ((size_t)nR + CHUNK - 1) / CHUNK;
    PoolArgs A;
    A.L = d_L; A.R = d_R; A.lines = d_lines; A.gt_xy = d_gt_xy; A.valid = d_valid;
    A.cb = (const Box *)d_boxes; A.gb = A.cb + nchunks + 1;
    A.nL = nL; A.nR = nR;
    A.epi_thr = p->pool_epi_thr; A.dist_tol = p->pool_dist; A.orient_tol = p->pool_orient_deg;
    const dim3 grid(gt_grid(ctx, nL, 4));
    ProfScope ps(ctx, s, K_GT_POOL);
    if (fill)
        hipLaunchKernelGGL(gt_pool_kernel<true>, grid, dim3(256), 0, s.stream, A, d_cnt, d_row_ptr, d_pool_idx, d_focused);
    else
        hipLaunchKernelGGL(gt_pool_kernel<false>, grid, dim3(256), 0, s.stream, A, d_cnt, d_row_ptr, d_pool_idx, d_focused);
    EBVO_HIP(ctx, hipGetLastError());
    return EBVO_OK;
}

int gt_census_enqueue(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_L, int nL, const ebvo_edge *d_R, int nR, const double *d_lines,
                      const double *d_gt_xy, const uint8_t *d_focused, const void *d_boxes, const ebvo_stereo_params *sp,
                      double tp_dist, int32_t *d_rows0, int32_t *d_rows1, int32_t *d_rows2)
{
    if (nL <= 0)
        return EBVO_OK;
    const size_t nchunks = ((size_t)nR + CHUNK - 1) / CHUNK;
    CensusArgs A;
    A.L = d_L; A.R = d_R; A.lines = d_lines; A.gt_xy = d_gt_xy; A.focused = d_focused;
    A.cb = (const Box *)d_boxes; A.gb = A.cb + nchunks + 1;
    A.nL = nL; A.nR = nR;
    A.epi_thr = sp->epi_thr; A.max_disp = sp->max_disp; A.orient_thr = sp->orient_thr_deg; A.tp_dist = tp_dist;
    A.mask = sp->stage_mask;
    A.rows[0] = d_rows0; A.rows[1] = d_rows1; A.rows[2] = d_rows2;
    ProfScope ps(ctx, s, K_GT_CENSUS);
    hipLaunchKernelGGL(gt_census_kernel, dim3(gt_grid(ctx, nL, 4)), dim3(256), 0, s.stream, A);
    EBVO_HIP(ctx, hipGetLastError());
    return EBVO_OK;
}

int gt_rows_enqueue(ebvo_ctx *ctx, Slot &s, const int32_t *d_row_ptr, const ebvo_edge *d_cand, const int32_t *d_col_idx,
                    const ebvo_edge *d_R, const uint8_t *d_flags, const double *d_gt_xy, const uint8_t *d_focused, int nL,
                    double tp_dist, int32_t *d_rows, unsigned long long *d_tot)
{
    if (nL <= 0)
        return EBVO_OK;
    {
        ProfScope ps(ctx, s, K_GT_ROWS);
        hipLaunchKernelGGL(gt_rows_kernel, dim3(chain_grid_cap(s, gt_grid(ctx, nL, 32))), dim3(256), 0, s.stream, d_row_ptr, d_cand, d_col_idx, d_R,
                           d_flags, d_gt_xy, d_focused, nL, tp_dist, d_rows);
        EBVO_HIP(ctx, hipGetLastError());
    }
    return gt_totals_enqueue(ctx, s, d_rows, d_focused, nL, d_tot);
}

int gt_totals_enqueue(ebvo_ctx *ctx, Slot &s, const int32_t *d_rows, const uint8_t *d_focused, int nL, unsigned long long *d_tot)
{
    EBVO_HIP(ctx, hipMemsetAsync(d_tot, 0, sizeof(unsigned long long) * 5, s.stream));
    if (nL <= 0)
        return EBVO_OK;
    ProfScope ps(ctx, s, K_GT_MISC);
    // sixteen rows per thread: the five integer atomics of a wave land on the same five words, so few waves
    hipLaunchKernelGGL(gt_totals_kernel, dim3(chain_grid_cap(s, gt_grid(ctx, nL, 256 * 16))), dim3(256), 0, s.stream, d_rows, d_focused, nL, d_tot);
    EBVO_HIP(ctx, hipGetLastError());
    return EBVO_OK;
}
