// Coverage of the current frame by the keyframe (ebvo_keyframe_cover_edges / ebvo_temporal_keyframe_cover).  The arithmetic
// contract is written once in include/ebvo_hip.h; tests/oracle_cover.py restates it on the CPU and the device matches it bit
// for bit.
//   (the alignment's own grids and ONE association under the pose come first, unchanged: align_associate_once, camera 0)
//   cover_mate_kernel     ONE lane per keyframe mate: Gamma (stereo_gamma_tangent), the dead test, Gamma / lambda, the
//                         projection, the in-frame test, the displacement from the keyframe position and its bin, then -- with
//                         the edge index the association left -- the residual, the inlier test and the byte of the explained
//                         edge.  The 64 bins are counted in LDS per workgroup and added with integer atomics
//   cover_edge_kernel     one lane per current edge: its coarse cell by grid_cell's rule, the two cell counts (integer
//                         atomics) and n_explained
//   cover_finish_kernel   one workgroup: the cells that hold enough edges and, of them, the covered ones; the median bin; the
//                         record
// The counters are wave sums of integers and one atomic per wave and counter.  `explained` holds the value 1 wherever some mate
// wrote it: the same byte from every writer, so no order enters.  The pose, the calibration and the parameters are kernel
// arguments.  No host read between the launches, no spin-wait, no grid-wide barrier (the stream orders them), every loop
// bounded by its arguments.  fp64 throughout, -ffp-contract=off (no FMA), IEEE division and sqrt.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "ebvo_internal.h"
#include "ebvo_math.h"
#include "ebvo_geom.h"
#include "ebvo_gn6.h"

namespace
{
struct CoverArgs
{
    double Kl[9], Rt[12];
    double margin, x_max, y_max, inlier, bin;
    int32_t n_kf, n0, cover_cell, cw, ch, min_edges, min_explained, pad;
};

// counters of the call, zeroed before the first launch
enum
{
    CV_DEAD,
    CV_IN_FRAME,
    CV_ASSOC,
    CV_INLIERS,
    CV_EXPLAINED,
    CV_COUNTS = 8
};

__global__ __launch_bounds__(256) void cover_mate_kernel(FinalCalib C, CoverArgs A, const ebvo_edge *__restrict__ kfL,
                                                         const ebvo_edge *__restrict__ kfR, const double *__restrict__ lam,
                                                         const ebvo_edge *__restrict__ E0, const int32_t *__restrict__ idx,
                                                         uint8_t *__restrict__ flags, int32_t *__restrict__ assoc,
                                                         double *__restrict__ disp, uint8_t *__restrict__ explained,
                                                         int32_t *__restrict__ hist, int32_t *__restrict__ counts)
{
    __shared__ int32_t bins[EBVO_COVER_BINS];
    if (threadIdx.x < EBVO_COVER_BINS)
        bins[threadIdx.x] = 0;
    __syncthreads();
    int n_dead = 0, n_in = 0, n_assoc = 0, n_inl = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.n_kf; i += gridDim.x * blockDim.x)
    {
        const ebvo_edge k = kfL[i];
        double G[3], T1[3], g1[3], g2[3];
        stereo_gamma_tangent(C, k, kfR[i], G, T1, g1, g2);
        unsigned fl = 0;
        int a = -1;
        double d = NAN;
        if (!live_mate(G))
        {
            fl = EBVO_COVER_DEAD;
            ++n_dead;
        }
        else
        {
            double Gs[3] = {G[0], G[1], G[2]};
            if (lam)
            {
                const double l = lam[i];
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    Gs[c] = G[c] / l;
            }
            double RG[3], X[3], q[3];
            pose_point(A.Rt, A.Rt + 9, Gs, RG, X);
            project3(A.Kl, X, q);
            if (live_projection(q[0], q[1], X[2], A.margin, A.x_max, A.y_max))
            {
                fl = EBVO_COVER_IN_FRAME;
                ++n_in;
                const double dx = q[0] - k.x, dy = q[1] - k.y;
                d = sqrt(dx * dx + dy * dy);
                const double b = d / A.bin;
                atomicAdd(&bins[b >= 63.0 ? 63 : (int)b], 1);
                const int j = idx[i];
                if (j >= 0 && j < A.n0)
                {
                    a = j;
                    fl |= EBVO_COVER_ASSOCIATED;
                    ++n_assoc;
                    explained[j] = 1;
                    const ebvo_edge e = E0[j];
                    double sn, cs;
                    ebvo_sincos(e.theta, &sn, &cs);
                    const double r = sn * (q[0] - e.x) + (-cs) * (q[1] - e.y);
                    if (fabs(r) < A.inlier)
                    {
                        fl |= EBVO_COVER_INLIER;
                        ++n_inl;
                    }
                }
            }
        }
        flags[i] = (uint8_t)fl;
        assoc[i] = a;
        disp[i] = d;
    }
    const int lane = threadIdx.x & 63;
    wave_count(n_dead, lane, &counts[CV_DEAD]);
    wave_count(n_in, lane, &counts[CV_IN_FRAME]);
    wave_count(n_assoc, lane, &counts[CV_ASSOC]);
    wave_count(n_inl, lane, &counts[CV_INLIERS]);
    __syncthreads();
    if (threadIdx.x < EBVO_COVER_BINS && bins[threadIdx.x])
        atomicAdd(&hist[threadIdx.x], bins[threadIdx.x]);
}

__global__ __launch_bounds__(256) void cover_edge_kernel(CoverArgs A, const ebvo_edge *__restrict__ E0, const uint8_t *__restrict__ explained,
                                                         int32_t *__restrict__ cell_edges, int32_t *__restrict__ cell_explained,
                                                         int32_t *__restrict__ counts)
{
    int n_exp = 0;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < A.n0; j += gridDim.x * blockDim.x)
    {
        const bool ex = explained[j] != 0;
        n_exp += ex ? 1 : 0;
        const int cx = grid_cell(E0[j].x, A.cover_cell, A.cw), cy = grid_cell(E0[j].y, A.cover_cell, A.ch);
        if (cx >= 0 && cy >= 0)
        {
            const int c = cy * A.cw + cx;
            atomicAdd(&cell_edges[c], 1);
            if (ex)
                atomicAdd(&cell_explained[c], 1);
        }
    }
    wave_count(n_exp, threadIdx.x & 63, &counts[CV_EXPLAINED]);
}

__global__ __launch_bounds__(256) void cover_finish_kernel(CoverArgs A, const int32_t *__restrict__ cell_edges,
                                                           const int32_t *__restrict__ cell_explained, const int32_t *__restrict__ hist,
                                                           const int32_t *__restrict__ counts, ebvo_keyframe_cover *__restrict__ rec)
{
    __shared__ int32_t cells[2];
    if (threadIdx.x < 2)
        cells[threadIdx.x] = 0;
    __syncthreads();
    const int n_cells = A.cw * A.ch;
    int cur = 0, cov = 0;
    for (int c = threadIdx.x; c < n_cells; c += blockDim.x)
        if (cell_edges[c] >= A.min_edges)
        {
            ++cur;
            if (cell_explained[c] >= A.min_explained)
                ++cov;
        }
    const int lane = threadIdx.x & 63;
    wave_count(cur, lane, &cells[0]);
    wave_count(cov, lane, &cells[1]);
    __syncthreads();
    if (threadIdx.x != 0)
        return;
    rec->n_kf = A.n_kf;
    rec->n_dead = counts[CV_DEAD];
    rec->n_in_frame = counts[CV_IN_FRAME];
    rec->n_assoc = counts[CV_ASSOC];
    rec->n_inliers = counts[CV_INLIERS];
    rec->n_edges = A.n0;
    rec->n_explained = counts[CV_EXPLAINED];
    rec->cw = A.cw;
    rec->ch = A.ch;
    rec->n_cells_cur = cells[0];
    rec->n_cells_covered = cells[1];
    const int64_t n_in = counts[CV_IN_FRAME];
    int median = -1;
    int64_t run = 0;
    for (int b = 0; b < EBVO_COVER_BINS; ++b)
    {
        const int32_t v = hist[b];
        rec->hist[b] = v;
        run += v;
        if (median < 0 && n_in > 0 && 2 * run >= n_in)
            median = b;
    }
    rec->disp_median_bin = median;
}
} // namespace

int cover_run(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, int n_kf, const double *d_lambda, const ebvo_edge *d_E0,
              int n0, int img_w, int img_h, const ebvo_stereo_calib *cal, const ebvo_cover_params *cp, const double *R, const double *t,
              ebvo_keyframe_cover *out, uint8_t *flags, int32_t *assoc, double *disp, uint8_t *explained, int32_t *cell_edges,
              int32_t *cell_explained)
{
    const int cc = cp->cover_cell;
    const int cw = (int)(((int64_t)img_w + cc - 1) / cc), ch = (int)(((int64_t)img_h + cc - 1) / cc);
    const size_t nk = (size_t)n_kf, ne = (size_t)n0, nc = (size_t)cw * (size_t)ch;
    // the record; what is zeroed (the counters, the bins, both cell planes, the explained bytes); the per-mate outputs
    const size_t o_rec = 0, o_cnt = round_up64(sizeof(ebvo_keyframe_cover)), o_hist = o_cnt + round_up64(sizeof(int32_t) * CV_COUNTS),
                 o_ce = o_hist + round_up64(sizeof(int32_t) * EBVO_COVER_BINS), o_cx = o_ce + round_up64(4 * nc), o_exp = o_cx + round_up64(4 * nc),
                 o_fl = o_exp + round_up64(ne), o_as = o_fl + round_up64(nk), o_d = o_as + round_up64(4 * nk), total = o_d + round_up64(8 * nk);
    if (int rc = ebvo_grow(ctx, s, s.cover_ws, total))
        return rc;
    char *base = (char *)s.cover_ws.p;
    ebvo_keyframe_cover *d_rec = (ebvo_keyframe_cover *)(base + o_rec);
    int32_t *d_cnt = (int32_t *)(base + o_cnt), *d_hist = (int32_t *)(base + o_hist), *d_ce = (int32_t *)(base + o_ce),
            *d_cx = (int32_t *)(base + o_cx), *d_as = (int32_t *)(base + o_as);
    uint8_t *d_exp = (uint8_t *)(base + o_exp), *d_fl = (uint8_t *)(base + o_fl);
    double *d_d = (double *)(base + o_d);
    // the alignment's association, camera 0, under its own defaults for everything the association does not read
    ebvo_align_params ap;
    ebvo_align_default_params(&ap);
    ap.radius = cp->radius;
    ap.cell_size = cp->cell_size;
    ap.orient_thr_deg = cp->orient_thr_deg;
    ap.img_margin = cp->img_margin;
    ap.cameras = 1;
    const int32_t *d_idx0 = nullptr, *d_idx1 = nullptr;
    if (int rc = align_associate_once(ctx, s, d_kfL, d_kfR, n_kf, d_E0, n0, nullptr, 0, img_w, img_h, cal, &ap, R, t, d_lambda, &d_idx0, &d_idx1))
        return rc;
    const FinalCalib C = final_calib_host(cal->K_left, cal->K_right, cal->R21, cal->T21);
    CoverArgs A;
    memcpy(A.Kl, cal->K_left, sizeof A.Kl);
    memcpy(A.Rt, R, sizeof(double) * 9);
    memcpy(A.Rt + 9, t, sizeof(double) * 3);
    A.margin = cp->img_margin;
    A.x_max = (double)img_w - cp->img_margin;
    A.y_max = (double)img_h - cp->img_margin;
    A.inlier = cp->inlier_px;
    A.bin = cp->bin_px;
    A.n_kf = n_kf;
    A.n0 = n0;
    A.cover_cell = cc;
    A.cw = cw;
    A.ch = ch;
    A.min_edges = cp->min_cell_edges;
    A.min_explained = cp->min_cell_explained;
    A.pad = 0;
    hipStream_t st = s.stream;
    {
        ProfScope ps(ctx, s, K_MISC);
        EBVO_HIP(ctx, hipMemsetAsync(d_cnt, 0, o_fl - o_cnt, st));
        const int64_t mb = ((int64_t)n_kf + 255) / 256, eb = ((int64_t)n0 + 255) / 256;
        hipLaunchKernelGGL(cover_mate_kernel, dim3(chain_grid_cap(s, (unsigned)(mb > 2048 ? 2048 : mb))), dim3(256), 0, st, C, A, d_kfL, d_kfR,
                           d_lambda, d_E0, d_idx0, d_fl, d_as, d_d, d_exp, d_hist, d_cnt);
        hipLaunchKernelGGL(cover_edge_kernel, dim3(chain_grid_cap(s, (unsigned)(eb > 2048 ? 2048 : eb))), dim3(256), 0, st, A, d_E0, d_exp, d_ce,
                           d_cx, d_cnt);
        hipLaunchKernelGGL(cover_finish_kernel, dim3(1), dim3(256), 0, st, A, d_ce, d_cx, d_hist, d_cnt, d_rec);
    }
    EBVO_HIP(ctx, hipGetLastError());
    EBVO_HIP(ctx, hipMemcpyAsync(out, d_rec, sizeof *out, hipMemcpyDeviceToHost, st));
    if (flags)
        EBVO_HIP(ctx, hipMemcpyAsync(flags, d_fl, nk, hipMemcpyDeviceToHost, st));
    if (assoc)
        EBVO_HIP(ctx, hipMemcpyAsync(assoc, d_as, 4 * nk, hipMemcpyDeviceToHost, st));
    if (disp)
        EBVO_HIP(ctx, hipMemcpyAsync(disp, d_d, 8 * nk, hipMemcpyDeviceToHost, st));
    if (explained)
        EBVO_HIP(ctx, hipMemcpyAsync(explained, d_exp, ne, hipMemcpyDeviceToHost, st));
    if (cell_edges)
        EBVO_HIP(ctx, hipMemcpyAsync(cell_edges, d_ce, 4 * nc, hipMemcpyDeviceToHost, st));
    if (cell_explained)
        EBVO_HIP(ctx, hipMemcpyAsync(cell_explained, d_cx, 4 * nc, hipMemcpyDeviceToHost, st));
    return EBVO_OK;
}
