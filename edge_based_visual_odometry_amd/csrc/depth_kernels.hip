// Inverse-depth filter of the keyframe mates (ebvo_depth_refine_edges / ebvo_temporal_refine_depth) and the scaling of the
// alignment's prepared planes by it.  The arithmetic contract is written once in include/ebvo_hip.h; tests/oracle_depth.py
// restates it on the CPU and the device matches it bit for bit.
//   depth_scale_kernel    one thread per mate: Gamma of a live mate over its lambda, in place on the planes
//                         align_prepare_kernel left (run only when refined depths are in use)
//   depth_update_kernel   one thread per mate, everything in registers: the prior or the incoming state, both cameras' terms
//                         at the incoming lambda, liveness and gate, `iterations` Gauss-Newton steps in one unknown, accept or
//                         restore.  A workgroup walks whole tiles of 1024 mates, so that the two squared residuals of its mates
//                         go through ebvo_gn6.h's trees (64-lane halving tree, 16 group sums through LDS) into the tile's
//                         two sums; the counts are wave sums of integers and one atomic per wave and counter
//   depth_finish_kernel   one thread: the tiles in ascending order from +0.0, the two rms values, the record
// The pose, the calibration and the parameters are kernel arguments.  No host read between the launches, no spin-wait, no
// grid-wide barrier (the stream orders the three), every loop bounded by its arguments.
// fp64 throughout, -ffp-contract=off (no FMA), IEEE division and sqrt.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "ebvo_internal.h"
#include "ebvo_math.h"
#include "ebvo_geom.h"
#include "ebvo_gn6.h"

namespace
{
constexpr int DP_TILE = 1024; // mates per tile = virtual lanes of a workgroup (the alignment's)
constexpr int DP_GROUPS = DP_TILE / 64;
constexpr int DP_COUNTS = 7; // dead, updated, restored, terms[2], gated[2]: the integers of DepthRecord in order

struct DepthArgs
{
    double Kl[9], Kr[9], R21[9], T21[3], Rt[12];
    double margin, x_max, y_max, sigma_disp, iv, huber, gate, lam_min, lam_max, info_max;
    int32_t n_kf, cameras, iterations, tiles, n_e[2];
};

__global__ __launch_bounds__(256) void depth_scale_kernel(double *__restrict__ GT, int n, const double *__restrict__ lam)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        const double G[3] = {GT[i], GT[(size_t)n + i], GT[2 * (size_t)n + i]};
        if (!live_mate(G))
            continue;
        const double l = lam[i];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            GT[(size_t)k * n + i] = G[k] / l;
    }
}

// the associated edge of one camera: its location and normal
struct DepthEdge
{
    double ex, ey, n0, n1;
    bool has;
};

__device__ static inline DepthEdge depth_edge(const ebvo_edge *__restrict__ E, int n_e, const int32_t *__restrict__ idx, int i)
{
    DepthEdge d;
    d.ex = d.ey = d.n0 = d.n1 = 0.0;
    const int a = idx ? idx[i] : -1;
    d.has = a >= 0 && a < n_e;
    if (d.has)
    {
        const ebvo_edge ed = E[a];
        double sn, cs;
        ebvo_sincos(ed.theta, &sn, &cs);
        d.ex = ed.x;
        d.ey = ed.y;
        d.n0 = sn;
        d.n1 = -cs;
    }
    return d;
}

// one camera's residual r and its derivative j in lambda; pi and Y_z for the liveness test
__device__ static inline void depth_camera(const double *K, const double *Rs, const double *Y, const double *RG, double lam, const DepthEdge &e,
                                           double &r, double &j, double &pix, double &piy)
{
    double jx[3], jy[3];
    const double pz = camera_pixel(K, Y, pix, piy);
    r = e.n0 * (pix - e.ex) + e.n1 * (piy - e.ey);
    camera_rows(K, Rs, pz, pix, piy, jx, jy);
    double m[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        m[k] = e.n0 * jx[k] + e.n1 * jy[k];
    j = -(dot3(m, RG) / lam);
}

// both cameras at lambda; a camera without an edge is not evaluated
__device__ static inline void depth_eval(const DepthArgs &A, const double *G, double lam, const DepthEdge &e0, const DepthEdge &e1, double *r,
                                         double *j, double *pix, double *piy, double *yz)
{
    const double Gs[3] = {G[0] / lam, G[1] / lam, G[2] / lam};
    double RG[3], X[3];
    pose_point(A.Rt, A.Rt + 9, Gs, RG, X);
    r[0] = r[1] = j[0] = j[1] = pix[0] = pix[1] = piy[0] = piy[1] = yz[0] = yz[1] = 0.0;
    if (e0.has)
    {
        depth_camera(A.Kl, nullptr, X, RG, lam, e0, r[0], j[0], pix[0], piy[0]);
        yz[0] = X[2];
    }
    if (e1.has)
    {
        double Y[3];
        stereo_point(A.R21, A.T21, X, Y);
        depth_camera(A.Kr, A.R21, Y, RG, lam, e1, r[1], j[1], pix[1], piy[1]);
        yz[1] = Y[2];
    }
}

// Workgroup b walks tiles b, b + gridDim.x, ...  A block of 256 or 512 threads owns lanes v, v + blockDim, ...: a wave always
// reduces 64 consecutive lanes.  The in-state may be the out-state: a thread reads its mate's before it writes it.
__global__ __launch_bounds__(DP_TILE) void depth_update_kernel(DepthArgs A, const double *__restrict__ GT, const ebvo_edge *__restrict__ E0,
                                                               const ebvo_edge *__restrict__ E1, const int32_t *__restrict__ idx0,
                                                               const int32_t *__restrict__ idx1, const double *lam_in, const double *info_in,
                                                               const int32_t *nobs_in, double *lam_out, double *info_out, int32_t *nobs_out,
                                                               uint8_t *__restrict__ flags, double *__restrict__ tile_sums,
                                                               int32_t *__restrict__ counts)
{
    __shared__ double part[2][DP_GROUPS];
    const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63;
    const size_t n = (size_t)A.n_kf;
    int cnt[DP_COUNTS];
#pragma unroll
    for (int k = 0; k < DP_COUNTS; ++k)
        cnt[k] = 0;
    for (int tile = blockIdx.x; tile < A.tiles; tile += gridDim.x)
    {
        for (int v = tid; v < DP_TILE; v += T)
        {
            const int64_t i64 = (int64_t)tile * DP_TILE + v;
            double sq_b = 0.0, sq_a = 0.0;
            if (i64 < (int64_t)n)
            {
                const int i = (int)i64;
                const double G[3] = {GT[i], GT[n + i], GT[2 * n + i]};
                const bool prior = lam_in == nullptr;
                double l_in = prior ? 1.0 : lam_in[i], f_in = prior ? 0.0 : info_in[i];
                int o_in = prior ? 0 : nobs_in[i];
                double l_out = l_in, f_out = f_in;
                int o_out = o_in;
                unsigned fl;
                if (!live_mate(G))
                {
                    fl = EBVO_DEPTH_DEAD;
                    ++cnt[0];
                }
                else
                {
                    if (prior)
                    {
                        const double b = sqrt(dot3(A.T21, A.T21));
                        const double s = (A.sigma_disp * G[2]) / (A.Kl[0] * b);
                        f_in = 1.0 / (s * s);
                        f_out = f_in;
                    }
                    const DepthEdge e0 = depth_edge(E0, A.n_e[0], idx0, i);
                    DepthEdge e1;
                    if (A.cameras > 1)
                        e1 = depth_edge(E1, A.n_e[1], idx1, i);
                    else
                    {
                        e1.ex = e1.ey = e1.n0 = e1.n1 = 0.0;
                        e1.has = false;
                    }
                    double r[2], j[2], pix[2], piy[2], yz[2], lam = l_in, h = 0.0;
                    bool surv[2] = {false, false};
                    fl = 0;
                    for (int it = 0;; ++it)
                    {
                        depth_eval(A, G, lam, e0, e1, r, j, pix, piy, yz);
                        if (it == 0)
                        {
#pragma unroll
                            for (int c = 0; c < 2; ++c)
                            {
                                const bool has = c ? e1.has : e0.has;
                                const bool live = has && live_projection(pix[c], piy[c], yz[c], A.margin, A.x_max, A.y_max);
                                const double rho = fabs(r[c]);
                                surv[c] = live && rho <= A.gate && rho < INFINITY;
                                if (live && !surv[c])
                                {
                                    fl |= c ? EBVO_DEPTH_GATED_RIGHT : EBVO_DEPTH_GATED_LEFT;
                                    ++cnt[5 + c];
                                }
                                if (surv[c])
                                    ++cnt[3 + c];
                            }
                            sq_b = 0.0 + ((surv[0] ? r[0] * r[0] : 0.0) + (surv[1] ? r[1] * r[1] : 0.0));
                        }
                        double Sh = 0.0, Sg = 0.0;
#pragma unroll
                        for (int c = 0; c < 2; ++c)
                            if (surv[c])
                            {
                                const double rho = fabs(r[c]);
                                const double w = huber_weight(rho, A.huber);
                                Sh = Sh + w * (j[c] * j[c]);
                                Sg = Sg + w * (j[c] * r[c]);
                            }
                        h = f_in + Sh * A.iv;
                        if (it >= A.iterations)
                            break;
                        const double g = f_in * (lam - l_in) + Sg * A.iv;
                        lam = lam - g / h;
                    }
                    const bool accept = finite_value(lam) && lam >= A.lam_min && lam <= A.lam_max && (surv[0] || surv[1]) && finite_value(h);
                    if (accept)
                    {
                        l_out = lam;
                        f_out = h < A.info_max ? h : A.info_max;
                        o_out = o_in + 1;
                        fl |= EBVO_DEPTH_UPDATED;
                        ++cnt[1];
                        sq_a = 0.0 + ((surv[0] ? r[0] * r[0] : 0.0) + (surv[1] ? r[1] * r[1] : 0.0));
                    }
                    else
                    {
                        fl |= EBVO_DEPTH_RESTORED;
                        ++cnt[2];
                        sq_a = sq_b;
                    }
                }
                lam_out[i] = l_out;
                info_out[i] = f_out;
                nobs_out[i] = o_out;
                flags[i] = (uint8_t)fl;
            }
            wave_sum(sq_b, lane, &part[0][v >> 6]);
            wave_sum(sq_a, lane, &part[1][v >> 6]);
        }
        __syncthreads();
        if (tid < 2)
            tile_sums[2 * (size_t)tile + tid] = group_sum<DP_GROUPS>(part[tid], 1, 0);
        __syncthreads(); // part is written again by the next tile
    }
#pragma unroll
    for (int k = 0; k < DP_COUNTS; ++k)
        wave_count(cnt[k], lane, &counts[k]);
}

__global__ __launch_bounds__(64) void depth_finish_kernel(int tiles, const double *__restrict__ tile_sums, const int32_t *__restrict__ counts,
                                                          DepthRecord *__restrict__ rec)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    double b = 0.0, a = 0.0;
    for (int t = 0; t < tiles; ++t) // ascending tile index from +0.0
    {
        b = b + tile_sums[2 * (size_t)t];
        a = a + tile_sums[2 * (size_t)t + 1];
    }
    const int nt = counts[3] + counts[4];
    rec->rms_before = nt > 0 ? sqrt(b / (double)nt) : 0.0;
    rec->rms_after = nt > 0 ? sqrt(a / (double)nt) : 0.0;
    rec->n_dead = counts[0];
    rec->n_updated = counts[1];
    rec->n_restored = counts[2];
    rec->n_terms[0] = counts[3];
    rec->n_terms[1] = counts[4];
    rec->n_gated[0] = counts[5];
    rec->n_gated[1] = counts[6];
    rec->pad = 0;
}
} // namespace

void depth_scale_enqueue(const Slot &s, double *d_gt, int n_kf, const double *d_lambda)
{
    const int64_t pb = ((int64_t)n_kf + 255) / 256;
    hipLaunchKernelGGL(depth_scale_kernel, dim3(chain_grid_cap(s, (unsigned)(pb > 2048 ? 2048 : pb))), dim3(256), 0, s.stream, d_gt, n_kf, d_lambda);
}

int depth_run(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, int n_kf, const ebvo_edge *d_E0, int n0,
              const ebvo_edge *d_E1, int n1, const int32_t *d_idx0, const int32_t *d_idx1, int img_w, int img_h,
              const ebvo_stereo_calib *cal, const ebvo_depth_params *dp, const double *R, const double *t, const double *d_lam_in,
              const double *d_info_in, const int32_t *d_nobs_in, double *d_lam, double *d_info, int32_t *d_nobs, uint8_t *d_flags,
              DepthRecord *rec)
{
    const int tiles = (n_kf + DP_TILE - 1) / DP_TILE;
    const size_t n = (size_t)n_kf;
    // the record, the seven counters, the tile sums, then the six planes
    const size_t o_rec = 0, o_cnt = round_up64(sizeof(DepthRecord)), o_tiles = o_cnt + round_up64(sizeof(int32_t) * DP_COUNTS),
                 o_gt = o_tiles + round_up64(sizeof(double) * 2 * (size_t)tiles), total = o_gt + round_up64(sizeof(double) * 6 * n);
    if (int rc = ebvo_grow(ctx, s, s.depth_ws, total))
        return rc;
    char *base = (char *)s.depth_ws.p;
    DepthRecord *d_rec = (DepthRecord *)(base + o_rec);
    int32_t *d_cnt = (int32_t *)(base + o_cnt);
    double *d_tiles = (double *)(base + o_tiles), *d_gt = (double *)(base + o_gt);
    DepthArgs A;
    memcpy(A.Kl, cal->K_left, sizeof A.Kl);
    memcpy(A.Kr, cal->K_right, sizeof A.Kr);
    memcpy(A.R21, cal->R21, sizeof A.R21);
    memcpy(A.T21, cal->T21, sizeof A.T21);
    memcpy(A.Rt, R, sizeof(double) * 9);
    memcpy(A.Rt + 9, t, sizeof(double) * 3);
    A.margin = dp->img_margin;
    A.x_max = (double)img_w - dp->img_margin;
    A.y_max = (double)img_h - dp->img_margin;
    A.sigma_disp = dp->sigma_disp_px;
    A.iv = 1.0 / (dp->sigma_normal_px * dp->sigma_normal_px);
    A.huber = dp->huber_px;
    A.gate = dp->gate_px;
    A.lam_min = dp->lambda_min;
    A.lam_max = dp->lambda_max;
    A.info_max = dp->info_max;
    A.n_kf = n_kf;
    A.cameras = dp->cameras;
    A.iterations = dp->iterations;
    A.tiles = tiles;
    A.n_e[0] = n0;
    A.n_e[1] = dp->cameras > 1 ? n1 : 0;
    const int bt = dp->block_threads ? dp->block_threads : DP_TILE;
    hipStream_t st = s.stream;
    {
        ProfScope ps(ctx, s, K_MISC);
        EBVO_HIP(ctx, hipMemsetAsync(d_cnt, 0, sizeof(int32_t) * DP_COUNTS, st));
        align_prepare_enqueue(s, cal, d_kfL, d_kfR, n_kf, d_gt);
        hipLaunchKernelGGL(depth_update_kernel, dim3(chain_grid_cap(s, (unsigned)(tiles > 4096 ? 4096 : tiles))), dim3(bt), 0, st, A, d_gt, d_E0,
                           d_E1, d_idx0, dp->cameras > 1 ? d_idx1 : nullptr, d_lam_in, d_info_in, d_nobs_in, d_lam, d_info, d_nobs, d_flags,
                           d_tiles, d_cnt);
        hipLaunchKernelGGL(depth_finish_kernel, dim3(1), dim3(64), 0, st, tiles, d_tiles, d_cnt, d_rec);
    }
    EBVO_HIP(ctx, hipGetLastError());
    EBVO_HIP(ctx, hipMemcpyAsync(rec, d_rec, sizeof *rec, hipMemcpyDeviceToHost, st));
    return EBVO_OK;
}
