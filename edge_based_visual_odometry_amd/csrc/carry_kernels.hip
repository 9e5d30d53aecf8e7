// Handover of the refined depths to the next keyframe on promotion (ebvo_depth_carry / ebvo_temporal_promote_keyframe).  The
// arithmetic contract is written once in include/ebvo_hip.h; tests/oracle_carry.py restates it on the CPU and the device
// matches it bit for bit.
//   carry_project_kernel   one thread per OLD mate: Gamma and T1 (stereo_gamma_tangent), the source test, Gamma / lambda under
//                          the pose, the projection and the mapped orientation as the alignment's camera 0 forms them.  It
//                          writes the projection as an ebvo_edge (x, y, theta = o, index = i; NaN x and y for a mate that is
//                          not a live source, which grid_cell puts in no cell) and a plane each for zp, a, info, n_obs
//   (the alignment's align_cells / align_cell_scan / align_cell_scatter kernels then build the CSR grid over that list,
//   unchanged: align_grid_enqueue)
//   carry_gather_kernel    ONE lane per NEW mate: Gamma' and the prior, the cell window around the mate's left edge, the
//                          smallest (d2, i), the fusion, the state and the flags.  The old mates are sparse (about 0.03 per
//                          pixel against the alignment's 0.24 edges per pixel): a window of 3 x 3 cells of 4 px holds four or
//                          five projections, so sixteen lanes per item would idle even more than they do in the alignment.
//                          The cells of one window row are neighbours in the CSR, so a row is ONE segment
//                          start[row, x0] .. start[row, x1 + 1]: two offsets and a short loop per row
// The counts are wave sums of integers and one atomic per wave and counter.  The pose, the calibration and the parameters are
// kernel arguments.  No host read between the launches, no spin-wait, no grid-wide barrier (the stream orders them), every loop
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
struct CarryArgs
{
    double Kl[9], Rt[12];
    double margin, x_max, y_max, r2, orient_thr, sigma_disp, carry, gate2, lam_min, lam_max, info_max;
    int32_t n_old, n_new, min_obs, cell, sr, gw, gh, pad;
};

// per old mate, what the gather reads of it
struct CarrySources
{
    ebvo_edge *proj; // [n_old] the projection as an edge
    double *zp, *a, *info;
    int32_t *nobs;
};

__global__ __launch_bounds__(256) void carry_project_kernel(FinalCalib C, CarryArgs A, const ebvo_edge *__restrict__ kfL,
                                                            const ebvo_edge *__restrict__ kfR, const double *__restrict__ lam_in,
                                                            const double *__restrict__ info_in, const int32_t *__restrict__ nobs_in,
                                                            CarrySources S, int32_t *__restrict__ counts)
{
    int n_src = 0, n_live = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < A.n_old; i += gridDim.x * blockDim.x)
    {
        double G[3], T1[3], g1[3], g2[3];
        stereo_gamma_tangent(C, kfL[i], kfR[i], G, T1, g1, g2);
        const double lam = lam_in[i], info = info_in[i];
        const int nobs = nobs_in[i];
        ebvo_edge out;
        out.x = out.y = NAN;
        out.theta = 0.0;
        out.index = i;
        out.pad = 0;
        double zp = 0.0, a = 0.0;
        const bool source = live_mate(G) && finite_value(lam) && lam > 0.0 && info > 0.0 && nobs >= A.min_obs;
        if (source)
        {
            ++n_src;
            const double Gs[3] = {G[0] / lam, G[1] / lam, G[2] / lam};
            double RG[3], X[3], q[3], T2[3];
            pose_point(A.Rt, A.Rt + 9, Gs, RG, X);
            project3(A.Kl, X, q); // the alignment's association, camera 0
            mv3(A.Rt, T1, T2);
            const double o = mapped_orientation(T2, q, C.Kli);
            if (live_projection(q[0], q[1], X[2], A.margin, A.x_max, A.y_max))
            {
                ++n_live;
                out.x = q[0];
                out.y = q[1];
                out.theta = o;
                zp = X[2];
                a = RG[2] / (zp * lam);
            }
        }
        S.proj[i] = out;
        S.zp[i] = zp;
        S.a[i] = a;
        S.info[i] = info;
        S.nobs[i] = nobs;
    }
    const int lane = threadIdx.x & 63;
    wave_count(n_src, lane, &counts[0]);
    wave_count(n_live, lane, &counts[1]);
}

// start == nullptr: no association was launched, every live mate is at its prior
__global__ __launch_bounds__(256) void carry_gather_kernel(FinalCalib C, CarryArgs A, const ebvo_edge *__restrict__ newL,
                                                           const ebvo_edge *__restrict__ newR, CarrySources S,
                                                           const int32_t *__restrict__ start, const int32_t *__restrict__ list,
                                                           double *__restrict__ lam_out, double *__restrict__ info_out,
                                                           int32_t *__restrict__ nobs_out, uint8_t *__restrict__ flags,
                                                           int32_t *__restrict__ src, int32_t *__restrict__ counts)
{
    int n_dead = 0, n_assoc = 0, n_carried = 0, n_gated = 0;
    for (int m = blockIdx.x * blockDim.x + threadIdx.x; m < A.n_new; m += gridDim.x * blockDim.x)
    {
        const ebvo_edge e = newL[m];
        double G[3], T1[3], g1[3], g2[3];
        stereo_gamma_tangent(C, e, newR[m], G, T1, g1, g2);
        double l_out = 1.0, f_out = 0.0;
        int o_out = 0, best_i = -1;
        unsigned fl = 0;
        if (!live_mate(G))
        {
            fl = EBVO_DEPTH_DEAD;
            ++n_dead;
        }
        else
        {
            const double b = sqrt(dot3(C.T21, C.T21));
            const double s = (A.sigma_disp * G[2]) / (A.Kl[0] * b);
            const double info0 = 1.0 / (s * s);
            f_out = info0;
            const int cx = grid_cell(e.x, A.cell, A.gw), cy = grid_cell(e.y, A.cell, A.gh);
            if (start && cx >= 0 && cy >= 0)
            {
                double best_d2 = INFINITY;
                int best = 0x7fffffff;
                const int y0 = max(cy - A.sr, 0), y1 = min(cy + A.sr, A.gh - 1);
                const int x0 = max(cx - A.sr, 0), x1 = min(cx + A.sr, A.gw - 1);
                for (int ry = y0; ry <= y1; ++ry)
                {
                    // the cells x0 .. x1 of a row are one segment of the list
                    const int ka = start[ry * A.gw + x0], kb = start[ry * A.gw + x1 + 1];
                    for (int k = ka; k < kb; ++k)
                    {
                        const int i = list[k];
                        const ebvo_edge p = S.proj[i];
                        const double dx = p.x - e.x, dy = p.y - e.y;
                        const double d2 = dx * dx + dy * dy;
                        if (d2 <= A.r2 && orient_close(p.theta, e.theta, A.orient_thr) && (d2 < best_d2 || (d2 == best_d2 && i < best)))
                        {
                            best_d2 = d2;
                            best = i;
                        }
                    }
                }
                if (best != 0x7fffffff)
                    best_i = best;
            }
            if (best_i >= 0)
            {
                ++n_assoc;
                const double lm = G[2] / S.zp[best_i];
                const double c = lm * S.a[best_i];
                const double im = (A.carry * S.info[best_i]) / (c * c);
                bool ok = finite_value(im) && im > 0.0;
                if (ok)
                {
                    const double d = lm - 1.0;
                    const double v = 1.0 / info0 + 1.0 / im;
                    ok = lm >= A.lam_min && lm <= A.lam_max && d * d <= A.gate2 * v;
                }
                if (ok)
                {
                    const double h = info0 + im;
                    l_out = (info0 + im * lm) / h;
                    f_out = h < A.info_max ? h : A.info_max;
                    o_out = S.nobs[best_i];
                    fl = EBVO_DEPTH_CARRIED;
                    ++n_carried;
                }
                else
                {
                    fl = EBVO_DEPTH_CARRY_GATED;
                    ++n_gated;
                }
            }
        }
        lam_out[m] = l_out;
        info_out[m] = f_out;
        nobs_out[m] = o_out;
        flags[m] = (uint8_t)fl;
        src[m] = best_i;
    }
    const int lane = threadIdx.x & 63;
    wave_count(n_dead, lane, &counts[2]);
    wave_count(n_assoc, lane, &counts[3]);
    wave_count(n_carried, lane, &counts[4]);
    wave_count(n_gated, lane, &counts[5]);
}

} // namespace

int carry_run(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_oldL, const ebvo_edge *d_oldR, int n_old, const double *d_lam_in,
              const double *d_info_in, const int32_t *d_nobs_in, const ebvo_edge *d_newL, const ebvo_edge *d_newR, int n_new, int img_w,
              int img_h, const ebvo_stereo_calib *cal, const ebvo_depth_carry_params *cp, const double *R, const double *t, double *d_lam,
              double *d_info, int32_t *d_nobs, uint8_t *d_flags, int32_t *d_src, int32_t *counts)
{
    const bool assoc = d_lam_in && n_old > 0;
    const int cell = cp->cell_size;
    const int gw = (int)(((int64_t)img_w + cell - 1) / cell), gh = (int)(((int64_t)img_h + cell - 1) / cell), n_cells = gw * gh;
    const size_t no = assoc ? (size_t)n_old : 0;
    // the counters, the projections, their four planes, the grid
    const size_t o_cnt = 0, o_proj = round_up64(sizeof(int32_t) * CARRY_COUNTS), o_zp = o_proj + round_up64(sizeof(ebvo_edge) * no),
                 o_a = o_zp + round_up64(8 * no), o_info = o_a + round_up64(8 * no), o_nobs = o_info + round_up64(8 * no), o_grid = o_nobs + round_up64(4 * no),
                 total = o_grid + (assoc ? round_up64(sizeof(int32_t) * align_grid_ints(n_old, n_cells)) : 0);
    if (int rc = ebvo_grow(ctx, s, s.carry_ws, total))
        return rc;
    char *base = (char *)s.carry_ws.p;
    int32_t *d_cnt = (int32_t *)(base + o_cnt);
    CarrySources S;
    S.proj = (ebvo_edge *)(base + o_proj);
    S.zp = (double *)(base + o_zp);
    S.a = (double *)(base + o_a);
    S.info = (double *)(base + o_info);
    S.nobs = (int32_t *)(base + o_nobs);
    const FinalCalib C = final_calib_host(cal->K_left, cal->K_right, cal->R21, cal->T21);
    CarryArgs A;
    memcpy(A.Kl, cal->K_left, sizeof A.Kl);
    memcpy(A.Rt, R, sizeof(double) * 9);
    memcpy(A.Rt + 9, t, sizeof(double) * 3);
    A.margin = cp->img_margin;
    A.x_max = (double)img_w - cp->img_margin;
    A.y_max = (double)img_h - cp->img_margin;
    A.r2 = cp->radius * cp->radius;
    A.orient_thr = cp->orient_thr_deg;
    A.sigma_disp = cp->sigma_disp_px;
    A.carry = cp->carry;
    A.gate2 = cp->gate_sigmas * cp->gate_sigmas;
    A.lam_min = cp->lambda_min;
    A.lam_max = cp->lambda_max;
    A.info_max = cp->info_max;
    A.n_old = n_old;
    A.n_new = n_new;
    A.min_obs = cp->min_obs;
    A.cell = cell;
    A.sr = (int)ceil(cp->radius / cell);
    A.gw = gw;
    A.gh = gh;
    A.pad = 0;
    hipStream_t st = s.stream;
    const int32_t *d_start = nullptr, *d_list = nullptr;
    {
        ProfScope ps(ctx, s, K_MISC);
        EBVO_HIP(ctx, hipMemsetAsync(d_cnt, 0, sizeof(int32_t) * CARRY_COUNTS, st));
        if (assoc)
        {
            const int64_t ob = ((int64_t)n_old + 255) / 256;
            hipLaunchKernelGGL(carry_project_kernel, dim3(chain_grid_cap(s, (unsigned)(ob > 2048 ? 2048 : ob))), dim3(256), 0, st, C, A, d_oldL,
                               d_oldR, d_lam_in, d_info_in, d_nobs_in, S, d_cnt);
            if (int rc = align_grid_enqueue(ctx, s, S.proj, n_old, cell, gw, gh, (int32_t *)(base + o_grid), &d_start, &d_list))
                return rc;
        }
        const int64_t nb = ((int64_t)n_new + 255) / 256;
        hipLaunchKernelGGL(carry_gather_kernel, dim3(chain_grid_cap(s, (unsigned)(nb > 2048 ? 2048 : nb))), dim3(256), 0, st, C, A, d_newL,
                           d_newR, S, d_start, d_list, d_lam, d_info, d_nobs, d_flags, d_src, d_cnt);
    }
    EBVO_HIP(ctx, hipGetLastError());
    EBVO_HIP(ctx, hipMemcpyAsync(counts, d_cnt, sizeof(int32_t) * CARRY_COUNTS, hipMemcpyDeviceToHost, st));
    return EBVO_OK;
}
