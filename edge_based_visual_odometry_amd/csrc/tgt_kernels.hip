// tgt_kernels.hip -- ground-truth evaluation of the temporal chain from a relative pose, on gfx950.
//
// Replaces, in the reference (the has_gt() == true branch of the temporal chain):
//   Temporal_Matches::build_Veridical_Quads                     src/Temporal_Matches.cpp:57-166
//   Temporal_Matches::orientation_mapping                       src/Temporal_Matches.cpp:294-333
//   SpatialGrid::getCandidatesWithinRadius(cv::Point2d, r)       include/Dataset.h:92-113
//   Temporal_Matches::Evaluate_Temporal_Edge_Pairs_on_Quads      src/Temporal_Matches.cpp:220-292 (per-row counts)
//
// tgt_project: one thread per keyframe mate (its second instantiation is the projection of a pose prior,
// ebvo_temporal_set_prior: the same arithmetic plus a depth test).  tgt_veridical: sixteen lanes per keyframe mate walk the grid cells of the
// current-frame mates that match_kernels.hip builds (the layout and the order of temporal_candidates_kernel: dy outer, dx
// inner, ascending mate index within a cell; a ballot ranks the survivors of a step).  tgt_rows: eight lanes per row of a
// CSR list of quads.  tgt_grid_rows: the grid stage of the chain (apply_spatial_grid_filtering_quads, :335-383), which
// temporal_candidates_kernel fuses with the orientation test and so never lists, counted and evaluated per keyframe mate
// with the same sixteen-lane walk.  No floating-point value is accumulated on the device: the kernels produce integer (n, tp) per row
// and a byte per quad, the stage totals are gt_totals' integer atomics, and the four doubles of a stage are summed on the
// host in keyframe index order (ebvo_capi.hip: tgt_stage_doubles).
//
// Compiled with -ffp-contract=off like the rest.
#include "ebvo_geom.h"
#include "ebvo_internal.h"
#include "ebvo_math.h"

namespace
{

struct TgtPose
{
    double R[9], t[3], Kl[9], Kr[9];
    double R21R[9]; // (R_stereo * rel_pose.R) of :321: the expression binds left to right, the 3x3 product comes first
    FinalCalib C;   // K_left^-1, K_right^-1, R21, T21
};

// :82-105 for one keyframe mate: both projections (over their own z), both mapped orientations and the two camera-frame
// points.  Shared by tgt_project_kernel and tprior_project_kernel, so that the prior stage searches at exactly the points
// the ground truth evaluates.  The pose step, project3 (:84-85) and mapped_orientation (:294-333) are ebvo_geom.h's, which
// the alignment and the depth carry project with too.
struct MateProjection
{
    double ql[3], qr[3], ol, orr, Gc[3], Gr[3];
};

__device__ inline void project_mate(const TgtPose &P, const ebvo_edge &kl, const ebvo_edge &kr, const double *gamma_i, MateProjection &m)
{
    double G[3], T1[3], g1[3], g2[3];
    stereo_gamma_tangent(P.C, kl, kr, G, T1, g1, g2); // T_1 of :312; G: the triangulated Gamma
    if (gamma_i)
    {
        G[0] = gamma_i[0];
        G[1] = gamma_i[1];
        G[2] = gamma_i[2];
    }
    double RG[3], T2l[3], T2r[3];
    pose_point(P.R, P.t, G, RG, m.Gc); // :83
    project3(P.Kl, m.Gc, m.ql);
    stereo_point(P.C.R21, P.C.T21, m.Gc, m.Gr); // :87
    project3(P.Kr, m.Gr, m.qr);
    mv3(P.R, T1, T2l);    // :317
    mv3(P.R21R, T1, T2r); // :321
    m.ol = mapped_orientation(T2l, m.ql, P.C.Kli);
    m.orr = mapped_orientation(T2r, m.qr, P.C.Kri);
}

// :100-105, both cameras against ONE width and height.  A projection with a NaN coordinate is not in the image (the
// reference would cast it to an int, which is undefined); neither is an infinite one.
__device__ inline bool projections_inside(const MateProjection &m, double margin, double x_max, double y_max)
{
    return inside_margin(m.ql[0], m.ql[1], margin, x_max, y_max) && inside_margin(m.qr[0], m.qr[1], margin, x_max, y_max);
}

// :82-105 per keyframe mate.  The orientations are computed before the margin test, as there.
// DEPTH = false: the ground truth's in_image.  DEPTH = true (the pose prior of ebvo_temporal_set_prior): the byte is `live`,
// which also asks for a positive depth in both cameras -- a point behind a camera projects into the image mirrored.
template <bool DEPTH>
__global__ __launch_bounds__(256) void tgt_project_kernel(const ebvo_edge *__restrict__ kfL, const ebvo_edge *__restrict__ kfR,
                                                          const double *__restrict__ gamma, int n, TgtPose P, double margin,
                                                          double x_max, double y_max, uint8_t *__restrict__ in_image,
                                                          double *__restrict__ pl, double *__restrict__ pr,
                                                          double *__restrict__ ol, double *__restrict__ orr)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        MateProjection m;
        project_mate(P, kfL[i], kfR[i], gamma ? gamma + (size_t)i * 3 : nullptr, m);
        ol[i] = m.ol;
        orr[i] = m.orr;
        pl[(size_t)i * 2] = m.ql[0];
        pl[(size_t)i * 2 + 1] = m.ql[1];
        pr[(size_t)i * 2] = m.qr[0];
        pr[(size_t)i * 2 + 1] = m.qr[1];
        bool inside = projections_inside(m, margin, x_max, y_max);
        if (DEPTH)
            inside = inside && m.Gc[2] > 0.0 && m.Gr[2] > 0.0;
        in_image[i] = inside ? 1 : 0;
    }
}

struct VerArgs
{
    const uint8_t *in_image;
    const double *pl, *pr, *ol, *orr;
    const ebvo_edge *cfL, *cfR;
    const MateCells *cells;
    const int32_t *cell_start, *cell_list;
    const uint8_t *is_tp;
    int n_kf, cell, sr, gw, gh;
    double dist_thr, orient_thr;
};

// :107-144 per keyframe mate whose projections are in the image.  FILL = false: cnt[i]; FILL = true: the mate indices at
// row_ptr[i] (never past cap) and on[i] = a veridical quad exists and the keyframe mate is a true positive (:233).
template <bool FILL>
__global__ __launch_bounds__(256) void tgt_veridical_kernel(VerArgs A, int32_t *__restrict__ cnt, const int32_t *__restrict__ row_ptr,
                                                            int32_t *__restrict__ idx, int64_t cap, uint8_t *__restrict__ on)
{
    const int lane = threadIdx.x & 63, e = lane & 15, gshift = lane & 48;
    const int groups = (gridDim.x * blockDim.x) >> 4;
    const int sr = A.sr, gw = A.gw, gh = A.gh;
    // the four groups of a wave advance together; a group past the end, or of a mate outside the image, walks nothing
    for (int w0 = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 4; w0 < A.n_kf; w0 += groups)
    {
        const int i0 = w0 + (lane >> 4);
        const bool have = i0 < A.n_kf;
        const int i = have ? i0 : 0;
        const bool live = have && A.in_image[i] != 0;
        const double plx = A.pl[(size_t)i * 2], ply = A.pl[(size_t)i * 2 + 1], prx = A.pr[(size_t)i * 2], pry = A.pr[(size_t)i * 2 + 1];
        const double po_l = A.ol[i], po_r = A.orr[i];
        // static_cast<int>(e_location.x) / cell_size (include/Dataset.h:95-96); inside the margin the casts are defined
        const int qlx = live ? (int)plx / A.cell : 0, qly = live ? (int)ply / A.cell : 0;
        const int qrx = live ? (int)prx / A.cell : 0, qry = live ? (int)pry / A.cell : 0;
        const int dy0 = max(-sr, -qly), dy1 = live ? min(sr, gh - 1 - qly) : dy0 - 1;
        const int dx0 = max(-sr, -qlx), dx1 = min(sr, gw - 1 - qlx);
        int c = 0;
        int64_t o = (FILL && have) ? row_ptr[i] : 0;
        for (int dy = dy0; dy <= dy1; ++dy)
            for (int dx = dx0; dx <= dx1; ++dx)
            {
                const int ny = qly + dy, nx = qlx + dx;
                const bool in_grid = live && ny >= 0 && ny < gh && nx >= 0 && nx < gw;
                const int a = in_grid ? A.cell_start[ny * gw + nx] : 0, b = in_grid ? A.cell_start[ny * gw + nx + 1] : 0;
                for (int k0 = a; __any(k0 < b); k0 += 16)
                {
                    const int k = k0 + e;
                    bool ok = false;
                    int j = 0;
                    if (k < b)
                    {
                        j = A.cell_list[k];
                        const MateCells m = A.cells[j];
                        // right_set.find(cf_idx) (:114): the mate's right edge is in the right grid and in a neighbour cell
                        // of the right projection's cell
                        if (m.rx >= 0 && abs(m.rx - qrx) <= sr && abs(m.ry - qry) <= sr)
                        {
                            const ebvo_edge l = A.cfL[j], r = A.cfR[j];
                            const double dxl = l.x - plx, dyl = l.y - ply, dxr = r.x - prx, dyr = r.y - pry;
                            ok = sqrt(dxl * dxl + dyl * dyl) < A.dist_thr && sqrt(dxr * dxr + dyr * dyr) < A.dist_thr && // :131, :133
                                 orient_close(po_l, l.theta, A.orient_thr) && orient_close(po_r, r.theta, A.orient_thr);
                        }
                    }
                    const unsigned hits = (unsigned)((__ballot(ok) >> gshift) & 0xffffull);
                    if (FILL && ok)
                    {
                        const int64_t pos = o + __popc(hits & ((1u << e) - 1u));
                        if (pos < cap)
                            idx[pos] = j;
                    }
                    const int nh = __popc(hits);
                    c += nh;
                    o += nh;
                }
            }
        if (have && e == 0)
        {
            if (FILL)
                on[i] = (c > 0 && (!A.is_tp || A.is_tp[i] != 0)) ? 1 : 0;
            else
                cnt[i] = c;
        }
    }
}

// Evaluate_Temporal_Edge_Pairs_on_Quads' inner loop (:242-257) on a CSR list: eight lanes per row.  The centres of quad k are
// cenL[k] / cenR[k], or cfL / cfR [col_idx[k]]; keep (optional): only quads with keep[k] != 0 are in the list.  is_tp[k] is
// written for the listed quads of the rows that are on (zeroed beforehand).
__global__ __launch_bounds__(256) void tgt_rows_kernel(const int32_t *__restrict__ row_ptr, const ebvo_edge *__restrict__ cenL,
                                                       const ebvo_edge *__restrict__ cenR, const int32_t *__restrict__ col_idx,
                                                       const ebvo_edge *__restrict__ cfL, const ebvo_edge *__restrict__ cfR,
                                                       const uint8_t *__restrict__ keep, const double *__restrict__ pl,
                                                       const double *__restrict__ pr, const uint8_t *__restrict__ on, int n_kf,
                                                       double tp_dist, int32_t *__restrict__ out, uint8_t *__restrict__ is_tp)
{
    const int lane = threadIdx.x & 63, e = lane & 7, gshift = lane & ~7;
    const int rows_per_pass = (gridDim.x * blockDim.x) >> 3;
    const int first = (blockIdx.x * blockDim.x + threadIdx.x) >> 3;
    // every lane of a wave runs the same number of passes (the ballots below need the whole wave)
    for (int base = 0; base < n_kf; base += rows_per_pass)
    {
        const int i = base + first;
        const bool live = i < n_kf && on[i];
        const int b = live ? row_ptr[i] : 0, len = live ? row_ptr[i + 1] - b : 0;
        const double glx = live ? pl[(size_t)i * 2] : 0.0, gly = live ? pl[(size_t)i * 2 + 1] : 0.0;
        const double grx = live ? pr[(size_t)i * 2] : 0.0, gry = live ? pr[(size_t)i * 2 + 1] : 0.0;
        int n = 0, tp = 0;
        int maxlen = len;
        for (int d = 32; d > 0; d >>= 1)
            maxlen = max(maxlen, __shfl_xor(maxlen, d));
        for (int k0 = 0; k0 < maxlen; k0 += 8)
        {
            const int k = k0 + e;
            bool in = k < len;
            if (in && keep)
                in = keep[b + k] != 0;
            bool hit = false;
            if (in)
            {
                const ebvo_edge &l = cenL ? cenL[b + k] : cfL[col_idx[b + k]];
                const ebvo_edge &r = cenR ? cenR[b + k] : cfR[col_idx[b + k]];
                const double dxl = l.x - glx, dyl = l.y - gly, dxr = r.x - grx, dyr = r.y - gry;
                hit = sqrt(dxl * dxl + dyl * dyl) < tp_dist && sqrt(dxr * dxr + dyr * dyr) < tp_dist; // :248, strict
                is_tp[b + k] = hit ? 1 : 0;
            }
            n += __popcll((__ballot(in) >> gshift) & 0xffull);
            tp += __popcll((__ballot(hit) >> gshift) & 0xffull);
        }
        if (e == 0 && i < n_kf)
        {
            out[(size_t)i * 2] = n;
            out[(size_t)i * 2 + 1] = tp;
        }
    }
}

// "Location Proximity": the output of apply_spatial_grid_filtering_quads (src/Temporal_Matches.cpp:335-383) evaluated by
// :242-257 without forming it.  The walk is temporal_candidates_kernel's (match_kernels.hip) less its orientation test:
// sixteen lanes per keyframe mate, the query cells of the mate's own edges (not clipped), the neighbours inside the grid,
// a current-frame mate counted when its right cell is in the right grid and within sr cells of the right query cell.
// Every counted mate is a quad of the row; it is a true positive when both its edges lie < tp_dist from the row's
// projections.  A row that is off walks nothing and writes (0, 0).
// PRIOR = true: the match searched under a pose prior (ebvo_temporal_set_prior), so the query cells are those of the
// prior's projections Q.pl / Q.pr and a mate that was not live walked nothing: its row is (0, 0).
template <bool PRIOR>
__global__ __launch_bounds__(256) void tgt_grid_rows_kernel(const ebvo_edge *__restrict__ kfL, const ebvo_edge *__restrict__ kfR,
                                                            int n_kf, const ebvo_edge *__restrict__ cfL,
                                                            const ebvo_edge *__restrict__ cfR, const MateCells *__restrict__ cells,
                                                            const int32_t *__restrict__ cell_start,
                                                            const int32_t *__restrict__ cell_list, int cell, int sr, int gw, int gh,
                                                            const uint8_t *__restrict__ on, const double *__restrict__ pl,
                                                            const double *__restrict__ pr, double tp_dist, int32_t *__restrict__ out,
                                                            TemporalPrior Q)
{
    const int lane = threadIdx.x & 63, e = lane & 15, gshift = lane & 48;
    const int groups = (gridDim.x * blockDim.x) >> 4;
    // the four groups of a wave advance together (the ballots below are wave-wide): a group past the end, or of a row that
    // is off, walks nothing
    for (int w0 = ((blockIdx.x * blockDim.x + threadIdx.x) >> 6) * 4; w0 < n_kf; w0 += groups)
    {
        const int i0 = w0 + (lane >> 4);
        const bool have = i0 < n_kf;
        const int i = have ? i0 : 0;
        const bool live = have && on[i] != 0 && (!PRIOR || Q.live[i] != 0);
        const double plx = pl[(size_t)i * 2], ply = pl[(size_t)i * 2 + 1], prx = pr[(size_t)i * 2], pry = pr[(size_t)i * 2 + 1];
        int qlx, qly, qrx, qry;
        if (PRIOR)
        {
            // a live mate's projections lie inside the image: the casts are defined
            qlx = live ? (int)Q.pl[(size_t)i * 2] / cell : 0, qly = live ? (int)Q.pl[(size_t)i * 2 + 1] / cell : 0;
            qrx = live ? (int)Q.pr[(size_t)i * 2] / cell : 0, qry = live ? (int)Q.pr[(size_t)i * 2 + 1] / cell : 0;
        }
        else
        {
            const ebvo_edge kl = kfL[i], kr = kfR[i];
            qlx = (int)kl.x / cell, qly = (int)kl.y / cell, qrx = (int)kr.x / cell, qry = (int)kr.y / cell;
        }
        const int dy0 = max(-sr, -qly), dy1 = live ? min(sr, gh - 1 - qly) : dy0 - 1;
        const int dx0 = max(-sr, -qlx), dx1 = min(sr, gw - 1 - qlx);
        int n = 0, tp = 0;
        for (int dy = dy0; dy <= dy1; ++dy)
            for (int dx = dx0; dx <= dx1; ++dx)
            {
                const int ny = qly + dy, nx = qlx + dx;
                const bool in_grid = live && ny >= 0 && ny < gh && nx >= 0 && nx < gw;
                const int a = in_grid ? cell_start[ny * gw + nx] : 0, b = in_grid ? cell_start[ny * gw + nx + 1] : 0;
                for (int k0 = a; __any(k0 < b); k0 += 16)
                {
                    const int k = k0 + e;
                    bool in = false, hit = false;
                    if (k < b)
                    {
                        const int j = cell_list[k];
                        const MateCells m = cells[j];
                        in = m.rx >= 0 && abs(m.rx - qrx) <= sr && abs(m.ry - qry) <= sr; // right_set.count(cf_idx), :357
                        if (in)
                        {
                            const ebvo_edge l = cfL[j], r = cfR[j];
                            const double dxl = l.x - plx, dyl = l.y - ply, dxr = r.x - prx, dyr = r.y - pry;
                            hit = sqrt(dxl * dxl + dyl * dyl) < tp_dist && sqrt(dxr * dxr + dyr * dyr) < tp_dist; // :246-248, strict
                        }
                    }
                    n += __popcll((__ballot(in) >> gshift) & 0xffffull);
                    tp += __popcll((__ballot(hit) >> gshift) & 0xffffull);
                }
            }
        if (have && e == 0)
        {
            out[(size_t)i * 2] = n;
            out[(size_t)i * 2 + 1] = tp;
        }
    }
}

int tgt_grid(const ebvo_ctx *ctx, int64_t items, int per_block)
{
    int64_t g = (items + per_block - 1) / per_block;
    const int64_t most = ctx->gt_blocks > 0 ? ctx->gt_blocks : 8192; // developer key 21 caps these grids too
    g = g < 1 ? 1 : g;
    return (int)(g < most ? g : most);
}

} // namespace

static TgtPose tgt_pose_host(const double *R, const double *t, const ebvo_stereo_calib *calib)
{
    TgtPose P;
    P.C = final_calib_host(calib->K_left, calib->K_right, calib->R21, calib->T21);
    for (int k = 0; k < 9; ++k)
    {
        P.R[k] = R[k];
        P.Kl[k] = calib->K_left[k];
        P.Kr[k] = calib->K_right[k];
    }
    for (int k = 0; k < 3; ++k)
        P.t[k] = t[k];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            P.R21R[i * 3 + j] = (calib->R21[i * 3] * R[j] + calib->R21[i * 3 + 1] * R[3 + j]) + calib->R21[i * 3 + 2] * R[6 + j];
    return P;
}

int tgt_project_enqueue(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, const double *d_gamma, int n_kf,
                        const double *R, const double *t, const ebvo_stereo_calib *calib, double margin, int img_w, int img_h,
                        uint8_t *d_in, double *d_pl, double *d_pr, double *d_ol, double *d_or)
{
    if (n_kf <= 0)
        return EBVO_OK;
    const TgtPose P = tgt_pose_host(R, t, calib);
    ProfScope ps(ctx, s, K_TGT_PROJECT);
    // get_left_width() - img_margin (:101): the same bound for both cameras
    hipLaunchKernelGGL(tgt_project_kernel<false>, dim3(tgt_grid(ctx, n_kf, 256)), dim3(256), 0, s.stream, d_kfL, d_kfR, d_gamma, n_kf, P,
                       margin, (double)img_w - margin, (double)img_h - margin, d_in, d_pl, d_pr, d_ol, d_or);
    EBVO_HIP(ctx, hipGetLastError());
    return EBVO_OK;
}

int tprior_project_enqueue(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, int n_kf, const double *R,
                           const double *t, const ebvo_stereo_calib *calib, double margin, int img_w, int img_h, uint8_t *d_live,
                           double *d_pl, double *d_pr, double *d_ol, double *d_or)
{
    if (n_kf <= 0)
        return EBVO_OK;
    const TgtPose P = tgt_pose_host(R, t, calib);
    ProfScope ps(ctx, s, K_TGT_PROJECT);
    // inside temporal_stage0_enqueue developer key 22 caps the grid as it caps every other launch of the chain
    hipLaunchKernelGGL(tgt_project_kernel<true>, dim3(chain_grid_cap(s, (unsigned)tgt_grid(ctx, n_kf, 256))), dim3(256), 0, s.stream, d_kfL,
                       d_kfR, (const double *)nullptr, n_kf, P, margin, (double)img_w - margin, (double)img_h - margin, d_live, d_pl, d_pr,
                       d_ol, d_or);
    EBVO_HIP(ctx, hipGetLastError());
    return EBVO_OK;
}

int tgt_veridical_enqueue(ebvo_ctx *ctx, Slot &s, int n_kf, const uint8_t *d_in, const double *d_pl, const double *d_pr,
                          const double *d_ol, const double *d_or, const ebvo_edge *d_cfL, const ebvo_edge *d_cfR, const void *d_grid,
                          int n_cf, int cell, int sr, int gw, int gh, double dist_thr, double orient_thr, const uint8_t *d_is_tp,
                          int32_t *d_cnt, const int32_t *d_row_ptr, int32_t *d_idx, int64_t cap, uint8_t *d_on)
{
    if (n_kf <= 0)
        return EBVO_OK;
    VerArgs A;
    A.in_image = d_in; A.pl = d_pl; A.pr = d_pr; A.ol = d_ol; A.orr = d_or;
    A.cfL = d_cfL; A.cfR = d_cfR;
    match_temporal_grid_view(d_grid, n_cf, gw * gh, &A.cells, &A.cell_start, &A.cell_list);
    A.is_tp = d_is_tp;
    A.n_kf = n_kf; A.cell = cell; A.sr = sr; A.gw = gw; A.gh = gh;
    A.dist_thr = dist_thr; A.orient_thr = orient_thr;
    const dim3 grid(tgt_grid(ctx, n_kf, 16)); // 16 mates per block of 256 threads
    ProfScope ps(ctx, s, K_TGT_VERIDICAL);
    if (d_row_ptr)
        hipLaunchKernelGGL(tgt_veridical_kernel<true>, grid, dim3(256), 0, s.stream, A, d_cnt, d_row_ptr, d_idx, cap, d_on);
    else
        hipLaunchKernelGGL(tgt_veridical_kernel<false>, grid, dim3(256), 0, s.stream, A, d_cnt, d_row_ptr, d_idx, cap, d_on);
    EBVO_HIP(ctx, hipGetLastError());
    return EBVO_OK;
}

int tgt_grid_rows_enqueue(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, int n_kf, const ebvo_edge *d_cfL,
                          const ebvo_edge *d_cfR, const void *d_grid, int n_cf, int cell, int sr, int gw, int gh, const uint8_t *d_on,
                          const double *d_pl, const double *d_pr, double tp_dist, int32_t *d_rows, unsigned long long *d_tot,
                          const TemporalPrior *prior)
{
    if (n_kf > 0)
    {
        const MateCells *cells;
        const int32_t *cell_start, *cell_list;
        match_temporal_grid_view(d_grid, n_cf, gw * gh, &cells, &cell_start, &cell_list);
        ProfScope ps(ctx, s, K_TGT_GRID);
        const dim3 grid(tgt_grid(ctx, n_kf, 16));
        if (prior)
            hipLaunchKernelGGL(tgt_grid_rows_kernel<true>, grid, dim3(256), 0, s.stream, d_kfL, d_kfR, n_kf, d_cfL, d_cfR, cells, cell_start,
                               cell_list, cell, sr, gw, gh, d_on, d_pl, d_pr, tp_dist, d_rows, *prior);
        else
            hipLaunchKernelGGL(tgt_grid_rows_kernel<false>, grid, dim3(256), 0, s.stream, d_kfL, d_kfR, n_kf, d_cfL, d_cfR, cells, cell_start,
                               cell_list, cell, sr, gw, gh, d_on, d_pl, d_pr, tp_dist, d_rows, TemporalPrior{});
        EBVO_HIP(ctx, hipGetLastError());
    }
    return gt_totals_enqueue(ctx, s, d_rows, d_on, n_kf, d_tot);
}

int tgt_rows_enqueue(ebvo_ctx *ctx, Slot &s, const int32_t *d_row_ptr, const ebvo_edge *d_cenL, const ebvo_edge *d_cenR,
                     const int32_t *d_col_idx, const ebvo_edge *d_cfL, const ebvo_edge *d_cfR, const uint8_t *d_keep,
                     const double *d_pl, const double *d_pr, const uint8_t *d_on, int n_kf, int64_t n_quads, double tp_dist,
                     int32_t *d_rows, uint8_t *d_is_tp, unsigned long long *d_tot)
{
    if (n_quads > 0)
        EBVO_HIP(ctx, hipMemsetAsync(d_is_tp, 0, (size_t)n_quads, s.stream));
    if (n_kf > 0)
    {
        ProfScope ps(ctx, s, K_TGT_ROWS);
        hipLaunchKernelGGL(tgt_rows_kernel, dim3(tgt_grid(ctx, n_kf, 32)), dim3(256), 0, s.stream, d_row_ptr, d_cenL, d_cenR, d_col_idx,
                           d_cfL, d_cfR, d_keep, d_pl, d_pr, d_on, n_kf, tp_dist, d_rows, d_is_tp);
        EBVO_HIP(ctx, hipGetLastError());
    }
    return gt_totals_enqueue(ctx, s, d_rows, d_on, n_kf, d_tot);
}
