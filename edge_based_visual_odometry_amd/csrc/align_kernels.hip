// Alignment of the relative pose to the current frame's TOED edges by normal distance (ebvo_pose_align_edges /
// ebvo_temporal_align_pose).  The arithmetic contract is written once in include/ebvo_hip.h; tests/oracle_align.py restates
// it on the CPU and the device matches it bit for bit.
//   align_prepare_kernel     one thread per keyframe mate: Gamma and the 3-D tangent T1 (stereo_gamma_tangent), six planes;
//                            they do not depend on the pose, so a call forms them once
//   align_cells_kernel       the cell of every TOED edge of one image and the cell populations; align_cell_scan_kernel and
//                            align_cell_scatter_kernel make the CSR grid (twins of the temporal grid's kernels in
//                            match_kernels.hip, which take mates, not edges).  No sort pass: the association takes the
//                            smallest (d2, j), which no traversal order enters
//   align_associate_kernel   sixteen lanes per (mate, camera): the projection and the mapped orientation under the pose IN
//                            DEVICE MEMORY, a walk over the cells within sr of the projection's cell, every lane its own best
//                            (d2, j), a 16-lane min-reduce, then the edge index and the planes the fit reads
//   align_sums_kernel        one workgroup per tile of 1024 mates: the tile's 28 sums (a 64-lane halving tree per value, the
//                            16 group sums through LDS and the same tree).  The workgroup that finishes last -- one integer
//                            counter behind a __threadfence, no waiting -- adds the tiles in ascending order, then runs the
//                            round's decisions, the 6 x 6 Cholesky and Exp and writes the pose and the loop's state back to
//                            device memory.  Every launch of every round is enqueued up front; a launch that finds its round
//                            finished or the call ended returns at once
//   align_metric_kernel      after the last association: n_assoc, inliers and the tile sums of r r; the last workgroup
//                            writes the result record
// No host read between steps or rounds, no spin-wait, no grid-wide barrier; every loop is bounded by its arguments.
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
constexpr int AL_TILE = 1024; // mates per tile = virtual lanes of a workgroup
constexpr int AL_GROUPS = AL_TILE / 64;
constexpr int AL_SUMS = 28;   // 21 upper entries of H (row-major, i <= j), 6 of g, the cost

// the call's constants: kernel arguments
struct AlignArgs
{
    double Kl[9], Kr[9], Kli[9], Kri[9], R21[9], T21[3];
    double margin, x_max, y_max, r2, orient_thr, huber, inlier, eps;
    int32_t n_kf, cameras, iterations, min_terms, cell, sr, gw, gh, tiles;
};

// the pose and the loop's state: device memory, written by the call itself (align_init_kernel, then the last workgroup of
// every align_sums launch)
struct AlignState
{
    double Rt[12], Pv[12]; // the pose (R row-major, then t), and the one before the last step
    double c_first, c_last, c_prev;
    int32_t status, stop, rounds_run, steps, fit_terms;
    int32_t go;      // the round's loop goes on: the next align_sums launch of this round has work
    int32_t done;    // the call ended (stop reason 3 or 4): every later launch of a round returns at once
    int32_t arrived; // workgroups of the running launch that have stored their tile; re-armed by the last one
    int32_t n_assoc[2]; // associated terms per camera of the last association
    int32_t inliers, pad;
};

// one image's edge grid inside the workspace
struct EdgeGrid
{
    const ebvo_edge *E;
    int32_t *cell_of, *cnt, *fill, *start, *list;
    int n;
};

// what the association leaves per camera
struct AssocPlanes
{
    int32_t *idx;             // [n_kf] edge index or -1
    double *ex, *ey, *n0, *n1; // [n_kf] each
};

struct AlignPose
{
    double Rt[12];
};

// the start pose travels as a kernel argument: nothing of the caller's memory is read after the call has returned
__global__ __launch_bounds__(64) void align_init_kernel(AlignState *__restrict__ st, AlignPose P)
{
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    for (int i = 0; i < 12; ++i)
        st->Rt[i] = st->Pv[i] = P.Rt[i];
    st->c_first = st->c_last = st->c_prev = 0.0;
    st->status = 0;
    st->stop = 4;
    st->rounds_run = st->steps = st->fit_terms = st->go = st->done = st->arrived = 0;
    st->n_assoc[0] = st->n_assoc[1] = 0;
    st->inliers = st->pad = 0;
}

__global__ __launch_bounds__(256) void align_prepare_kernel(FinalCalib C, const ebvo_edge *__restrict__ kfL,
                                                            const ebvo_edge *__restrict__ kfR, int n, double *__restrict__ GT)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    {
        double G[3], T[3], g1[3], g2[3];
        stereo_gamma_tangent(C, kfL[i], kfR[i], G, T, g1, g2);
#pragma unroll
        for (int k = 0; k < 3; ++k)
        {
            GT[(size_t)k * n + i] = G[k];
            GT[(size_t)(3 + k) * n + i] = T[k];
        }
    }
}

__global__ __launch_bounds__(256) void align_cells_kernel(const ebvo_edge *__restrict__ E, int n, int cell, int gw, int gh,
                                                          int32_t *__restrict__ cell_of, int32_t *__restrict__ cnt)
{
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
    {
        const int cx = grid_cell(E[j].x, cell, gw), cy = grid_cell(E[j].y, cell, gh);
        const int c = (cx >= 0 && cy >= 0) ? cy * gw + cx : -1;
        cell_of[j] = c;
        if (c >= 0)
            atomicAdd(&cnt[c], 1);
    }
}

// exclusive scan of the cell populations (one block) -> start[0 .. n_cells]
__global__ __launch_bounds__(256) void align_cell_scan_kernel(const int32_t *__restrict__ cnt, int n_cells, int32_t *__restrict__ start)
{
    __shared__ int32_t part[256];
    const int per = (n_cells + 255) / 256;
    const int beg = min(n_cells, (int)threadIdx.x * per), end = min(n_cells, beg + per);
    int32_t sum = 0;
    for (int c = beg; c < end; ++c)
        sum += cnt[c];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0)
    {
        int32_t run = 0;
        for (int t = 0; t < 256; ++t)
        {
            const int32_t v = part[t];
            part[t] = run;
            run += v;
        }
        start[n_cells] = run;
    }
    __syncthreads();
    int32_t run = part[threadIdx.x];
    for (int c = beg; c < end; ++c)
    {
        start[c] = run;
        run += cnt[c];
    }
}

// edges into their cell's segment, in arrival order (the association does not depend on it)
__global__ __launch_bounds__(256) void align_cell_scatter_kernel(const int32_t *__restrict__ cell_of, int n,
                                                                 const int32_t *__restrict__ start, int32_t *__restrict__ fill,
                                                                 int32_t *__restrict__ list)
{
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x)
    {
        const int c = cell_of[j];
        if (c >= 0)
            list[start[c] + atomicAdd(&fill[c], 1)] = j;
    }
}

// Sixteen lanes per item; item = camera * n_kf + mate.  The pose is read from the state.  A launch of a round (round >= 0)
// returns at once when the call has ended; the last association (round < 0) always runs.  cnt: st->n_assoc, zeroed by the
// consumer of the association before this launch (align_init / the last workgroup of the launch that read it).
__global__ __launch_bounds__(256) void align_associate_kernel(AlignArgs A, AlignState *__restrict__ st, int round,
                                                              const double *__restrict__ GT, EdgeGrid g0, EdgeGrid g1,
                                                              AssocPlanes P0, AssocPlanes P1)
{
    if (round >= 0 && st->done)
        return;
    const int n = A.n_kf, items = n * A.cameras;
    const int e = threadIdx.x & 15;
    const int groups = (gridDim.x * blockDim.x) >> 4;
    double Rt[12], M[9];
#pragma unroll
    for (int i = 0; i < 12; ++i)
        Rt[i] = st->Rt[i];
    mm3(A.R21, Rt, M); // R21 R
    // every lane of a wave runs the same number of passes: the 16-lane reduce below needs its four groups converged
    for (int base = 0; base < items; base += groups)
    {
        const int it = base + ((blockIdx.x * blockDim.x + threadIdx.x) >> 4);
        const bool have = it < items;
        const int cam = have && it >= n ? 1 : 0, i = have ? it - cam * n : 0;
        const EdgeGrid &g = cam ? g1 : g0;
        double best_d2 = INFINITY;
        int best_j = 0x7fffffff;
        if (have && g.n > 0)
        {
            const double G[3] = {GT[i], GT[(size_t)n + i], GT[2 * (size_t)n + i]};
            const double T1[3] = {GT[3 * (size_t)n + i], GT[4 * (size_t)n + i], GT[5 * (size_t)n + i]};
            double RG[3], Y[3], q[3], T2[3];
            pose_point(Rt, Rt + 9, G, RG, Y);
            if (cam)
            {
                const double X[3] = {Y[0], Y[1], Y[2]};
                stereo_point(A.R21, A.T21, X, Y);
            }
            project3(cam ? A.Kr : A.Kl, Y, q);
            mv3(cam ? M : Rt, T1, T2);
            const double o = mapped_orientation(T2, q, cam ? A.Kri : A.Kli);
            if (live_projection(q[0], q[1], Y[2], A.margin, A.x_max, A.y_max))
            {
                // inside the margin the casts are defined and the cell is inside the grid
                const int qx = min((int)q[0] / A.cell, A.gw - 1), qy = min((int)q[1] / A.cell, A.gh - 1);
                const int y0 = max(qy - A.sr, 0), y1 = min(qy + A.sr, A.gh - 1);
                const int x0 = max(qx - A.sr, 0), x1 = min(qx + A.sr, A.gw - 1);
                for (int cy = y0; cy <= y1; ++cy)
                    for (int cx = x0; cx <= x1; ++cx)
                    {
                        const int a = g.start[cy * A.gw + cx], b = g.start[cy * A.gw + cx + 1];
                        for (int k = a + e; k < b; k += 16)
                        {
                            const int j = g.list[k];
                            const ebvo_edge ed = g.E[j];
                            const double dx = ed.x - q[0], dy = ed.y - q[1];
                            const double d2 = dx * dx + dy * dy;
                            if (d2 <= A.r2 && orient_close(o, ed.theta, A.orient_thr) && (d2 < best_d2 || (d2 == best_d2 && j < best_j)))
                            {
                                best_d2 = d2;
                                best_j = j;
                            }
                        }
                    }
            }
        }
#pragma unroll
        for (int s = 8; s >= 1; s >>= 1) // the smallest (d2, j) of the sixteen lanes, in every one of them
        {
            const double od = __shfl_xor(best_d2, s);
            const int oj = __shfl_xor(best_j, s);
            if (od < best_d2 || (od == best_d2 && oj < best_j))
            {
                best_d2 = od;
                best_j = oj;
            }
        }
        if (have && e == 0)
        {
            const AssocPlanes &P = cam ? P1 : P0;
            const bool got = best_j != 0x7fffffff;
            double ex = 0.0, ey = 0.0, sn = 0.0, cs = 0.0;
            if (got)
            {
                const ebvo_edge ed = g.E[best_j];
                ex = ed.x;
                ey = ed.y;
                ebvo_sincos(ed.theta, &sn, &cs);
                atomicAdd(&st->n_assoc[cam], 1);
            }
            P.idx[i] = got ? best_j : -1;
            P.ex[i] = ex;
            P.ey[i] = ey;
            P.n0[i] = sn;
            P.n1[i] = -cs;
        }
    }
}

// one camera's normal residual, weight, cost and Jacobian row; valid: associated and rho < +inf
struct AlignCam
{
    double J[6], r, w, cost;
    bool valid;
};

__device__ static inline void align_camera(const double *K, const double *Y, const double *RG, const double *Rs, bool assoc, double ex,
                                           double ey, double n0, double n1, double delta, AlignCam &o)
{
    double pix, piy, jx[3], jy[3];
    const double pz = camera_pixel(K, Y, pix, piy);
    o.r = n0 * (pix - ex) + n1 * (piy - ey);
    const double rho = fabs(o.r);
    o.valid = assoc && rho < INFINITY;
    o.w = huber_weight(rho, delta);
    o.cost = huber_cost(rho, delta);
    camera_rows(K, Rs, pz, pix, piy, jx, jy);
    double Jx[3], Jy[3];
    cross3(RG, jx, Jx); // m . -[R Gamma]x = R Gamma x m
    cross3(RG, jy, Jy);
#pragma unroll
    for (int j = 0; j < 3; ++j)
    {
        o.J[j] = n0 * Jx[j] + n1 * Jy[j];
        o.J[3 + j] = n0 * jx[j] + n1 * jy[j];
    }
}

// both cameras of mate i under the pose
__device__ static inline void align_mate(const AlignArgs &A, const double *Rt, const double *__restrict__ GT, int i,
                                         const AssocPlanes &P0, const AssocPlanes &P1, AlignCam &L, AlignCam &R)
{
    const size_t n = (size_t)A.n_kf;
    const double G[3] = {GT[i], GT[n + i], GT[2 * n + i]};
    double RG[3], X[3], Y[3];
    pose_point(Rt, Rt + 9, G, RG, X);
    stereo_point(A.R21, A.T21, X, Y);
    align_camera(A.Kl, X, RG, nullptr, P0.idx[i] >= 0, P0.ex[i], P0.ey[i], P0.n0[i], P0.n1[i], A.huber, L);
    if (A.cameras > 1)
        align_camera(A.Kr, Y, RG, A.R21, P1.idx[i] >= 0, P1.ex[i], P1.ey[i], P1.n0[i], P1.n1[i], A.huber, R);
    else
    {
        R.valid = false;
        R.r = R.w = R.cost = 0.0;
#pragma unroll
        for (int k = 0; k < 6; ++k)
            R.J[k] = 0.0;
    }
}

// The tile is stored; true in every thread of the workgroup that arrived last (which re-arms the counter).  The classic
// fence-and-count: every writer fences its stores, the barrier orders them before thread 0's atomic.
__device__ static inline bool align_last_workgroup(AlignState *st, int tiles, int *flag)
{
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0)
    {
        const int old = atomicAdd(&st->arrived, 1);
        *flag = old == tiles - 1;
        if (*flag)
            st->arrived = 0;
    }
    __syncthreads();
    const bool last = *flag != 0;
    if (last)
        __threadfence(); // the other workgroups' tiles are visible from here on
    return last;
}

// what follows the 28 sums of step `it` of round `rnd`: the round's first step consumes the association's counts, then the
// shared decision (ebvo_gn6.h); stop reasons 3 and 4 end the call
__device__ static inline void align_decide(const AlignArgs &A, int rnd, int it, const double *sums, AlignState &st)
{
    if (it == 0)
    {
        ++st.rounds_run;
        st.fit_terms = st.n_assoc[0] + st.n_assoc[1];
        st.n_assoc[0] = st.n_assoc[1] = 0; // consumed: the next association counts from zero
        if (st.fit_terms < A.min_terms)
        {
            st.go = 0;
            st.stop = 4;
            st.done = 1;
            if (rnd == 0)
                st.status = 1;
            return;
        }
    }
    if (gn6_decide(rnd, it, A.iterations, A.eps, sums, st) == 3)
        st.done = 1;
}

// Step `it` of round `rnd`: workgroup t forms the 28 sums of tile t.  A block of 256 or 512 threads owns lanes v, v + blockDim,
// ...: a wave always reduces 64 consecutive lanes.
__global__ __launch_bounds__(AL_TILE) void align_sums_kernel(AlignArgs A, AlignState *__restrict__ st, int rnd, int it,
                                                             const double *__restrict__ GT, AssocPlanes P0, AssocPlanes P1,
                                                             double *__restrict__ tile_sums)
{
    __shared__ double part[AL_GROUPS * AL_SUMS];
    __shared__ double sums[AL_SUMS];
    __shared__ AlignState ls;
    __shared__ int flag;
    // the state is written by the LAST workgroup of a launch only, so every workgroup of this one reads the same values
    if (st->done || (it > 0 && !st->go))
        return;
    const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, tile = blockIdx.x;
    double Rt[12];
#pragma unroll
    for (int i = 0; i < 12; ++i)
        Rt[i] = st->Rt[i];
    for (int v = tid; v < AL_TILE; v += T)
    {
        const int i = tile * AL_TILE + v;
        double term[AL_SUMS];
#pragma unroll
        for (int s = 0; s < AL_SUMS; ++s)
            term[s] = 0.0;
        if (i < A.n_kf)
        {
            AlignCam L, R;
            align_mate(A, Rt, GT, i, P0, P1, L, R);
            int s = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b, ++s)
                {
                    const double l = L.w * (L.J[a] * L.J[b]), r = R.w * (R.J[a] * R.J[b]);
                    term[s] = 0.0 + ((L.valid ? l : 0.0) + (R.valid ? r : 0.0));
                }
#pragma unroll
            for (int a = 0; a < 6; ++a)
            {
                const double l = L.w * (L.J[a] * L.r), r = R.w * (R.J[a] * R.r);
                term[21 + a] = 0.0 + ((L.valid ? l : 0.0) + (R.valid ? r : 0.0));
            }
            term[27] = 0.0 + ((L.valid ? L.cost : 0.0) + (R.valid ? R.cost : 0.0));
        }
#pragma unroll
        for (int s = 0; s < AL_SUMS; ++s)
            wave_sum(term[s], lane, &part[(v >> 6) * AL_SUMS + s]);
    }
    __syncthreads();
    if (tid < AL_SUMS)
        tile_sums[(size_t)tile * AL_SUMS + tid] = group_sum<AL_GROUPS>(part, AL_SUMS, tid);
    if (!align_last_workgroup(st, A.tiles, &flag))
        return;
    if (tid < AL_SUMS)
    {
        const volatile double *ts = tile_sums;
        double x = 0.0;
        for (int t = 0; t < A.tiles; ++t) // ascending tile index from +0.0
            x = x + ts[(size_t)t * AL_SUMS + tid];
        sums[tid] = x;
    }
    __syncthreads();
    if (tid == 0)
    {
        ls = *st;
        align_decide(A, rnd, it, sums, ls);
        *st = ls;
    }
}

// After the last association: per tile the sum of r r, and the counts.  The last workgroup writes the result record.
__global__ __launch_bounds__(AL_TILE) void align_metric_kernel(AlignArgs A, AlignState *__restrict__ st, const double *__restrict__ GT,
                                                               AssocPlanes P0, AssocPlanes P1, double *__restrict__ tile_sums,
                                                               AlignResult *__restrict__ out)
{
    __shared__ double part[AL_GROUPS];
    __shared__ int flag;
    const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, tile = blockIdx.x;
    double Rt[12];
#pragma unroll
    for (int i = 0; i < 12; ++i)
        Rt[i] = st->Rt[i];
    for (int v = tid; v < AL_TILE; v += T)
    {
        const int i = tile * AL_TILE + v;
        double term = 0.0;
        int inl = 0;
        if (i < A.n_kf)
        {
            AlignCam L, R;
            align_mate(A, Rt, GT, i, P0, P1, L, R);
            term = 0.0 + ((L.valid ? L.r * L.r : 0.0) + (R.valid ? R.r * R.r : 0.0));
            inl = (L.valid && fabs(L.r) < A.inlier ? 1 : 0) + (R.valid && fabs(R.r) < A.inlier ? 1 : 0);
        }
        wave_count(inl, lane, &st->inliers);
        wave_sum(term, lane, &part[v >> 6]);
    }
    __syncthreads();
    if (tid == 0)
        tile_sums[tile] = group_sum<AL_GROUPS>(part, 1, 0);
    if (!align_last_workgroup(st, A.tiles, &flag))
        return;
    if (tid == 0)
    {
        const volatile double *ts = tile_sums;
        const volatile AlignState *vs = st;
        double x = 0.0;
        for (int t = 0; t < A.tiles; ++t)
            x = x + ts[t];
        const int n0 = vs->n_assoc[0], n1 = vs->n_assoc[1], na = n0 + n1;
#pragma unroll
        for (int i = 0; i < 12; ++i)
            out->Rt[i] = vs->Rt[i];
        out->cost_first = vs->c_first;
        out->cost_last = vs->c_last;
        out->rms_normal = na > 0 ? sqrt(x / (double)na) : 0.0;
        out->status = vs->status;
        out->stop = vs->stop;
        out->rounds_run = vs->rounds_run;
        out->steps_kept = vs->steps;
        out->fit_terms = vs->fit_terms;
        out->n_assoc[0] = n0;
        out->n_assoc[1] = n1;
        out->inliers = atomicAdd(&st->inliers, 0);
    }
}

struct AlignLayout
{
    size_t o_state, o_out, o_tiles, o_gt, o_assoc[2], o_grid[2], total;
};

// per camera: idx [n] then four planes of n doubles; per grid: cell_of [ne], cnt, fill [cells each], start [cells + 1], list [ne]
AlignLayout align_layout(int n_kf, int tiles, int n_cells, const int ne[2])
{
    AlignLayout L;
    const size_t n = (size_t)n_kf;
    size_t o = 0;
    L.o_state = o;
    o += round_up64(sizeof(AlignState));
    L.o_out = o;
    o += round_up64(sizeof(AlignResult));
    L.o_tiles = o;
    o += round_up64(sizeof(double) * AL_SUMS * (size_t)tiles);
    L.o_gt = o;
    o += round_up64(sizeof(double) * 6 * n);
    for (int c = 0; c < 2; ++c)
    {
        L.o_assoc[c] = o;
        o += round_up64(sizeof(int32_t) * n) + round_up64(sizeof(double) * 4 * n);
    }
    for (int c = 0; c < 2; ++c)
    {
        L.o_grid[c] = o;
        o += round_up64(sizeof(int32_t) * (2 * (size_t)ne[c] + 3 * (size_t)n_cells + 1));
    }
    L.total = o;
    return L;
}

// the workspace carved and the call's constants filled; nothing is enqueued
struct AlignSetup
{
    AlignArgs A;
    FinalCalib C;
    AlignPose P0;
    AlignState *d_state;
    AlignResult *d_out;
    double *d_tiles, *d_gt;
    AssocPlanes P[2];
    EdgeGrid g[2];
    int ne[2], n_cells, tiles, bt;
    unsigned anb;
};

int align_setup(ebvo_ctx *ctx, Slot &s, int n_kf, const ebvo_edge *d_E0, int n0, const ebvo_edge *d_E1, int n1, int img_w, int img_h,
                const ebvo_stereo_calib *cal, const ebvo_align_params *ap, const double *R0, const double *t0, AlignSetup &S)
{
    const int cams = ap->cameras, cell = ap->cell_size;
    const int gw = (int)(((int64_t)img_w + cell - 1) / cell), gh = (int)(((int64_t)img_h + cell - 1) / cell), n_cells = gw * gh;
    const int tiles = (n_kf + AL_TILE - 1) / AL_TILE;
    const int ne[2] = {n0, cams > 1 ? n1 : 0};
    const AlignLayout L = align_layout(n_kf, tiles, n_cells, ne);
    if (int rc = ebvo_grow(ctx, s, s.align_ws, L.total))
        return rc;
    char *base = (char *)s.align_ws.p;
    S.d_state = (AlignState *)(base + L.o_state);
    S.d_out = (AlignResult *)(base + L.o_out);
    S.d_tiles = (double *)(base + L.o_tiles);
    S.d_gt = (double *)(base + L.o_gt);
    S.n_cells = n_cells;
    S.tiles = tiles;
    const size_t n = (size_t)n_kf;
    AssocPlanes *P = S.P;
    EdgeGrid *g = S.g;
    for (int c = 0; c < 2; ++c)
    {
        S.ne[c] = ne[c];
        char *a = base + L.o_assoc[c];
        P[c].idx = (int32_t *)a;
        P[c].ex = (double *)(a + round_up64(sizeof(int32_t) * n));
        P[c].ey = P[c].ex + n;
        P[c].n0 = P[c].ey + n;
        P[c].n1 = P[c].n0 + n;
        int32_t *q = (int32_t *)(base + L.o_grid[c]);
        g[c].E = c ? d_E1 : d_E0;
        g[c].n = ne[c];
        g[c].cell_of = q;
        g[c].cnt = q + ne[c];
        g[c].fill = g[c].cnt + n_cells;
        g[c].start = g[c].fill + n_cells;
        g[c].list = g[c].start + n_cells + 1;
    }
    AlignArgs &A = S.A;
    const FinalCalib C = S.C = final_calib_host(cal->K_left, cal->K_right, cal->R21, cal->T21); // the TRUE K_right, as the prior's projection
    memcpy(A.Kl, cal->K_left, sizeof A.Kl);
    memcpy(A.Kr, cal->K_right, sizeof A.Kr);
    memcpy(A.Kli, C.Kli, sizeof A.Kli);
    memcpy(A.Kri, C.Kri, sizeof A.Kri);
    memcpy(A.R21, cal->R21, sizeof A.R21);
    memcpy(A.T21, cal->T21, sizeof A.T21);
    A.margin = ap->img_margin;
    A.x_max = (double)img_w - ap->img_margin;
    A.y_max = (double)img_h - ap->img_margin;
    A.r2 = ap->radius * ap->radius;
    A.orient_thr = ap->orient_thr_deg;
    A.huber = ap->huber_px;
    A.inlier = ap->inlier_px;
    A.eps = ap->step_eps;
    A.n_kf = n_kf;
    A.cameras = cams;
    A.iterations = ap->iterations;
    A.min_terms = ap->min_terms;
    A.cell = cell;
    A.sr = (int)ceil(ap->radius / cell);
    A.gw = gw;
    A.gh = gh;
    A.tiles = tiles;
    memcpy(S.P0.Rt, R0, sizeof(double) * 9);
    memcpy(S.P0.Rt + 9, t0, sizeof(double) * 3);
    S.bt = ap->block_threads ? ap->block_threads : AL_TILE;
    const int64_t ab = ((int64_t)n_kf * cams + 15) / 16; // 16 items per block of 256 threads
    S.anb = chain_grid_cap(s, (unsigned)(ab > 8192 ? 8192 : ab));
    return EBVO_OK;
}

// what precedes the first association: the state, Gamma and T1 (over d_lambda for the live mates when the keyframe's refined
// depths are in use: one more launch, depth_kernels.hip), the two edge grids
int align_enqueue_front(ebvo_ctx *ctx, Slot &s, const AlignSetup &S, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, const double *d_lambda)
{
    hipStream_t st = s.stream;
    const int n_kf = S.A.n_kf, n_cells = S.n_cells;
    hipLaunchKernelGGL(align_init_kernel, dim3(1), dim3(64), 0, st, S.d_state, S.P0);
    const int64_t pb = ((int64_t)n_kf + 255) / 256;
    hipLaunchKernelGGL(align_prepare_kernel, dim3(chain_grid_cap(s, (unsigned)(pb > 2048 ? 2048 : pb))), dim3(256), 0, st, S.C, d_kfL, d_kfR,
                       n_kf, S.d_gt);
    if (d_lambda)
        depth_scale_enqueue(s, S.d_gt, n_kf, d_lambda);
    for (int c = 0; c < S.A.cameras; ++c)
    {
        const EdgeGrid &g = S.g[c];
        if (S.ne[c] <= 0)
        {
            // a camera without edges still has an (all-zero) start array
            EBVO_HIP(ctx, hipMemsetAsync(g.cnt, 0, sizeof(int32_t) * (3 * (size_t)n_cells + 1), st));
            continue;
        }
        const int32_t *start, *list; // = g.start, g.list: the grid's arrays are carved in align_grid_enqueue's order
        if (int rc = align_grid_enqueue(ctx, s, g.E, S.ne[c], S.A.cell, S.A.gw, S.A.gh, g.cell_of, &start, &list))
            return rc;
    }
    return EBVO_OK;
}
} // namespace

void align_prepare_enqueue(const Slot &s, const ebvo_stereo_calib *cal, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, int n_kf, double *d_gt)
{
    const FinalCalib C = final_calib_host(cal->K_left, cal->K_right, cal->R21, cal->T21);
    const int64_t pb = ((int64_t)n_kf + 255) / 256;
    hipLaunchKernelGGL(align_prepare_kernel, dim3(chain_grid_cap(s, (unsigned)(pb > 2048 ? 2048 : pb))), dim3(256), 0, s.stream, C, d_kfL, d_kfR,
                       n_kf, d_gt);
}

// The three grid kernels over any edge list: the alignment's own two, and carry_kernels.hip's list of projected old mates.
// cnt and fill are zeroed, and start too.
int align_grid_enqueue(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_E, int n, int cell, int gw, int gh, int32_t *ws, const int32_t **start,
                       const int32_t **list)
{
    const int n_cells = gw * gh;
    int32_t *cell_of = ws, *cnt = cell_of + n, *fill = cnt + n_cells, *st_ = fill + n_cells, *lst = st_ + n_cells + 1;
    EBVO_HIP(ctx, hipMemsetAsync(cnt, 0, sizeof(int32_t) * (3 * (size_t)n_cells + 1), s.stream));
    const int64_t eb = ((int64_t)n + 255) / 256;
    const unsigned nb = chain_grid_cap(s, (unsigned)(eb > 2048 ? 2048 : eb));
    hipLaunchKernelGGL(align_cells_kernel, dim3(nb), dim3(256), 0, s.stream, d_E, n, cell, gw, gh, cell_of, cnt);
    hipLaunchKernelGGL(align_cell_scan_kernel, dim3(1), dim3(256), 0, s.stream, cnt, n_cells, st_);
    hipLaunchKernelGGL(align_cell_scatter_kernel, dim3(nb), dim3(256), 0, s.stream, cell_of, n, st_, fill, lst);
    *start = st_;
    *list = lst;
    return EBVO_OK;
}

// One association under (R, t), enqueued and not waited for: the edge index (or -1) per mate and camera stays in the workspace.
int align_associate_once(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, int n_kf, const ebvo_edge *d_E0, int n0,
                         const ebvo_edge *d_E1, int n1, int img_w, int img_h, const ebvo_stereo_calib *cal, const ebvo_align_params *ap,
                         const double *R, const double *t, const double *d_lambda, const int32_t **idx0, const int32_t **idx1)
{
    AlignSetup S;
    if (int rc = align_setup(ctx, s, n_kf, d_E0, n0, d_E1, n1, img_w, img_h, cal, ap, R, t, S))
        return rc;
    {
        ProfScope ps(ctx, s, K_MISC);
        if (int rc = align_enqueue_front(ctx, s, S, d_kfL, d_kfR, d_lambda))
            return rc;
        hipLaunchKernelGGL(align_associate_kernel, dim3(S.anb), dim3(256), 0, s.stream, S.A, S.d_state, -1, S.d_gt, S.g[0], S.g[1], S.P[0], S.P[1]);
    }
    EBVO_HIP(ctx, hipGetLastError());
    *idx0 = S.P[0].idx;
    *idx1 = ap->cameras > 1 ? S.P[1].idx : nullptr;
    return EBVO_OK;
}

// Every launch of the call is enqueued here, then the result record and the association arrays are copied back and waited
// for.  d_E1 / n1 are not read with cameras = 1.  d_lambda (may be NULL): the keyframe's inverse-depth ratios.
int align_run(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, int n_kf, const ebvo_edge *d_E0, int n0,
              const ebvo_edge *d_E1, int n1, int img_w, int img_h, const ebvo_stereo_calib *cal, const ebvo_align_params *ap,
              const double *R0, const double *t0, const double *d_lambda, AlignResult *res, int32_t *assoc_left, int32_t *assoc_right)
{
    AlignSetup S;
    if (int rc = align_setup(ctx, s, n_kf, d_E0, n0, d_E1, n1, img_w, img_h, cal, ap, R0, t0, S))
        return rc;
    const AlignArgs &A = S.A;
    const AssocPlanes *P = S.P;
    const EdgeGrid *g = S.g;
    AlignState *d_state = S.d_state;
    double *d_tiles = S.d_tiles, *d_gt = S.d_gt;
    AlignResult *d_out = S.d_out;
    const int cams = ap->cameras, tiles = S.tiles, bt = S.bt;
    const unsigned anb = S.anb;
    const size_t n = (size_t)n_kf;
    hipStream_t st = s.stream;
    {
        ProfScope ps(ctx, s, K_MISC);
        if (int rc = align_enqueue_front(ctx, s, S, d_kfL, d_kfR, d_lambda))
            return rc;
        for (int rnd = 0; rnd < ap->rounds; ++rnd)
        {
            hipLaunchKernelGGL(align_associate_kernel, dim3(anb), dim3(256), 0, st, A, d_state, rnd, d_gt, g[0], g[1], P[0], P[1]);
            for (int it = 0; it <= ap->iterations; ++it)
                hipLaunchKernelGGL(align_sums_kernel, dim3(tiles), dim3(bt), 0, st, A, d_state, rnd, it, d_gt, P[0], P[1], d_tiles);
        }
        // every association of a round was consumed by its first align_sums launch (or never ran): the counters are zero
        hipLaunchKernelGGL(align_associate_kernel, dim3(anb), dim3(256), 0, st, A, d_state, -1, d_gt, g[0], g[1], P[0], P[1]);
        hipLaunchKernelGGL(align_metric_kernel, dim3(tiles), dim3(bt), 0, st, A, d_state, d_gt, P[0], P[1], d_tiles, d_out);
    }
    EBVO_HIP(ctx, hipGetLastError());
    EBVO_HIP(ctx, hipMemcpyAsync(res, d_out, sizeof *res, hipMemcpyDeviceToHost, st));
    if (assoc_left)
        EBVO_HIP(ctx, hipMemcpyAsync(assoc_left, P[0].idx, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    if (assoc_right && cams > 1)
        EBVO_HIP(ctx, hipMemcpyAsync(assoc_right, P[1].idx, sizeof(int32_t) * n, hipMemcpyDeviceToHost, st));
    EBVO_HIP(ctx, hipStreamSynchronize(st));
    if (assoc_right && cams == 1)
        for (size_t i = 0; i < n; ++i)
            assoc_right[i] = -1;
    return EBVO_OK;
}
