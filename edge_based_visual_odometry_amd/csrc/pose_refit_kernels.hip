// Inlier refit of the relative pose: Gauss-Newton on the reprojection error of both cameras over the inliers of a start pose.
// The arithmetic contract is written once in include/ebvo_hip.h (ebvo_pose_refine_from_quads); tests/oracle_pose_refit.py
// restates it on the CPU and the device matches it bit for bit.
//   pose_refit_prepare_kernel   one thread per quad: Gamma of its keyframe mate (as pose_prepare_kernel forms it) and the CF
//                               left / right centres, seven planes of n
//   pose_refit_kernel           ONE workgroup runs every round and step: fit set, 28 sums over 1024 virtual lanes (a lane's
//                               quads in ascending order, a 64-lane halving tree per value, the 16 group sums through LDS and
//                               the same tree), the 6 x 6 Cholesky and Exp by one lane with the pose and the loop's state in
//                               LDS, then the final mask and count.  No spin-wait, no grid-wide barrier, no host read between steps; every loop is bounded by
//                               rounds x (iterations + 1) x ceil(n / 1024).
// A block of 256 or 512 threads owns virtual lanes v, v + blockDim, ...: one pass per owned lane, so a wave always reduces 64
// consecutive virtual lanes and the sums do not depend on the launch geometry.
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
constexpr int RF_LANES = 1024; // virtual lanes
constexpr int RF_GROUPS = RF_LANES / 64;
constexpr int RF_SUMS = 28;    // 21 upper entries of H (row-major, i <= j), 6 of g, the cost
constexpr int RF_PLANES = 7;   // Gamma x, y, z, CF left x, y, CF right x, y

struct RefitArgs
{
    double K[9], R21[9], T21[3], Rt[12]; // Rt: the start pose, R row-major then t
    double thr, huber, eps;
    int32_t rounds, iterations, n;
};

__global__ void pose_refit_prepare_kernel(FinalCalib C, const ebvo_edge *__restrict__ kfL, const ebvo_edge *__restrict__ kfR,
                                          const int32_t *__restrict__ rp, int n_kf, const ebvo_edge *__restrict__ cfL,
                                          const ebvo_edge *__restrict__ cfR, int n, double *__restrict__ pts)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x)
    {
        const int lo = quad_row(rp, n_kf, k);
        double G[3], T[3], g1[3], g2[3];
        stereo_gamma_tangent(C, kfL[lo], kfR[lo], G, T, g1, g2);
        const ebvo_edge cl = cfL[k], cr = cfR[k];
        pts[k] = G[0];
        pts[(size_t)n + k] = G[1];
        pts[2 * (size_t)n + k] = G[2];
        pts[3 * (size_t)n + k] = cl.x;
        pts[4 * (size_t)n + k] = cl.y;
        pts[5 * (size_t)n + k] = cr.x;
        pts[6 * (size_t)n + k] = cr.y;
    }
}

// one camera's residual, weight, cost and Jacobian rows (J = Jpi A [-[R Gamma]x | I]; Rs = A: NULL for the identity)
struct RefitCam
{
    double Jx[6], Jy[6], rx, ry, w, cost;
    bool valid;
};

__device__ static inline void refit_camera(const double *K, const double *Y, const double *RG, const double *Rs, double cx, double cy,
                                           double delta, RefitCam &o)
{
    double pix, piy, jx[3], jy[3];
    const double pz = camera_pixel(K, Y, pix, piy);
    o.rx = pix - cx;
    o.ry = piy - cy;
    const double rho = sqrt(o.rx * o.rx + o.ry * o.ry);
    o.valid = rho < INFINITY;
    o.w = huber_weight(rho, delta);
    o.cost = huber_cost(rho, delta);
    camera_rows(K, Rs, pz, pix, piy, jx, jy);
    cross3(RG, jx, o.Jx); // m . -[R Gamma]x = R Gamma x m
    cross3(RG, jy, o.Jy);
#pragma unroll
    for (int j = 0; j < 3; ++j)
    {
        o.Jx[3 + j] = jx[j];
        o.Jy[3 + j] = jy[j];
    }
}

// acc[i] = acc[i] + (left term + right term), an invalid camera's terms +0.0
__device__ static inline void refit_accumulate(const RefitArgs &A, const double *Rt, const double *G, double ux, double uy, double bx,
                                               double by, double *acc)
{
    double RG[3], X[3], Y[3];
    pose_point(Rt, Rt + 9, G, RG, X);
    stereo_point(A.R21, A.T21, X, Y);
    RefitCam L, R;
    refit_camera(A.K, X, RG, nullptr, ux, uy, A.huber, L);
    refit_camera(A.K, Y, RG, A.R21, bx, by, A.huber, R);
    int s = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j, ++s)
        {
            const double l = L.w * (L.Jx[i] * L.Jx[j] + L.Jy[i] * L.Jy[j]), r = R.w * (R.Jx[i] * R.Jx[j] + R.Jy[i] * R.Jy[j]);
            acc[s] = acc[s] + ((L.valid ? l : 0.0) + (R.valid ? r : 0.0));
        }
#pragma unroll
    for (int i = 0; i < 6; ++i)
    {
        const double l = L.w * (L.Jx[i] * L.rx + L.Jy[i] * L.ry), r = R.w * (R.Jx[i] * R.rx + R.Jy[i] * R.ry);
        acc[21 + i] = acc[21 + i] + ((L.valid ? l : 0.0) + (R.valid ? r : 0.0));
    }
    acc[27] = acc[27] + ((L.valid ? L.cost : 0.0) + (R.valid ? R.cost : 0.0));
}

// pose_inlier over every selected quad: dst[map ? map[k] : k] and the count (the same in every thread)
__device__ static inline int refit_select(const RefitArgs &A, const double *Rt, const double *__restrict__ pts,
                                          const int32_t *__restrict__ map, uint8_t *__restrict__ dst, int *cnt)
{
    const int T = blockDim.x, n = A.n, chunks = (n + RF_LANES - 1) / RF_LANES;
    if (threadIdx.x == 0)
        *cnt = 0;
    __syncthreads();
    for (int v = threadIdx.x; v < RF_LANES; v += T)
        for (int c = 0; c < chunks; ++c)
        {
            const int k = v + c * RF_LANES;
            const bool have = k < n;
            bool in = false;
            if (have)
            {
                const double G[3] = {pts[k], pts[(size_t)n + k], pts[2 * (size_t)n + k]};
                in = pose_inlier(Rt, A.K, G, pts[3 * (size_t)n + k], pts[4 * (size_t)n + k], A.thr);
                dst[map ? map[k] : k] = in ? 1 : 0;
            }
            const unsigned long long m = __ballot(in);
            if ((threadIdx.x & 63) == 0 && m)
                atomicAdd(cnt, (int)__popcll(m));
        }
    __syncthreads();
    const int r = *cnt;
    __syncthreads();
    return r;
}

// The pose and the loop's state live in LDS: thread 0 runs the decisions, the solve and Exp between two barriers, every lane
// reads the pose back per quad.  (Kept in registers of every lane they cost 48 VGPRs next to the 56 of the accumulators.)
struct RefitState
{
    double Rt[12], Pv[12]; // the pose, and the one before the last step
    double c_first, c_last, c_prev;
    int32_t status, stop, rounds_run, steps, fitn, go;
};

// fit: n bytes of scratch (the fit set of the round); mask: the inliers of the returned pose, at map[k] (or k)
__global__ __launch_bounds__(RF_LANES) void pose_refit_kernel(RefitArgs A, const double *__restrict__ pts, const int32_t *__restrict__ map,
                                                              uint8_t *__restrict__ fit, uint8_t *__restrict__ mask,
                                                              PoseRefitOut *__restrict__ out)
{
    __shared__ double part[RF_GROUPS * RF_SUMS];
    __shared__ double sums[RF_SUMS];
    __shared__ RefitState st;
    __shared__ int cnt;
    const int T = blockDim.x, tid = threadIdx.x, lane = tid & 63, n = A.n, chunks = (n + RF_LANES - 1) / RF_LANES;
    if (tid == 0)
    {
#pragma unroll
        for (int i = 0; i < 12; ++i)
            st.Rt[i] = st.Pv[i] = A.Rt[i];
        st.c_first = st.c_last = st.c_prev = 0.0;
        st.status = 0;
        st.stop = 4;
        st.rounds_run = st.steps = st.fitn = st.go = 0;
    }
    __syncthreads();
    const volatile double *pose = st.Rt; // read anew for every quad: the pose is not kept in registers across the loops
    for (int rnd = 0; rnd < A.rounds; ++rnd)
    {
        const int fitn = refit_select(A, st.Rt, pts, nullptr, fit, &cnt);
        if (tid == 0)
        {
            ++st.rounds_run;
            st.fitn = fitn;
        }
        if (fitn < 3)
        {
            if (tid == 0)
            {
                st.stop = 4;
                if (rnd == 0)
                    st.status = 1;
            }
            break;
        }
        for (int it = 0; it <= A.iterations; ++it)
        {
            for (int v = tid; v < RF_LANES; v += T) // the virtual lanes this thread owns: a wave holds 64 consecutive ones
            {
                double acc[RF_SUMS];
#pragma unroll
                for (int i = 0; i < RF_SUMS; ++i)
                    acc[i] = 0.0;
                for (int c = 0; c < chunks; ++c)
                {
                    const int k = v + c * RF_LANES;
                    if (k < n && fit[k])
                    {
                        double Rt[12];
#pragma unroll
                        for (int i = 0; i < 12; ++i)
                            Rt[i] = pose[i];
                        const double G[3] = {pts[k], pts[(size_t)n + k], pts[2 * (size_t)n + k]};
                        refit_accumulate(A, Rt, G, pts[3 * (size_t)n + k], pts[4 * (size_t)n + k], pts[5 * (size_t)n + k],
                                         pts[6 * (size_t)n + k], acc);
                    }
                }
#pragma unroll
                for (int i = 0; i < RF_SUMS; ++i)
                    wave_sum(acc[i], lane, &part[(v >> 6) * RF_SUMS + i]);
            }
            __syncthreads();
            if (tid < RF_SUMS)
                sums[tid] = group_sum<RF_GROUPS>(part, RF_SUMS, tid);
            __syncthreads();
            if (tid == 0) // go = 0 ends the round
                gn6_decide(rnd, it, A.iterations, A.eps, sums, st);
            __syncthreads();
            if (!st.go)
                break;
        }
        if (st.status == 2)
            break;
    }
    const int inl = refit_select(A, st.Rt, pts, map, mask, &cnt);
    if (tid == 0)
    {
#pragma unroll
        for (int i = 0; i < 12; ++i)
            out->Rt[i] = st.Rt[i];
        out->cost_first = st.c_first;
        out->cost_last = st.c_last;
        out->status = st.status;
        out->stop = st.stop;
        out->rounds_run = st.rounds_run;
        out->steps_kept = st.steps;
        out->fit = st.fitn;
        out->inliers = inl;
    }
}
} // namespace

int pose_refit_device(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, const int32_t *d_rp, int n_kf,
                      const ebvo_edge *d_cfL, const ebvo_edge *d_cfR, int n, const int32_t *d_map, int n_full,
                      const ebvo_stereo_calib *cal, double thr, const ebvo_pose_refine_params *rp, const double *R0, const double *t0,
                      PoseRefitOut *res, uint8_t *inlier)
{
    const size_t nz = (size_t)n, fz = (size_t)n_full;
    const size_t o_fit = sizeof(double) * RF_PLANES * nz, o_mask = o_fit + round_up64(nz), o_out = o_mask + round_up64(fz);
    if (int rc = ebvo_grow(ctx, s, s.pose_refit, o_out + sizeof(PoseRefitOut)))
        return rc;
    char *base = (char *)s.pose_refit.p;
    double *d_pts = (double *)base;
    uint8_t *d_fit = (uint8_t *)(base + o_fit), *d_mask = (uint8_t *)(base + o_mask);
    PoseRefitOut *d_out = (PoseRefitOut *)(base + o_out);
    hipStream_t st = s.stream;
    // K_right := K_left, as everywhere in the pose stage
    const FinalCalib C = final_calib_host(cal->K_left, cal->K_left, cal->R21, cal->T21);
    RefitArgs A;
    memcpy(A.K, cal->K_left, sizeof A.K);
    memcpy(A.R21, cal->R21, sizeof A.R21);
    memcpy(A.T21, cal->T21, sizeof A.T21);
    memcpy(A.Rt, R0, sizeof(double) * 9);
    memcpy(A.Rt + 9, t0, sizeof(double) * 3);
    A.thr = thr;
    A.huber = rp->huber_px;
    A.eps = rp->step_eps;
    A.rounds = rp->rounds;
    A.iterations = rp->iterations;
    A.n = n;
    if (d_map && inlier)
        EBVO_HIP(ctx, hipMemsetAsync(d_mask, 0, fz, st)); // zero on the quads not selected
    {
        ProfScope ps(ctx, s, K_MISC);
        const int64_t b = ((int64_t)n + 255) / 256;
        hipLaunchKernelGGL(pose_refit_prepare_kernel, dim3((unsigned)(b > 2048 ? 2048 : b)), dim3(256), 0, st, C, d_kfL, d_kfR, d_rp, n_kf,
                           d_cfL, d_cfR, n, d_pts);
        hipLaunchKernelGGL(pose_refit_kernel, dim3(1), dim3(rp->block_threads ? rp->block_threads : RF_LANES), 0, st, A, d_pts, d_map,
                           d_fit, d_mask, d_out);
    }
    EBVO_HIP(ctx, hipGetLastError());
    EBVO_HIP(ctx, hipMemcpyAsync(res, d_out, sizeof *res, hipMemcpyDeviceToHost, st));
    if (inlier)
        EBVO_HIP(ctx, hipMemcpyAsync(inlier, d_mask, fz, hipMemcpyDeviceToHost, st));
    EBVO_HIP(ctx, hipStreamSynchronize(st));
    return EBVO_OK;
}
