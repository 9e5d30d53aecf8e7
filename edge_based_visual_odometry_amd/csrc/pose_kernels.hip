// Relative pose from the temporal quads: MotionTracker::estimate_Relative_Pose_From_Quad_Pairs (src/MotionTracker.cpp:175-253).
//
// The index pairs the loop draws depend on the random stream alone, never on what a draw scores, so the device evaluates a
// BATCH of draws speculatively and the host replays the loop's control flow over the batch, draw by draw:
//   pose_prepare_kernel   one thread per quad: Gamma, Gamma_bar, T, T_bar (get_Gammas_and_Tangents_From_Quads :28-66)
//   pose_rank_kernel      one thread per KF mate: its quads' positions in the rank order (:90-103)
//   (host)                the batch's index pairs from the restated glibc generator, uploaded
//   pose_hyp_kernel       one thread per draw: the four constraints (:108-134) and, if they pass, R and t (:136-153)
//   pose_score_kernel     hypotheses x quads -> integer inlier counts (:155-173): hypothesis tiles in LDS, a quad per lane,
//                         ballot + popcount + integer atomics (order-free sums)
//   (host)                exact sequential replay of the loop over the accept flags and counts; the next batch only if the
//                         loop has not ended (draws past its end are never observed; the generator is rewound to them)
//   pose_mask_kernel      the inlier mask of the best hypothesis
// fp64 throughout, -ffp-contract=off (no FMA), IEEE division and sqrt; every dot / norm / product in the order of
// ebvo_geom.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "ebvo_internal.h"
#include "ebvo_math.h"
#include "ebvo_geom.h"

namespace
{
constexpr int POSE_RANK_TILE = 1024; // KF row lengths per LDS tile of the rank kernel
constexpr int POSE_TILE_H = 64;      // hypotheses per LDS tile of the scoring kernel
constexpr int POSE_BATCH_DEFAULT = 4096;

struct PoseTaus
{
    double len, t1, t2, tan;
};
struct PoseK
{
    double K[9];
};
struct PoseRt
{
    double Rt[12]; // R row-major, then t
};

// geom row of a quad: Gamma 0-2, Gamma_bar 3-5, T 6-8, T_bar 9-11.  pts: five planes of n (Gamma x, y, z, CF left x, y).
__global__ void pose_prepare_kernel(FinalCalib C, const ebvo_edge *__restrict__ kfL, const ebvo_edge *__restrict__ kfR,
                                    const int32_t *__restrict__ rp, int n_kf, const ebvo_edge *__restrict__ cfL,
                                    const ebvo_edge *__restrict__ cfR, int n, double *__restrict__ geom, double *__restrict__ pts)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x)
    {
        const int lo = quad_row(rp, n_kf, k);
        double G[3], Gb[3], T[3], Tb[3], g1[3], g2[3];
        stereo_gamma_tangent(C, kfL[lo], kfR[lo], G, T, g1, g2);
        const ebvo_edge cl = cfL[k];
        stereo_gamma_tangent(C, cl, cfR[k], Gb, Tb, g1, g2);
        double *o = geom + (size_t)k * 12;
#pragma unroll
        for (int i = 0; i < 3; ++i)
        {
            o[i] = G[i];
            o[3 + i] = Gb[i];
            o[6 + i] = T[i];
            o[9 + i] = Tb[i];
        }
        pts[k] = G[0];
        pts[(size_t)n + k] = G[1];
        pts[2 * (size_t)n + k] = G[2];
        pts[3 * (size_t)n + k] = cl.x;
        pts[4 * (size_t)n + k] = cl.y;
    }
}

// The rank order is a strict total order on (row length, KF index, candidate index); the quads of row i start at
// off(i) = sum of len_j over the rows j ordered before it.  One thread per row, the row lengths streamed through LDS.
__global__ __launch_bounds__(256) void pose_rank_kernel(const int32_t *__restrict__ rp, int n_kf, int32_t *__restrict__ order)
{
    __shared__ int32_t len_s[POSE_RANK_TILE];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int li = i < n_kf ? rp[i + 1] - rp[i] : 0;
    int off = 0;
    for (int base = 0; base < n_kf; base += POSE_RANK_TILE)
    {
        const int m = min(POSE_RANK_TILE, n_kf - base);
        __syncthreads();
        for (int j = threadIdx.x; j < m; j += blockDim.x)
            len_s[j] = rp[base + j + 1] - rp[base + j];
        __syncthreads();
        if (li > 0)
            for (int j = 0; j < m; ++j)
            {
                const int lj = len_s[j];
                off += (lj < li || (lj == li && base + j < i)) ? lj : 0;
            }
    }
    if (li > 0)
    {
        const int r0 = rp[i];
        for (int c = 0; c < li; ++c)
            order[off + c] = r0 + c;
    }
}

// Apply_Normalized_Length / T1 / T2 / Tangent_Angle_Similarity_Constraint (:108-134) in the loop's order: the number of
// constraints the pair passed before its first failure (4 = all of them).  d21 / d21b: Gamma_2 - Gamma_1 and its barred twin,
// which the pose of a passing pair starts from.  One function for the search (pose_hyp_kernel) and for the constraint
// cascade (pose_cascade_kernel): the same operations in the same order.
__device__ static inline int pose_constraints(const double *a, const double *b, const PoseTaus &tau, double *d21, double *d21b)
{
    double d12[3], d12b[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
    {
        d12[i] = a[i] - b[i];
        d12b[i] = a[3 + i] - b[3 + i];
        d21[i] = b[i] - a[i];
        d21b[i] = b[3 + i] - a[3 + i];
    }
    // (a zero length ends in NaN / inf: the comparison is false, the draw is rejected, as in the reference)
    const double lG = sqrt(dot3(d12, d12)), lGb = sqrt(dot3(d12b, d12b));
    if (!(fabs(lG - lGb) / lG < tau.len))
        return 0;
    const double n21 = sqrt(dot3(d21, d21)), n21b = sqrt(dot3(d21b, d21b));
    {
        const double c = dot3(d21, a + 6) / n21, cb = dot3(d21b, a + 9) / n21b;
        if (!(fabs(fabs(c) - fabs(cb)) < tau.t1))
            return 1;
    }
    {
        const double c = dot3(d21, b + 6) / n21, cb = dot3(d21b, b + 9) / n21b;
        if (!(fabs(fabs(c) - fabs(cb)) < tau.t2))
            return 2;
    }
    const double c = dot3(a + 6, b + 6), cb = dot3(a + 9, b + 9);
    return fabs(fabs(c) - fabs(cb)) < tau.tan ? 4 : 3;
}

// the four constraints and, if they pass, estimate_Pose_From_a_Quad_Pair
__global__ void pose_hyp_kernel(const int32_t *__restrict__ draws, int nb, const int32_t *__restrict__ order,
                                const double *__restrict__ geom, PoseTaus tau, uint8_t *__restrict__ ok, double *__restrict__ hyp)
{
    for (int d = blockIdx.x * blockDim.x + threadIdx.x; d < nb; d += gridDim.x * blockDim.x)
    {
        const double *a = geom + (size_t)order[draws[2 * d]] * 12;     // q1
        const double *b = geom + (size_t)order[draws[2 * d + 1]] * 12; // q2
        double d21[3], d21b[3];
        const bool pass = pose_constraints(a, b, tau, d21, d21b) == 4;
        ok[d] = pass ? 1 : 0;
        if (!pass)
            continue;
        double e1[3], e1b[3], u1[3], u1b[3], e3[3], e3b[3];
#pragma unroll
        for (int i = 0; i < 3; ++i)
        {
            e1[i] = d21[i];
            e1b[i] = d21b[i];
        }
        normalize3(e1);
        normalize3(e1b);
        const double s = dot3(e1, a + 6), sb = dot3(e1b, a + 9);
#pragma unroll
        for (int i = 0; i < 3; ++i)
        {
            u1[i] = a[6 + i] - s * e1[i];
            u1b[i] = a[9 + i] - sb * e1b[i];
        }
        normalize3(u1); // e2
        normalize3(u1b);
        cross3(e1, u1, e3);
        cross3(e1b, u1b, e3b);
        double *o = hyp + (size_t)d * 12;
        double R[9];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) // (B_bar B^T)(i, j) = sum_k B_bar(i, k) B(j, k)
                R[i * 3 + j] = (e1b[i] * e1[j] + u1b[i] * u1[j]) + e3b[i] * e3[j];
        double RG[3];
        mv3(R, a, RG);
#pragma unroll
        for (int i = 0; i < 9; ++i)
            o[i] = R[i];
#pragma unroll
        for (int i = 0; i < 3; ++i)
            o[9 + i] = a[3 + i] - RG[i];
    }
}

// pose_inlier (score_Pose_Hypothesis for one quad) is in ebvo_geom.h: the refit (pose_refit_kernels.hip) selects with it too

// grid (quad chunks of 256, hypothesis tiles of POSE_TILE_H); counts[] zeroed before
__global__ __launch_bounds__(256) void pose_score_kernel(const double *__restrict__ hyp, const uint8_t *__restrict__ ok, int nb,
                                                         const double *__restrict__ pts, int n, PoseK K, double thr,
                                                         int32_t *__restrict__ counts)
{
    __shared__ double hs[POSE_TILE_H * 12];
    __shared__ int oks[POSE_TILE_H], cnt[POSE_TILE_H];
    const int h0 = blockIdx.y * POSE_TILE_H;
    const int nh = min(POSE_TILE_H, nb - h0);
    for (int j = threadIdx.x; j < POSE_TILE_H; j += blockDim.x)
    {
        oks[j] = j < nh && ok[h0 + j];
        cnt[j] = 0;
    }
    for (int j = threadIdx.x; j < nh * 12; j += blockDim.x)
        hs[j] = hyp[(size_t)h0 * 12 + j];
    __syncthreads();
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    const bool have = k < n;
    double G[3] = {0.0, 0.0, 0.0}, ux = 0.0, uy = 0.0;
    if (have)
    {
        G[0] = pts[k];
        G[1] = pts[(size_t)n + k];
        G[2] = pts[2 * (size_t)n + k];
        ux = pts[3 * (size_t)n + k];
        uy = pts[4 * (size_t)n + k];
    }
    const int lane = threadIdx.x & (warpSize - 1);
    for (int h = 0; h < nh; ++h)
    {
        if (!oks[h]) // the same for the whole block
            continue;
        const bool in = have && pose_inlier(hs + h * 12, K.K, G, ux, uy, thr);
        const unsigned long long m = __ballot(in);
        if (lane == 0 && m)
            atomicAdd(&cnt[h], (int)__popcll(m));
    }
    __syncthreads();
    for (int j = threadIdx.x; j < nh; j += blockDim.x)
        if (cnt[j])
            atomicAdd(&counts[h0 + j], cnt[j]);
}

__global__ void pose_mask_kernel(PoseRt H, const double *__restrict__ pts, int n, PoseK K, double thr, uint8_t *__restrict__ mask)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x)
    {
        const double G[3] = {pts[k], pts[(size_t)n + k], pts[2 * (size_t)n + k]};
        mask[k] = pose_inlier(H.Rt, K.K, G, pts[3 * (size_t)n + k], pts[4 * (size_t)n + k], thr) ? 1 : 0;
    }
}

// ---- the search and the constraint cascade over ground-truth rows (the has_gt() branch of get_Quad_for_Pose_Solution :68-106)
// The selected rows are COMPACTED on the device and the kernels above run unchanged on the compacted arrays: dropping rows
// does not change the relative order of the rest under (row length, KF index, candidate index).
//   pose_select_scan_kernel     one block: exclusive scans over on[i] (compacted row) and on[i] * len[i] (compacted quad
//                               offset), the compacted row_ptr and the two totals
//   pose_select_gather_kernel   one thread per selected row: its KF mate, its quads, their CSR indices (map) and flags
//   pose_scatter_kernel         mask and geometry back to the CSR order, the rank order as CSR indices, -1 beyond
//   pose_cascade_kernel         Solution_Constraints_Application (:255-381): one thread per draw, grid.y = runs
constexpr int POSE_SCAN_T = 256;
constexpr int POSE_CASC_T = 256;
constexpr int POSE_CASC_COUNTERS = 2 * EBVO_PC_NUM_STAGES; // per run: surviving per stage, then veridical per stage

__global__ __launch_bounds__(POSE_SCAN_T) void pose_select_scan_kernel(const uint8_t *__restrict__ on, const int32_t *__restrict__ rp,
                                                                      int n_kf, int32_t *__restrict__ crow, int32_t *__restrict__ cq,
                                                                      int32_t *__restrict__ crp, int32_t *__restrict__ tot)
{
    __shared__ int32_t sr[POSE_SCAN_T], sq[POSE_SCAN_T];
    const int t = threadIdx.x;
    int32_t rows = 0, quads = 0; // the totals of the tiles before this one (the same in every thread)
    for (int base = 0; base < n_kf; base += POSE_SCAN_T)
    {
        const int i = base + t;
        const bool o = i < n_kf && on[i];
        const int32_t r = o ? 1 : 0, q = o ? rp[i + 1] - rp[i] : 0;
        sr[t] = r;
        sq[t] = q;
        __syncthreads();
        for (int off = 1; off < POSE_SCAN_T; off <<= 1)
        {
            const int32_t ar = t >= off ? sr[t - off] : 0, aq = t >= off ? sq[t - off] : 0;
            __syncthreads();
            sr[t] += ar;
            sq[t] += aq;
            __syncthreads();
        }
        if (i < n_kf)
        {
            crow[i] = rows + sr[t] - r;
            cq[i] = quads + sq[t] - q;
            if (o)
                crp[rows + sr[t] - r] = quads + sq[t] - q;
        }
        rows += sr[POSE_SCAN_T - 1];
        quads += sq[POSE_SCAN_T - 1];
        __syncthreads();
    }
    if (t == 0)
    {
        crp[rows] = quads;
        tot[0] = rows;
        tot[1] = quads;
    }
}

// tp (may be NULL: no quad is veridical): b_is_TP per quad in CSR order; otp (may be NULL): the same per compacted quad
__global__ void pose_select_gather_kernel(const uint8_t *__restrict__ on, const int32_t *__restrict__ rp, int n_kf,
                                          const int32_t *__restrict__ crow, const int32_t *__restrict__ cq,
                                          const ebvo_edge *__restrict__ kfL, const ebvo_edge *__restrict__ kfR,
                                          const ebvo_edge *__restrict__ cfL, const ebvo_edge *__restrict__ cfR,
                                          const uint8_t *__restrict__ tp, ebvo_edge *__restrict__ okfL, ebvo_edge *__restrict__ okfR,
                                          ebvo_edge *__restrict__ ocfL, ebvo_edge *__restrict__ ocfR, int32_t *__restrict__ map,
                                          uint8_t *__restrict__ otp)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n_kf; i += gridDim.x * blockDim.x)
    {
        if (!on[i])
            continue;
        const int r = crow[i], q0 = rp[i], len = rp[i + 1] - q0, o0 = cq[i];
        okfL[r] = kfL[i];
        okfR[r] = kfR[i];
        for (int c = 0; c < len; ++c)
        {
            ocfL[o0 + c] = cfL[q0 + c];
            ocfR[o0 + c] = cfR[q0 + c];
            map[o0 + c] = q0 + c;
            if (otp)
                otp[o0 + c] = tp ? (tp[q0 + c] ? 1 : 0) : 0;
        }
    }
}

// n: selected quads, n_full: all quads.  mask / geom (may be NULL) were zeroed before; order (may be NULL) has n_full entries
__global__ void pose_scatter_kernel(const int32_t *__restrict__ map, int n, int n_full, const uint8_t *__restrict__ cmask,
                                    uint8_t *__restrict__ mask, const double *__restrict__ cgeom, double *__restrict__ geom,
                                    const int32_t *__restrict__ corder, int32_t *__restrict__ order)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n_full; k += gridDim.x * blockDim.x)
    {
        if (k < n)
        {
            const size_t m = (size_t)map[k];
            if (mask)
                mask[m] = cmask[k];
            if (geom)
#pragma unroll
                for (int j = 0; j < 12; ++j)
                    geom[m * 12 + j] = cgeom[(size_t)k * 12 + j];
        }
        if (order)
            order[k] = k < n ? map[corder[k]] : -1;
    }
}

// grid (chunks of a run's draws, runs): no block straddles two runs.  stage[]: bits 0-2 the constraints passed, bit 7 both
// quads veridical.  counters[run][POSE_CASC_COUNTERS] zeroed before: ballot + popcount into LDS, then one integer atomic per
// block and counter (order-free sums, as in pose_score_kernel).
__global__ __launch_bounds__(POSE_CASC_T) void pose_cascade_kernel(const int32_t *__restrict__ draws, int per_run, int n_runs,
                                                                  const int32_t *__restrict__ order, const double *__restrict__ geom,
                                                                  const uint8_t *__restrict__ tp, PoseTaus tau,
                                                                  uint8_t *__restrict__ stage, int32_t *__restrict__ counters)
{
    __shared__ int cnt[POSE_CASC_COUNTERS];
    const int d = blockIdx.x * POSE_CASC_T + threadIdx.x;
    const bool have = d < per_run;
    const int lane = threadIdx.x & (warpSize - 1);
    for (int run = blockIdx.y; run < n_runs; run += gridDim.y)
    {
        if (threadIdx.x < POSE_CASC_COUNTERS)
            cnt[threadIdx.x] = 0;
        __syncthreads();
        int np = -1;
        bool ver = false;
        if (have)
        {
            const size_t g = (size_t)run * (size_t)per_run + (size_t)d;
            const int q1 = order[draws[2 * g]], q2 = order[draws[2 * g + 1]];
            double d21[3], d21b[3];
            np = pose_constraints(geom + (size_t)q1 * 12, geom + (size_t)q2 * 12, tau, d21, d21b);
            ver = tp[q1] && tp[q2];
            stage[g] = (uint8_t)(np | (ver ? 0x80 : 0));
        }
#pragma unroll
        for (int k = 0; k < EBVO_PC_NUM_STAGES; ++k)
        {
            const unsigned long long m = __ballot(np >= k), mv = __ballot(np >= k && ver);
            if (lane == 0 && m)
                atomicAdd(&cnt[k], (int)__popcll(m));
            if (lane == 0 && mv)
                atomicAdd(&cnt[EBVO_PC_NUM_STAGES + k], (int)__popcll(mv));
        }
        __syncthreads();
        if (threadIdx.x < POSE_CASC_COUNTERS && cnt[threadIdx.x])
            atomicAdd(&counters[(size_t)run * POSE_CASC_COUNTERS + threadIdx.x], cnt[threadIdx.x]);
        __syncthreads();
    }
}

unsigned grid_for(int64_t n, int64_t cap)
{
    const int64_t b = (n + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

// ---- glibc rand(), restated (__srandom_r / __random_r, TYPE_3: degree 31, separation 3) --------------------------------
int32_t rng_next(PoseRng &g)
{
    const int a = g.pos, b = (g.pos + 28) % 31; // x[i - 31], x[i - 3]
    const uint32_t v = (uint32_t)g.r[a] + (uint32_t)g.r[b];
    g.r[a] = (int32_t)v;
    g.pos = (g.pos + 1) % 31;
    return (int32_t)(v >> 1);
}

void rng_seed(PoseRng &g, uint32_t seed)
{
    int32_t word = (int32_t)(seed == 0 ? 1u : seed);
    g.r[0] = word;
    for (int i = 1; i < 31; ++i)
    {
        const long hi = word / 127773, lo = word % 127773; // 16807 * word mod 2^31 - 1 without overflow (Schrage)
        word = (int32_t)(16807 * lo - 2836 * hi);
        if (word < 0)
            word += 2147483647;
        g.r[i] = word;
    }
    g.pos = 3; // x[31..33] = x[0..2] are already in place; the next word is x[34]
    for (int k = 0; k < 310; ++k)
        (void)rng_next(g);
    g.seeded = true;
}

// the loop's `do { idx1 = rand() % top_n; idx2 = rand() % top_n; } while (idx1 == idx2);`, nb times
void draw_pairs(PoseRng &g, int64_t top_n, int nb, int32_t *out)
{
    for (int d = 0; d < nb; ++d)
    {
        uint64_t i1, i2;
        do
        {
            i1 = (uint64_t)rng_next(g) % (uint64_t)top_n;
            i2 = (uint64_t)rng_next(g) % (uint64_t)top_n;
        } while (i1 == i2);
        out[2 * d] = (int32_t)i1;
        out[2 * d + 1] = (int32_t)i2;
    }
}
} // namespace

int pose_run(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, const int32_t *d_rp, int n_kf,
             const ebvo_edge *d_cfL, const ebvo_edge *d_cfR, int n, const ebvo_stereo_calib *cal, const ebvo_pose_params *p,
             ebvo_pose_result *res, uint8_t *inlier, double *quad_geom, int32_t *rank_order, bool insufficient)
{
    ebvo_pose_result r;
    memset(&r, 0, sizeof r);
    r.R[0] = r.R[4] = r.R[8] = 1.0;
    r.best_q1 = r.best_q2 = -1;
    r.n_quads = n;
    r.top_n = (int64_t)(p->top_rank_fraction * (double)n);
    r.dynamic_max_iter = p->max_iterations;
    PoseRng &g = ctx->pose_rng;
    if (!p->continue_stream || !g.seeded)
        rng_seed(g, p->rand_seed);
    if (insufficient || n < 2 || r.top_n < 2)
    {
        r.status = 1;
        if (inlier && n > 0)
            memset(inlier, 0, (size_t)n);
        *res = r;
        return EBVO_OK;
    }
    const int B = ctx->pose_batch > 0 ? ctx->pose_batch : POSE_BATCH_DEFAULT;
    const size_t nz = (size_t)n, bz = (size_t)B;
    int rc;
    if ((rc = ebvo_grow(ctx, s, s.pose_geom, sizeof(double) * 17 * nz)) || (rc = ebvo_grow(ctx, s, s.pose_order, (sizeof(int32_t) + 1) * nz)) ||
        (rc = ebvo_grow(ctx, s, s.pose_draw, sizeof(int32_t) * 3 * bz)) || (rc = ebvo_grow(ctx, s, s.pose_hyp, (sizeof(double) * 12 + 1) * bz)))
        return rc;
    double *d_geom = (double *)s.pose_geom.p, *d_pts = d_geom + 12 * nz, *d_hyp = (double *)s.pose_hyp.p;
    int32_t *d_order = (int32_t *)s.pose_order.p, *d_draws = (int32_t *)s.pose_draw.p, *d_cnt = d_draws + 2 * bz;
    uint8_t *d_ok = (uint8_t *)(d_hyp + 12 * bz), *d_mask = (uint8_t *)(d_order + nz);
    hipStream_t st = s.stream;
    // MotionTracker uses get_left_calib_matrix() for both cameras (src/MotionTracker.cpp:76)
    const FinalCalib C = final_calib_host(cal->K_left, cal->K_left, cal->R21, cal->T21);
    PoseK K;
    memcpy(K.K, cal->K_left, sizeof K.K);
    const PoseTaus tau{p->tau_length, p->tau_t1, p->tau_t2, p->tau_tangent};
    const double thr = p->max_reproj_error;
    {
        ProfScope ps(ctx, s, K_MISC);
        hipLaunchKernelGGL(pose_prepare_kernel, dim3(grid_for(n, 2048)), dim3(256), 0, st, C, d_kfL, d_kfR, d_rp, n_kf, d_cfL, d_cfR,
                           n, d_geom, d_pts);
        hipLaunchKernelGGL(pose_rank_kernel, dim3(grid_for(n_kf, 1 << 30)), dim3(256), 0, st, d_rp, n_kf, d_order);
    }
    EBVO_HIP(ctx, hipGetLastError());
    if (quad_geom)
        EBVO_HIP(ctx, hipMemcpyAsync(quad_geom, d_geom, sizeof(double) * 12 * nz, hipMemcpyDeviceToHost, st));
    if (rank_order)
        EBVO_HIP(ctx, hipMemcpyAsync(rank_order, d_order, sizeof(int32_t) * nz, hipMemcpyDeviceToHost, st));

    // the loop's state (Ransac_State) and its sequential replay
    const int64_t max_it = p->max_iterations, min_it = p->min_iterations;
    const double log_prob_missing_model = std::log(1.0 - p->success_prob);
    int64_t it = 0, dyn = max_it, best = 0;
    double ratio = 0.0;
    double best_rt[12];
    std::vector<int32_t> draws(2 * bz), cnt(bz);
    std::vector<uint8_t> ok(bz);
    // 0: the loop goes on; 1: it ended (for condition or termination test); 2: it needs a draw beyond max_draws
    auto top = [&]() {
        if (!(it < max_it) || (it > min_it && it > dyn))
            return 1;
        return r.draws >= p->max_draws ? 2 : 0;
    };
    int state;
    while ((state = top()) == 0)
    {
        const int nb = (int)std::min<int64_t>(B, p->max_draws - r.draws);
        const PoseRng g0 = g;
        draw_pairs(g, r.top_n, nb, draws.data());
        EBVO_HIP(ctx, hipMemcpyAsync(d_draws, draws.data(), sizeof(int32_t) * 2 * nb, hipMemcpyHostToDevice, st));
        EBVO_HIP(ctx, hipMemsetAsync(d_cnt, 0, sizeof(int32_t) * nb, st));
        {
            ProfScope ps(ctx, s, K_MISC);
            hipLaunchKernelGGL(pose_hyp_kernel, dim3(grid_for(nb, 2048)), dim3(256), 0, st, d_draws, nb, d_order, d_geom, tau, d_ok,
                               d_hyp);
            hipLaunchKernelGGL(pose_score_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)((nb + POSE_TILE_H - 1) / POSE_TILE_H)),
                               dim3(256), 0, st, d_hyp, d_ok, nb, d_pts, n, K, thr, d_cnt);
        }
        EBVO_HIP(ctx, hipGetLastError());
        EBVO_HIP(ctx, hipMemcpyAsync(ok.data(), d_ok, (size_t)nb, hipMemcpyDeviceToHost, st));
        EBVO_HIP(ctx, hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int32_t) * nb, hipMemcpyDeviceToHost, st));
        EBVO_HIP(ctx, hipStreamSynchronize(st));
        int used = 0, best_d = -1;
        for (; used < nb; ++used)
        {
            if (used > 0 && (state = top()) != 0)
                break;
            ++r.draws;
            if (!ok[used])
            {
                it = it > 0 ? it - 1 : 0; // a rejected draw (:113-133), then the for loop's ++
                ++it;
                continue;
            }
            ++r.hypotheses;
            const int64_t c = cnt[used];
            if (c > best)
            {
                best = c;
                ratio = (double)c / (double)n;
                best_d = used;
                r.best_q1 = draws[2 * used];
                r.best_q2 = draws[2 * used + 1];
            }
            if (ratio >= 0.95)
                dyn = min_it;
            else if (ratio <= 0.05)
                dyn = max_it;
            else
            {
                // std::pow(ratio, 2) is compiled to ratio * ratio
                const double prob_outlier = 1.0 - ratio * ratio;
                double v = std::ceil(log_prob_missing_model / std::log(prob_outlier) * p->dyn_num_trials_mult);
                v = !(v > 0.0) ? 0.0 : v > 0x1p62 ? 0x1p62 : v; // clamped before the integer conversion (a divergence)
                dyn = (int64_t)v;
            }
            ++it;
        }
        if (used < nb) // the generator ends where the loop stopped drawing
        {
            g = g0;
            draw_pairs(g, r.top_n, used, draws.data());
        }
        if (best_d >= 0)
        {
            EBVO_HIP(ctx, hipMemcpyAsync(best_rt, d_hyp + (size_t)best_d * 12, sizeof best_rt, hipMemcpyDeviceToHost, st));
            EBVO_HIP(ctx, hipStreamSynchronize(st)); // before the next batch overwrites it
        }
        if (state)
            break;
    }
    r.status = state == 2 ? 2 : 0;
    r.iterations = it;
    r.dynamic_max_iter = dyn;
    r.best_inliers = best;
    r.inlier_ratio = ratio;
    r.found = best > 0;
    if (r.found)
    {
        memcpy(r.R, best_rt, sizeof r.R);
        memcpy(r.t, best_rt + 9, sizeof r.t);
    }
    if (inlier)
    {
        if (r.found)
        {
            PoseRt H;
            memcpy(H.Rt, best_rt, sizeof H.Rt);
            hipLaunchKernelGGL(pose_mask_kernel, dim3(grid_for(n, 2048)), dim3(256), 0, st, H, d_pts, n, K, thr, d_mask);
            EBVO_HIP(ctx, hipGetLastError());
            EBVO_HIP(ctx, hipMemcpyAsync(inlier, d_mask, nz, hipMemcpyDeviceToHost, st));
        }
        else
            memset(inlier, 0, nz);
    }
    EBVO_HIP(ctx, hipStreamSynchronize(st));
    *res = r;
    return EBVO_OK;
}

// ---- ground-truth rows ---------------------------------------------------------------------------------------------------
namespace
{
struct PoseSel // the selected rows, compacted (pointers into Slot::pose_sel)
{
    ebvo_edge *kfL, *kfR, *cfL, *cfR;
    double *full_geom;
    int32_t *rp, *map, *crow, *cq, *tot, *full_order;
    uint8_t *tp, *full_mask;
    int n_rows, n;
};

// d_on: per KF mate, its quads are selected; d_tp (may be NULL): b_is_TP per quad.  Waits for the two totals.
int pose_select(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, const int32_t *d_rp, int n_kf,
                const ebvo_edge *d_cfL, const ebvo_edge *d_cfR, int n, const uint8_t *d_on, const uint8_t *d_tp, bool want_tp, PoseSel *out)
{
    const size_t kz = (size_t)n_kf, nz = (size_t)n;
    const size_t o_geom = sizeof(ebvo_edge) * 2 * (kz + nz), o_i32 = o_geom + sizeof(double) * 12 * nz,
                 n_i32 = (kz + 1) + nz + 2 * kz + 2 + nz, o_u8 = o_i32 + sizeof(int32_t) * n_i32;
    if (int rc = ebvo_grow(ctx, s, s.pose_sel, o_u8 + 2 * nz + 64))
        return rc;
    char *base = (char *)s.pose_sel.p;
    PoseSel S;
    S.kfL = (ebvo_edge *)base;
    S.kfR = S.kfL + kz;
    S.cfL = S.kfR + kz;
    S.cfR = S.cfL + nz;
    S.full_geom = (double *)(base + o_geom);
    S.rp = (int32_t *)(base + o_i32);
    S.map = S.rp + kz + 1;
    S.crow = S.map + nz;
    S.cq = S.crow + kz;
    S.tot = S.cq + kz;
    S.full_order = S.tot + 2;
    S.tp = (uint8_t *)(base + o_u8);
    S.full_mask = S.tp + nz;
    S.n_rows = S.n = 0;
    if (n_kf > 0 && n > 0)
    {
        hipStream_t st = s.stream;
        int32_t tot[2] = {0, 0};
        {
            ProfScope ps(ctx, s, K_MISC);
            hipLaunchKernelGGL(pose_select_scan_kernel, dim3(1), dim3(POSE_SCAN_T), 0, st, d_on, d_rp, n_kf, S.crow, S.cq, S.rp, S.tot);
        }
        EBVO_HIP(ctx, hipGetLastError());
        EBVO_HIP(ctx, hipMemcpyAsync(tot, S.tot, sizeof tot, hipMemcpyDeviceToHost, st));
        EBVO_HIP(ctx, hipStreamSynchronize(st));
        if (tot[0] < 0 || tot[0] > n_kf || tot[1] < 0 || tot[1] > n)
        {
            ctx->last_error = "pose row selection: the device totals exceed the rows given";
            return EBVO_ERR_HIP;
        }
        S.n_rows = tot[0];
        S.n = tot[1];
        if (S.n > 0)
        {
            ProfScope ps(ctx, s, K_MISC);
            hipLaunchKernelGGL(pose_select_gather_kernel, dim3(grid_for(n_kf, 2048)), dim3(256), 0, st, d_on, d_rp, n_kf, S.crow, S.cq,
                               d_kfL, d_kfR, d_cfL, d_cfR, d_tp, S.kfL, S.kfR, S.cfL, S.cfR, S.map, want_tp ? S.tp : nullptr);
            EBVO_HIP(ctx, hipGetLastError());
        }
    }
    *out = S;
    return EBVO_OK;
}
} // namespace

int pose_run_gt(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, const int32_t *d_rp, int n_kf,
                const ebvo_edge *d_cfL, const ebvo_edge *d_cfR, int n, const uint8_t *d_on, int64_t n_listed,
                const ebvo_stereo_calib *cal, const ebvo_pose_params *p, ebvo_pose_result *res, uint8_t *inlier, double *quad_geom,
                int32_t *rank_order)
{
    PoseSel S;
    if (int rc = pose_select(ctx, s, d_kfL, d_kfR, d_rp, n_kf, d_cfL, d_cfR, n, d_on, nullptr, false, &S))
        return rc;
    const size_t nz = (size_t)n, cz = (size_t)S.n;
    std::vector<uint8_t> cmask(inlier ? cz : 0); // pose_run forms the mask on the device only for a caller that asks for it
    if (int rc = pose_run(ctx, s, S.kfL, S.kfR, S.rp, S.n_rows, S.cfL, S.cfR, S.n, cal, p, res, inlier ? cmask.data() : nullptr, nullptr,
                          nullptr, n_listed < 2))
        return rc;
    if (inlier && n > 0)
        memset(inlier, 0, nz);
    if (res->status == 1 || !(inlier || quad_geom || rank_order))
        return EBVO_OK;
    // pose_run left the compacted geometry, rank order and mask in the slot (its own layout over cz quads)
    hipStream_t st = s.stream;
    const double *c_geom = (const double *)s.pose_geom.p;
    const int32_t *c_order = (const int32_t *)s.pose_order.p;
    const uint8_t *c_mask = (const uint8_t *)(c_order + cz);
    const bool mask = inlier && res->found;
    if (mask)
        EBVO_HIP(ctx, hipMemsetAsync(S.full_mask, 0, nz, st));
    if (quad_geom)
        EBVO_HIP(ctx, hipMemsetAsync(S.full_geom, 0, sizeof(double) * 12 * nz, st));
    {
        ProfScope ps(ctx, s, K_MISC);
        hipLaunchKernelGGL(pose_scatter_kernel, dim3(grid_for(n, 2048)), dim3(256), 0, st, S.map, S.n, n, mask ? c_mask : nullptr,
                           mask ? S.full_mask : nullptr, c_geom, quad_geom ? S.full_geom : nullptr, c_order,
                           rank_order ? S.full_order : nullptr);
    }
    EBVO_HIP(ctx, hipGetLastError());
    if (mask)
        EBVO_HIP(ctx, hipMemcpyAsync(inlier, S.full_mask, nz, hipMemcpyDeviceToHost, st));
    if (quad_geom)
        EBVO_HIP(ctx, hipMemcpyAsync(quad_geom, S.full_geom, sizeof(double) * 12 * nz, hipMemcpyDeviceToHost, st));
    if (rank_order)
        EBVO_HIP(ctx, hipMemcpyAsync(rank_order, S.full_order, sizeof(int32_t) * nz, hipMemcpyDeviceToHost, st));
    EBVO_HIP(ctx, hipStreamSynchronize(st));
    return EBVO_OK;
}

void pose_cascade_insufficient(ebvo_ctx *ctx, const ebvo_pose_params *p, int64_t n, int n_runs, ebvo_pose_cascade_run *runs)
{
    PoseRng &g = ctx->pose_rng;
    if (!p->continue_stream || !g.seeded)
        rng_seed(g, p->rand_seed);
    for (int k = 0; k < n_runs; ++k)
    {
        ebvo_pose_cascade_run &r = runs[k];
        memset(&r, 0, sizeof r);
        r.status = 1;
        r.n_quads = n;
        r.top_n = (int64_t)(p->top_rank_fraction * (double)n);
        for (int j = 0; j < EBVO_PC_NUM_STAGES; ++j)
            r.stages[j].stage = j;
    }
}

int pose_cascade_run(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, const int32_t *d_rp, int n_kf,
                     const ebvo_edge *d_cfL, const ebvo_edge *d_cfR, int n, const uint8_t *d_on, int64_t n_listed, const uint8_t *d_tp,
                     const ebvo_stereo_calib *cal, const ebvo_pose_params *p, int n_runs, ebvo_pose_cascade_run *runs,
                     int32_t *draw_idx, uint8_t *draw_stage)
{
    PoseSel S;
    if (int rc = pose_select(ctx, s, d_kfL, d_kfR, d_rp, n_kf, d_cfL, d_cfR, n, d_on, d_tp, true, &S))
        return rc;
    const int64_t top_n = (int64_t)(p->top_rank_fraction * (double)S.n);
    if (n_listed < 2 || S.n < 2 || top_n < 2)
    {
        pose_cascade_insufficient(ctx, p, S.n, n_runs, runs);
        return EBVO_OK;
    }
    PoseRng &g = ctx->pose_rng;
    if (!p->continue_stream || !g.seeded)
        rng_seed(g, p->rand_seed);
    const int per_run = p->max_iterations;
    const size_t cz = (size_t)S.n, dz = (size_t)n_runs * (size_t)per_run, rz = (size_t)n_runs;
    int rc;
    if ((rc = ebvo_grow(ctx, s, s.pose_geom, sizeof(double) * 17 * cz)) || (rc = ebvo_grow(ctx, s, s.pose_order, (sizeof(int32_t) + 1) * cz)) ||
        (rc = ebvo_grow(ctx, s, s.pose_casc, sizeof(int32_t) * (2 * dz + POSE_CASC_COUNTERS * rz) + dz + 64)))
        return rc;
    double *d_geom = (double *)s.pose_geom.p, *d_pts = d_geom + 12 * cz;
    int32_t *d_order = (int32_t *)s.pose_order.p, *d_draws = (int32_t *)s.pose_casc.p, *d_cnt = d_draws + 2 * dz;
    uint8_t *d_stage = (uint8_t *)(d_cnt + POSE_CASC_COUNTERS * rz);
    hipStream_t st = s.stream;
    std::vector<int32_t> draws(2 * dz), cnt(POSE_CASC_COUNTERS * rz, 0);
    EBVO_HIP(ctx, hipMemsetAsync(d_cnt, 0, sizeof(int32_t) * POSE_CASC_COUNTERS * rz, st));
    if (dz)
    {
        const FinalCalib C = final_calib_host(cal->K_left, cal->K_left, cal->R21, cal->T21);
        const PoseTaus tau{p->tau_length, p->tau_t1, p->tau_t2, p->tau_tangent};
        {
            ProfScope ps(ctx, s, K_MISC);
            hipLaunchKernelGGL(pose_prepare_kernel, dim3(grid_for(S.n, 2048)), dim3(256), 0, st, C, S.kfL, S.kfR, S.rp, S.n_rows, S.cfL,
                               S.cfR, S.n, d_geom, d_pts);
            hipLaunchKernelGGL(pose_rank_kernel, dim3(grid_for(S.n_rows, 1 << 30)), dim3(256), 0, st, S.rp, S.n_rows, d_order);
        }
        EBVO_HIP(ctx, hipGetLastError());
        // every draw of every run depends on the random stream alone: run k + 1 continues where run k stopped
        draw_pairs(g, top_n, (int)dz, draws.data());
        EBVO_HIP(ctx, hipMemcpyAsync(d_draws, draws.data(), sizeof(int32_t) * 2 * dz, hipMemcpyHostToDevice, st));
        {
            ProfScope ps(ctx, s, K_POSE_CASCADE);
            hipLaunchKernelGGL(pose_cascade_kernel, dim3((unsigned)((per_run + POSE_CASC_T - 1) / POSE_CASC_T), (unsigned)std::min(n_runs, 32768)),
                               dim3(POSE_CASC_T), 0, st, d_draws, per_run, n_runs, d_order, d_geom, S.tp, tau, d_stage, d_cnt);
        }
        EBVO_HIP(ctx, hipGetLastError());
        EBVO_HIP(ctx, hipMemcpyAsync(cnt.data(), d_cnt, sizeof(int32_t) * POSE_CASC_COUNTERS * rz, hipMemcpyDeviceToHost, st));
        if (draw_stage)
            EBVO_HIP(ctx, hipMemcpyAsync(draw_stage, d_stage, dz, hipMemcpyDeviceToHost, st));
        EBVO_HIP(ctx, hipStreamSynchronize(st));
        if (draw_idx)
            memcpy(draw_idx, draws.data(), sizeof(int32_t) * 2 * dz);
    }
    for (int k = 0; k < n_runs; ++k)
    {
        const int32_t *c = cnt.data() + (size_t)k * POSE_CASC_COUNTERS;
        if (c[0] != per_run)
        {
            ctx->last_error = "constraint cascade: the device counted other draws than were drawn";
            return EBVO_ERR_HIP;
        }
        ebvo_pose_cascade_run &r = runs[k];
        memset(&r, 0, sizeof r);
        r.n_quads = S.n;
        r.top_n = top_n;
        r.draws = per_run;
        const int64_t initial = c[EBVO_PC_NUM_STAGES];
        for (int j = 0; j < EBVO_PC_NUM_STAGES; ++j)
        {
            ebvo_pose_cascade_stage &g2 = r.stages[j];
            g2.stage = j;
            g2.surviving = c[j];
            g2.veridical = c[EBVO_PC_NUM_STAGES + j];
            if (j == EBVO_PC_BASELINE)
            {
                g2.precision = static_cast<double>(g2.veridical) / static_cast<double>(per_run);
                g2.recall = 1.0;
            }
            else
            {
                g2.recall = static_cast<double>(g2.veridical) / static_cast<double>(initial);
                g2.precision = (g2.surviving == 0) ? 0.0 : static_cast<double>(g2.veridical) / static_cast<double>(g2.surviving);
            }
        }
    }
    return EBVO_OK;
}

// ---- inlier refit (pose_refit_kernels.hip) over every quad or over the ground-truth rows -----------------------------------
int pose_refit_run(ebvo_ctx *ctx, Slot &s, const ebvo_edge *d_kfL, const ebvo_edge *d_kfR, const int32_t *d_rp, int n_kf,
                   const ebvo_edge *d_cfL, const ebvo_edge *d_cfR, int n, const uint8_t *d_on, const ebvo_stereo_calib *cal,
                   const ebvo_pose_params *p, const ebvo_pose_refine_params *rp, const double *R0, const double *t0,
                   ebvo_pose_refined *out, uint8_t *inlier)
{
    ebvo_pose_refined r;
    memset(&r, 0, sizeof r);
    memcpy(r.R, R0, sizeof r.R);
    memcpy(r.t, t0, sizeof r.t);
    r.status = 1;
    r.stop_reason = 4;
    r.n_quads = n;
    PoseSel S;
    if (d_on)
    {
        if (int rc = pose_select(ctx, s, d_kfL, d_kfR, d_rp, n_kf, d_cfL, d_cfR, n, d_on, nullptr, false, &S))
            return rc;
        r.n_quads = S.n;
    }
    if (r.n_quads < 2) // nothing to fit: nothing launched
    {
        if (inlier && n > 0)
            memset(inlier, 0, (size_t)n);
        *out = r;
        return EBVO_OK;
    }
    PoseRefitOut o;
    if (int rc = d_on ? pose_refit_device(ctx, s, S.kfL, S.kfR, S.rp, S.n_rows, S.cfL, S.cfR, S.n, S.map, n, cal, p->max_reproj_error, rp,
                                          R0, t0, &o, inlier)
                      : pose_refit_device(ctx, s, d_kfL, d_kfR, d_rp, n_kf, d_cfL, d_cfR, n, nullptr, n, cal, p->max_reproj_error, rp, R0,
                                          t0, &o, inlier))
        return rc;
    memcpy(r.R, o.Rt, sizeof r.R);
    memcpy(r.t, o.Rt + 9, sizeof r.t);
    r.status = o.status;
    r.stop_reason = o.stop;
    r.rounds_run = o.rounds_run;
    r.steps_kept = o.steps_kept;
    r.fit_quads = o.fit;
    r.inliers = o.inliers;
    r.cost_first = o.cost_first;
    r.cost_last = o.cost_last;
    *out = r;
    return EBVO_OK;
}
