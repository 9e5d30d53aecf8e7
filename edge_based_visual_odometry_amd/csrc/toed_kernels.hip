// toed_kernels.hip -- third-order edge detection on gfx950 (MI355X).
//
// Replaces ThirdOrderEdgeDetectionCPU::{preprocessing, convolve_img, non_maximum_suppresion}
// (src/toed/cpu_toed.cpp:82-120, :122-376, :386-582 of the reference).
//
// Arithmetic contract (bit parity with the CPU path): IEEE double, separate multiply and add
// (this file is compiled with -ffp-contract=off), every accumulator receives its addends in the
// reference's order (p ascending, q ascending), each addend has the reference's shape:
//   integer phase   fx += v*(Gx[q]*G[p]),  fy += v*(G[q]*Gx[p]),  others (v*Kcol[q])*Krow[p]
//   shifted phases  all nine (v*Kcol[q])*Krow[p]
// Common sub-expressions (v*Kcol[q] feeds several responses and two phases) are formed once;
// that does not change any rounded value.  Out-of-image taps are fed as +0.0 from a zero-padded
// LDS tile instead of being skipped: x + (+-0.0) == x for every running sum that started at +0.0.
//
// Kernels
//   toed_conv_kernel     K1: LDS-staged fp64 tile (8 x 32 pixels + 9-pixel halo); one thread per
//                            (input pixel, x-phase): the two sub-pixel phases that share the column
//                            taps (18 fp64 accumulators) in registers, filter taps as scalar (SGPR)
//                            operands, software-pipelined tap fetch
//   toed_nms_kernel      K2: NMS + parabola fit per interpolated pixel, flags + per-row counts
//   toed_rowscan_kernel  K3a: exclusive scan of the per-row counts
//   toed_compact_kernel  K3b: ordered (raster) stream compaction of the flagged pixels
//   toed_finalize_kernel K3c: dense per-edge epilogue (sub-pixel position, atan2, records)
// Hybrid mode (second half of the file; same bits out):
//   toed_screen_fused_kernel   S1+S2: separable fp32 screen and relaxed NMS of a 12 x 30-pixel tile, all in LDS
//   toed_compact_phase_kernel (offsets of a row: the counts of the rows in front of it, summed by the row's own wave)
//                              S2b/c: candidate ranks and the four phase lists, ordered, no atomics; one wave per grid row,
//                              eight flag bytes per lane, no LDS
//   toed_exact_centre_kernel   S3b: the nine exact responses of every candidate; marks its NMS neighbours
//   toed_need_{count,compact}_kernel
//                              S3c-0..1: the distinct neighbour grid points, by phase (a wave per row, a bitmap word per lane)
//   toed_exact_mags_kernel     S3c-3: exact gradient magnitude of every distinct neighbour point
//   toed_exact_decide_kernel   S3d: exact NMS + sub-pixel fit;  toed_cand_scatter_kernel S4: edge records
#include <cstring>

#include <hip/hip_ext.h>

#include "ebvo_internal.h"
#include <atomic>
#include "ebvo_math.h"

namespace
{

// sigma = 2 Gaussian-derivative taps (values: src/toed/cpu_toed.cpp:143-146 and :157-160).
// [d][k]: derivative order d = 0..3, tap k = offset + 9.
const double h_TAP_INT[4][19] = {
    {7.99187055345274e-06, 6.69151128824427e-05, 0.000436341347522880, 0.00221592420596900,
     0.00876415024678427, 0.0269954832565940, 0.0647587978329459, 0.120985362259572, 0.176032663382150,
     0.199471140200716, 0.176032663382150, 0.120985362259572, 0.0647587978329459, 0.0269954832565940,
     0.00876415024678427, 0.00221592420596900, 0.000436341347522880, 6.69151128824427e-05,
     7.99187055345274e-06},
    {1.79817087452687e-05, 0.000133830225764885, 0.000763597358165040, 0.00332388630895351,
     0.0109551878084803, 0.0269954832565940, 0.0485690983747094, 0.0604926811297858, 0.0440081658455374, 0,
     -0.0440081658455374, -0.0604926811297858, -0.0485690983747094, -0.0269954832565940,
     -0.0109551878084803, -0.00332388630895351, -0.000763597358165040, -0.000133830225764885,
     -1.79817087452687e-05},
    {3.84608770384913e-05, 0.000250931673309160, 0.00122721003990810, 0.00443184841193801,
     0.0115029471989044, 0.0202466124424455, 0.0202371243227956, 0, -0.0330061243841531,
     -0.0498677850501791, -0.0330061243841531, 0, 0.0202371243227956, 0.0202466124424455,
     0.0115029471989044, 0.00443184841193801, 0.00122721003990810, 0.000250931673309160,
     3.84608770384913e-05},
    {7.75461189639711e-05, 0.000434948233735878, 0.00176581889075666, 0.00498582946343026,
     0.00890109009439027, 0.00674887081414851, -0.00910670594525801, -0.0302463405648929,
     -0.0302556140188070, 0, 0.0302556140188070, 0.0302463405648929, 0.00910670594525801,
     -0.00674887081414851, -0.00890109009439027, -0.00498582946343026, -0.00176581889075666,
     -0.000434948233735878, -7.75461189639711e-05},
};
const double h_TAP_HALF[4][19] = {
    {2.38593182706025e-05, 0.000176297841183723, 0.00101452402864988, 0.00454678125079553,
     0.0158698259178337, 0.0431386594132558, 0.0913245426945110, 0.150568716077402, 0.193334058401425,
     0.193334058401425, 0.150568716077402, 0.0913245426945110, 0.0431386594132558, 0.0158698259178337,
     0.00454678125079553, 0.00101452402864988, 0.000176297841183723, 2.38593182706025e-05,
     2.51475364429622e-06},
    {5.07010513250303e-05, 0.000330558452219480, 0.00164860154655606, 0.00625182421984385,
     0.0178535541575629, 0.0377463269865988, 0.0570778391840694, 0.0564632685290258, 0.0241667573001781,
     -0.0241667573001781, -0.0564632685290258, -0.0570778391840694, -0.0377463269865988,
     -0.0178535541575629, -0.00625182421984385, -0.00164860154655606, -0.000330558452219480,
     -5.07010513250303e-05, -5.97253990520353e-06},
    {0.000101774904498039, 0.000575722637615595, 0.00242534650599113, 0.00745956298958641,
     0.0161177919477999, 0.0222433712599600, 0.0128425138164156, -0.0164684533209659,
     -0.0453126699378339, -0.0453126699378339, -0.0164684533209659, 0.0128425138164156,
     0.0222433712599600, 0.0161177919477999, 0.00745956298958641, 0.00242534650599113,
     0.000575722637615595, 0.000101774904498039, 1.35560938637843e-05},
    {0.000190921146395817, 0.000914200719419500, 0.00311688729895755, 0.00713098700075939,
     0.00920573886249338, 0.000589786359165606, -0.0205123484567749, -0.0344073042598751,
     -0.0177474623923183, 0.0177474623923183, 0.0344073042598751, 0.0205123484567749,
     -0.000589786359165606, -0.00920573886249338, -0.00713098700075939, -0.00311688729895755,
     -0.000914200719419500, -0.000190921146395817, -2.92094529738860e-05},
};

// Filter tables in device memory, passed to the kernel as one pointer (a kernel argument keeps
// the base address in SGPRs; __constant__ symbols are reached through the GOT under -fPIC and
// the compiler re-loads that address inside the tap loop).  Wave-uniform indices -> s_load.
//   INT[4][19], HALF[4][19], then the integer-phase products formed before touching the pixel
//   (src/toed/cpu_toed.cpp:207-208): PROD_FX[p+8][q+8] = Gx[q]*G[p], PROD_FY[p+8][q+8] = G[q]*Gx[p]
struct ToedTables
{
    double tap_int[4][19];
    double tap_half[4][19];
    double prod_fx[17][17];
    double prod_fy[17][17];
    float screen_dc[4][2]; // FP32 screen: 127.5 * sum(K_row) * sum(K_col) of (gx, gy) per phase (sy << 1 | sx)
};
ToedTables *g_tables_dev[16] = {nullptr}; // per HIP device

constexpr int TILE_W = 32;
constexpr int TILE_H = 8;
constexpr int HALO = 9;
constexpr int LDS_W = TILE_W + 2 * HALO; // 50
constexpr int LDS_H = TILE_H + 2 * HALO; // 26
constexpr int MAX_BATCH = 2;

struct CandRec
{
    double x, y, smag, tox, toy;
};

struct ImgBatch
{
    const uint8_t *img[MAX_BATCH];
    double *maps[MAX_BATCH];
    uint8_t *flag[MAX_BATCH];
    int32_t *row_cnt[MAX_BATCH];
    int32_t *row_off[MAX_BATCH];
    int32_t *counts[MAX_BATCH];
    int32_t *src[MAX_BATCH];
    ebvo_edge *edges[MAX_BATCH];
    double *all4[MAX_BATCH];
    // hybrid mode: per-candidate records and flags
    CandRec *rec[MAX_BATCH];
    int32_t *cand_flag[MAX_BATCH]; // [2][cap]: is a maximum, is a kept maximum
    int32_t *cand_off[MAX_BATCH];  // [2][cap+1]: exclusive scans of the flags
    int32_t *lists[MAX_BATCH];     // hybrid: [12][cap] candidate lists (0-3 by phase)
    int32_t *lcount[MAX_BATCH];    // hybrid: [12] their lengths
};

// nine responses: fx fy fxx fxy fyy fxxy fxyy fxxx fyyy -> (x-derivative order, y-derivative order)
#define EBVO_ACCUM9(acc, cp, rp)  \
    acc[0] += cp[1] * rp[0];      \
    acc[1] += cp[0] * rp[1];      \
    acc[2] += cp[2] * rp[0];      \
    acc[3] += cp[1] * rp[1];      \
    acc[4] += cp[0] * rp[2];      \
    acc[5] += cp[2] * rp[1];      \
    acc[6] += cp[1] * rp[2];      \
    acc[7] += cp[3] * rp[0];      \
    acc[8] += cp[0] * rp[3];

// third-order orientation vector (unnormalised), src/toed/cpu_toed.cpp:224-225
__device__ inline void third_order_dir(const double *f, double &tx, double &ty)
{
    const double fx = f[0], fy = f[1], fxx = f[2], fxy = f[3], fyy = f[4], fxxy = f[5], fxyy = f[6],
                 fxxx = f[7], fyyy = f[8];
    double TO_Ix = fx * (2 * fxx * fxx + 2 * fxy * fxy) + fy * (2 * fxx * fxy + 2 * fyy * fxy) +
                   2 * fx * fy * fxxy + fy * fy * fxyy + fx * fx * fxxx;
    double TO_Iy = fx * (2 * fxx * fxy + 2 * fyy * fxy) + fy * (2 * fyy * fyy + 2 * fxy * fxy) +
                   2 * fx * fy * fxyy + fx * fx * fxxy + fy * fy * fyyy;
    // the normalisation (:226-228) is applied in toed_finalize_kernel, only where an edge survives NMS
    tx = TO_Ix;
    ty = TO_Iy;
}

// Interpolated pixel (I, J) of a 2H x 2W plane lives in the sub-plane of its phase (I&1, J&1) at
// (I>>1, J>>1): [sy][sx][H][W].  Keeps every access of a fixed phase unit-stride.
__device__ inline size_t midx(int I, int J, int h, int w)
{
    return ((size_t)(((I & 1) << 1) | (J & 1)) * h + (I >> 1)) * w + (J >> 1);
}

// K1 ---------------------------------------------------------------------------------------
// SX = 0: phases (0,0) [17x17, integer grid] and (1,0); SX = 1: phases (0,1) and (1,1).
// Both phases of a thread use the same column taps, so v*Kcol[q] is formed once per tap.
template <int SX>
__device__ inline void conv_body(const double (*tile)[LDS_W], const ToedTables *__restrict__ T,
                                 double *__restrict__ maps, int h, int w, int i, int j, int ty, int tx)
{
    const double(*colk)[19] = SX ? T->tap_half : T->tap_int;
    double a0[9], a1[9]; // phase (0, SX) and (1, SX)
#pragma unroll
    for (int r = 0; r < 9; ++r)
        a0[r] = a1[r] = 0.0;

#pragma unroll 1
    for (int p = -HALO; p <= HALO; ++p)
    {
        double ru[4], rs[4]; // row taps: integer grid / half-pixel grid (wave-uniform -> SGPRs)
#pragma unroll
        for (int d = 0; d < 4; ++d)
        {
            ru[d] = T->tap_int[d][p + 9];
            rs[d] = T->tap_half[d][p + 9];
        }
        const bool row00 = (p >= -8) && (p <= 8);
        const int pr = row00 ? p + 8 : 0;
        const double *__restrict__ trow = &tile[ty + HALO - p][tx + HALO];
        // software pipeline: the pixel and the column taps of tap q+1 are fetched while tap q is accumulated
        double vn = trow[HALO];
        double kn[4], pxn = 0, pyn = 0;
#pragma unroll
        for (int d = 0; d < 4; ++d)
            kn[d] = colk[d][0];
        if (SX == 0)
        {
            pxn = T->prod_fx[pr][0];
            pyn = T->prod_fy[pr][0];
        }
#pragma unroll 1
        for (int q = -HALO; q <= HALO; ++q)
        {
            const double v = vn, px = pxn, py = pyn;
            double ck[4];
#pragma unroll
            for (int d = 0; d < 4; ++d)
                ck[d] = v * kn[d];
            const int qn = min(q + 1, HALO);
            vn = trow[-qn];
#pragma unroll
            for (int d = 0; d < 4; ++d)
                kn[d] = colk[d][qn + 9];
            if (SX == 0)
            {
                const int qp = min(max(qn + 8, 0), 16);
                pxn = T->prod_fx[pr][qp];
                pyn = T->prod_fy[pr][qp];
                if (row00 && q >= -8 && q <= 8) // wave-uniform; integer phase, src/toed/cpu_toed.cpp:207-216
                {
                    a0[0] += v * px;
                    a0[1] += v * py;
                    a0[2] += ck[2] * ru[0];
                    a0[3] += ck[1] * ru[1];
                    a0[4] += ck[0] * ru[2];
                    a0[5] += ck[2] * ru[1];
                    a0[6] += ck[1] * ru[2];
                    a0[7] += ck[3] * ru[0];
                    a0[8] += ck[0] * ru[3];
                }
            }
            else
            {
                EBVO_ACCUM9(a0, ck, ru) // shifted in x only, :251-260
            }
            EBVO_ACCUM9(a1, ck, rs) // shifted in y (SX = 0, :295-304) or in both (SX = 1, :339-348)
        }
    }

    const size_t plane = (size_t)4 * h * w;
    double tx0, ty0;
    {
        const size_t o = midx(2 * i, 2 * j + SX, h, w);
        maps[PL_IX * plane + o] = a0[0];
        maps[PL_IY * plane + o] = a0[1];
        maps[PL_MAG * plane + o] = sqrt(a0[0] * a0[0] + a0[1] * a0[1]);
        third_order_dir(a0, tx0, ty0);
        maps[PL_TOX * plane + o] = tx0;
        maps[PL_TOY * plane + o] = ty0;
    }
    {
        const size_t o = midx(2 * i + 1, 2 * j + SX, h, w);
        maps[PL_IX * plane + o] = a1[0];
        maps[PL_IY * plane + o] = a1[1];
        maps[PL_MAG * plane + o] = sqrt(a1[0] * a1[0] + a1[1] * a1[1]);
        third_order_dir(a1, tx0, ty0);
        maps[PL_TOX * plane + o] = tx0;
        maps[PL_TOY * plane + o] = ty0;
    }
}

// grid (tiles_x, tiles_y, 2 * n_img): z = 2 * image + x-phase
__global__ __launch_bounds__(256) void toed_conv_kernel(ImgBatch B, const ToedTables *__restrict__ T, int h,
                                                        int w)
{
    __shared__ double tile[LDS_H][LDS_W];
    const int im = blockIdx.z >> 1, sx = blockIdx.z & 1;
    const uint8_t *__restrict__ img = B.img[im];
    double *__restrict__ maps = B.maps[im];
    const int j0 = blockIdx.x * TILE_W, i0 = blockIdx.y * TILE_H;

    for (int t = threadIdx.x; t < LDS_H * LDS_W; t += 256)
    {
        const int r = t / LDS_W, c = t - r * LDS_W;
        const int ii = i0 + r - HALO, jj = j0 + c - HALO;
        double v = 0.0;
        if (ii >= 0 && ii < h && jj >= 0 && jj < w)
            v = (double)img[(size_t)ii * w + jj];
        tile[r][c] = v;
    }
    __syncthreads();

    const int tx = threadIdx.x & (TILE_W - 1), ty = threadIdx.x >> 5;
    const int i = i0 + ty, j = j0 + tx;
    if (i >= h || j >= w)
        return;
    if (sx)
        conv_body<1>(tile, T, maps, h, w, i, j, ty, tx);
    else
        conv_body<0>(tile, T, maps, h, w, i, j, ty, tx);
}

// NMS + parabola fit at interpolated pixel (i, j): src/toed/cpu_toed.cpp:406-511, in two steps.
// Step 1 (:406-477): early rejects, unit gradient, the sector's neighbour offsets -- (a1, b1) the axis
// neighbour and (a2, b2) the diagonal neighbour on the plus side, the minus side negates both -- and slope.
struct NmsSector
{
    double nx, ny, slope;
    int a1, b1, a2, b2;
};

__device__ inline bool nms_sector(double m, double gx, double gy, NmsSector &S)
{
    if (m <= 2) // :406
        return false;
    if (fabs(gx) < 10e-6 && fabs(gy) < 10e-6) // :410
        return false;
    const double nx = gx / m, ny = gy / m;
    int a1, b1, a2, b2;
    double slope;
    if (gx >= 0 && gy >= 0)
    {
        if (gx >= gy) { slope = ny / nx; a1 = 0; b1 = 1; a2 = 1; b2 = 1; }
        else { slope = nx / ny; a1 = 1; b1 = 0; a2 = 1; b2 = 1; }
    }
    else if (gx < 0 && gy >= 0)
    {
        if (fabs(gx) < gy) { slope = -nx / ny; a1 = 1; b1 = 0; a2 = 1; b2 = -1; }
        else { slope = -ny / nx; a1 = 0; b1 = -1; a2 = 1; b2 = -1; }
    }
    else if (gx < 0 && gy < 0)
    {
        if (fabs(gx) >= fabs(gy)) { slope = ny / nx; a1 = 0; b1 = -1; a2 = -1; b2 = -1; }
        else { slope = nx / ny; a1 = -1; b1 = 0; a2 = -1; b2 = -1; }
    }
    else if (gx >= 0 && gy < 0)
    {
        if (gx < fabs(gy)) { slope = -nx / ny; a1 = -1; b1 = 0; a2 = -1; b2 = 1; }
        else { slope = -ny / nx; a1 = 0; b1 = 1; a2 = -1; b2 = 1; }
    }
    else
        return false;
    S.nx = nx; S.ny = ny; S.slope = slope;
    S.a1 = a1; S.b1 = b1; S.a2 = a2; S.b2 = b2;
    return true;
}

// Step 2 (:423-511): the four neighbour magnitudes in the order (a1,b1), (a2,b2), (-a1,-b1), (-a2,-b2).
__device__ inline bool nms_finish(double m, const NmsSector &S, int i, int j, double m_p1, double m_p2, double m_m1,
                                  double m_m2, double &pos_x, double &pos_y, double &smag)
{
    const double slope = S.slope, nx = S.nx, ny = S.ny;
    const double fp = m_p1 * (1 - slope) + m_p2 * slope;
    const double fm = m_m1 * (1 - slope) + m_m2 * slope;
    const double s = sqrt(1 + slope * slope);
    if (!((m > fm && m > fp) || (m > fm && m >= fp) || (m >= fm && m > fp))) // :481-483
        return false;
    const double A = (fm + fp - 2 * m) / (2 * s * s);
    const double Bc = (fp - fm) / (2 * s);
    const double C = m;
    const double s_star = -Bc / (2 * A);
    const double max_f = A * s_star * s_star + Bc * s_star + C;
    if (!(fabs(s_star) <= sqrt(2.0))) // :494
        return false;
    const double sgx = max_f * nx, sgy = max_f * ny;
    smag = sqrt(sgx * sgx + sgy * sgy);
    pos_x = j + s_star * nx;
    pos_y = i + s_star * ny;
    return true;
}

template <class MagAt>
__device__ inline bool nms_core(double m, double gx, double gy, int i, int j, MagAt mag_at, double &pos_x,
                                double &pos_y, double &smag)
{
    NmsSector S;
    if (!nms_sector(m, gx, gy, S))
        return false;
    const double m_p1 = mag_at(S.a1, S.b1), m_p2 = mag_at(S.a2, S.b2);
    const double m_m1 = mag_at(-S.a1, -S.b1), m_m2 = mag_at(-S.a2, -S.b2);
    return nms_finish(m, S, i, j, m_p1, m_p2, m_m1, m_m2, pos_x, pos_y, smag);
}

__device__ inline bool nms_eval(const double *__restrict__ Ix, const double *__restrict__ Iy,
                                const double *__restrict__ M, int h, int w, int i, int j, double &pos_x,
                                double &pos_y, double &smag)
{
    const size_t o = midx(i, j, h, w);
    return nms_core(M[o], Ix[o], Iy[o], i, j, [&](int di, int dj) { return M[midx(i + di, j + dj, h, w)]; }, pos_x,
                    pos_y, smag);
}

// K2 ---------------------------------------------------------------------------------------
// grid (ceil((W2-20)/64), ceil((H2-20)/4), n_img), block (64, 4): one wave per row segment.
__global__ __launch_bounds__(256) void toed_nms_kernel(ImgBatch B, int h, int w)
{
    const int W2 = 2 * w, H2 = 2 * h;
    const size_t plane = (size_t)H2 * W2;
    const double *maps = B.maps[blockIdx.z];
    const int j = 10 + blockIdx.x * 64 + threadIdx.x;
    const int i = 10 + blockIdx.y * 4 + threadIdx.y;
    if (i >= H2 - 10) // wave-uniform
        return;
    int f = 0;
    if (j < W2 - 10)
    {
        double px, py, sm;
        if (nms_eval(maps + PL_IX * plane, maps + PL_IY * plane, maps + PL_MAG * plane, h, w, i, j, px, py, sm))
        {
            const double x = (px - 1) / 2, y = (py - 1) / 2; // :538,542
            f = (x > 10 && x < w - 10 && y > 10 && y < h - 10) ? 3 : 1; // :553-554
        }
        B.flag[blockIdx.z][(size_t)i * W2 + j] = (uint8_t)f;
    }
    const unsigned long long any = __ballot(f != 0), kept = __ballot(f == 3);
    if (threadIdx.x == 0 && any)
    {
        atomicAdd(&B.row_cnt[blockIdx.z][i], __popcll(any));
        atomicAdd(&B.row_cnt[blockIdx.z][H2 + i], __popcll(kept));
    }
}

// K3a --------------------------------------------------------------------------------------
// one wave per image: exclusive scan of both per-row counters; totals to counts[0..1].
__global__ __launch_bounds__(64) void toed_rowscan_kernel(ImgBatch B, int H2, int count_base)
{
    const int32_t *cnt = B.row_cnt[blockIdx.x];
    int32_t *off = B.row_off[blockIdx.x];
    const int lane = threadIdx.x;
    const int per = (H2 + 63) / 64;
    for (int which = 0; which < 2; ++which)
    {
        const int32_t *c = cnt + which * H2;
        int32_t *o = off + which * (H2 + 1);
        const int beg = lane * per, end = min(H2, beg + per);
        int s = 0;
        for (int r = beg; r < end; ++r)
            s += c[r];
        int incl = s;
        for (int d = 1; d < 64; d <<= 1)
        {
            const int t = __shfl_up(incl, d);
            if (lane >= d)
                incl += t;
        }
        int run = incl - s;
        for (int r = beg; r < end; ++r)
        {
            o[r] = run;
            run += c[r];
        }
        if (lane == 63)
        {
            o[H2] = incl;
            B.counts[blockIdx.x][count_base + which] = incl;
        }
    }
}

// K3b --------------------------------------------------------------------------------------
// one block per interpolated row; ordered compaction of the flagged pixels of that row.
__global__ __launch_bounds__(256) void toed_compact_kernel(ImgBatch B, int h, int w, int cap)
{
    const int W2 = 2 * w, H2 = 2 * h;
    const int i = 10 + blockIdx.x;
    if (i >= H2 - 10)
        return;
    const uint8_t *flag = B.flag[blockIdx.y] + (size_t)i * W2;
    const int32_t *off = B.row_off[blockIdx.y];
    int32_t *src = B.src[blockIdx.y];
    int base_all = off[i], base_kept = off[(H2 + 1) + i];
    __shared__ int w_all[4], w_kept[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int j0 = 10; j0 < W2 - 10; j0 += 256)
    {
        const int j = j0 + threadIdx.x;
        const int f = (j < W2 - 10) ? flag[j] : 0;
        const unsigned long long m_all = __ballot(f != 0), m_kept = __ballot(f == 3);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (lane == 0)
        {
            w_all[wid] = __popcll(m_all);
            w_kept[wid] = __popcll(m_kept);
        }
        __syncthreads();
        int pre_all = 0, pre_kept = 0, tot_all = 0, tot_kept = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
        {
            if (k < wid)
            {
                pre_all += w_all[k];
                pre_kept += w_kept[k];
            }
            tot_all += w_all[k];
            tot_kept += w_kept[k];
        }
        if (f)
        {
            const int r_all = base_all + pre_all + __popcll(m_all & below);
            const int r_kept = (f == 3) ? base_kept + pre_kept + __popcll(m_kept & below) : -1;
            if (r_all < cap)
            {
                src[2 * r_all] = i * W2 + j;
                src[2 * r_all + 1] = r_kept;
            }
        }
        base_all += tot_all;
        base_kept += tot_kept;
        __syncthreads();
    }
}

// K3c --------------------------------------------------------------------------------------
// dense epilogue: one thread per NMS maximum (grid-stride; the count lives in device memory).
__global__ __launch_bounds__(256) void toed_finalize_kernel(ImgBatch B, int h, int w, int cap)
{
    const int W2 = 2 * w, H2 = 2 * h;
    const size_t plane = (size_t)H2 * W2;
    const double *maps = B.maps[blockIdx.y];
    const int32_t *src = B.src[blockIdx.y];
    ebvo_edge *edges = B.edges[blockIdx.y];
    double *all4 = B.all4[blockIdx.y];
    const int n = min(B.counts[blockIdx.y][0], cap);
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x)
    {
        const int o = src[2 * t], kr = src[2 * t + 1];
        const int i = o / W2, j = o - i * W2;
        double px = 0, py = 0, sm = 0;
        nms_eval(maps + PL_IX * plane, maps + PL_IY * plane, maps + PL_MAG * plane, h, w, i, j, px, py, sm);
        const double x = (px - 1) / 2, y = (py - 1) / 2;
        if (!all4 && !(kr >= 0 && kr < cap)) // the resident pipeline keeps no subpix_edge_pts_final: a maximum outside the
            continue;                         // 10-px border leaves nothing behind
        const size_t mo = midx(i, j, h, w);
        // src/toed/cpu_toed.cpp:226-229: normalise the third-order vector, then atan2(TO_Ix, -TO_Iy)
        double TO_Ix = maps[PL_TOX * plane + mo], TO_Iy = maps[PL_TOY * plane + mo];
        const double TO_mag = sqrt(TO_Ix * TO_Ix + TO_Iy * TO_Iy);
        TO_Ix /= TO_mag;
        TO_Iy /= TO_mag;
        const double th = ebvo_atan2(TO_Ix, -TO_Iy);
        if (all4)
        {
            all4[(size_t)t * 4 + 0] = x;
            all4[(size_t)t * 4 + 1] = y;
            all4[(size_t)t * 4 + 2] = th;
            all4[(size_t)t * 4 + 3] = sm;
        }
        if (kr >= 0 && kr < cap)
        {
            ebvo_edge e;
            e.x = x;
            e.y = y;
            e.theta = th;
            e.index = kr; // src/toed/cpu_toed.cpp:562
            e.pad = 0;
            edges[kr] = e;
        }
    }
}


// ==========================================================================================
// Hybrid TOED: separable screening + exact re-evaluation.  Bit-identical results, ~3x less work.
//
// The direct-form convolution above spends 27.6 k fp64 operations on every pixel, but only ~7 % of the
// interpolated pixels become edges.  Here a cheap SEPARABLE convolution (it is only a screen) produces gx, gy, |g|,
// a RELAXED non-maximum test with a tolerance well above the screen's error selects a superset of the pixels the
// reference accepts, and every selected pixel is then evaluated in the reference's exact arithmetic (same taps, same
// order, no FMA): its nine responses and the two-response magnitude of its four NMS neighbours (each distinct
// neighbour grid point once).  The exact NMS decision, sub-pixel position, magnitude and orientation are computed
// from those exact values only, so the edge list equals the strict path's bit for bit; a pixel that the relaxed
// screen rejects is rejected by the exact test too.
//
// The screen runs in FP32 (round 3; it was fp64 with a tolerance of 1e-6).  Round 4: the pixels are RECENTRED,
// x = v - 127.5 (exact in float, |x| <= 127.5; a pixel outside the image is v = 0, i.e. x = -127.5, in every row and column
// alike), and the constant 127.5 * sum(K_row) * sum(K_col) is added back after the column pass -- every partial sum of the
// two passes is at most half of what it was, and so is the worst-case rounding error.  The budget below is no longer a
// hand derivation: tools/screen_error_bound.py computes it from THIS file's tap tables and the kernel's accumulation
// order (FMA chain s_k = fl(s_{k-1} + x_k fl(K_k)): |error| <= u X (sum|K| + sum_k cum_k), cum_k the running sum of |K| --
// each step rounds a partial sum of magnitude <= X cum_k; the column pass adds sum|K_col| times the row error), and
// tests/test_screen_bound.py re-derives it and checks the constants and the static_asserts below.  u = 2^-24:
//   |d gx|, |d gy| <= 7.66e-5                                                              (SCREEN_E_G)
//   |d |g||        <= sqrt(2) E_G + 3 u max|g| = 1.22e-4,  max |g| = 72.7                  (SCREEN_E_M)
//   |d slope|      <= 2 E_G / |major| + u = 1.09e-4,  |major| >= |g| / sqrt(2) >= 1.41    (SCREEN_E_S)
//   a comparison   m >= f - tol of two screened magnitudes, f = p1 (1 - s) + p2 s:
//                  tol >= 2 E_M + 6 u max|g| + E_S |p2 - p1| = 2.69e-4 + 1.09e-4 |p2 - p1|
// These are worst-case bounds (every rounding error aligned); what the screen really does is MEASURED: the diagnostic
// entry point ebvo_toed_screen_audit runs the detector with a variant of this kernel that keeps its gx, gy, |g| and
// returns max |screen - exact| over all candidates and neighbour points (tests/test_gpu_screen_audit.py: ~1e-6 on the three
// full-size workloads and on full-size saturating 0 / 255 stripe and checkerboard images; asserted below the budget).
// The relaxed test uses TOL_M = 5e-4 (1.9 x what a comparison needs, 4.1 x E_M, 6.5 x E_G) wherever a magnitude or a gradient
// component is compared with a constant or with another component, and TOL_M + TOL_S |p2 - p1|, TOL_S = 2.5e-4
// (2.3 x E_S), where it is compared with an interpolated neighbour:
//   |g| > 2 - TOL_M, and |g| >= fm - tol and |g| >= fp - tol with the screen's own interpolated neighbours; where the gradient
//   sector is ambiguous (|gx|, |gy| or ||gx| - |gy|| below TOL_M: the exact sector could be either of two) the point is tested
//   against both of them (see the kernel); the |s*| <= sqrt(2) test is left to the exact stage.
// A wider tolerance only adds candidates, never removes one (round 3: 1e-3 / 5e-4 against twice these error bounds,
// +2.1 % candidates; now +1.0 %); every TOED parity test runs in this mode.
// ==========================================================================================
constexpr float SCREEN_TOL_M = 5e-4f;
constexpr float SCREEN_TOL_S = 2.5e-4f;
constexpr float SCREEN_CENTRE = 127.5f;
// tools/screen_error_bound.py (rounded up)
constexpr double SCREEN_E_G = 7.67e-5, SCREEN_E_M = 1.22e-4, SCREEN_E_S = 1.09e-4, SCREEN_G_MAX = 72.8;
constexpr double SCREEN_U = 5.9604644775390625e-08; // 2^-24
static_assert(SCREEN_TOL_M >= 1.5 * (2.0 * SCREEN_E_M + 6.0 * SCREEN_U * SCREEN_G_MAX), "a comparison of two screened magnitudes");
static_assert(SCREEN_TOL_M >= 3.0 * (2.0 * SCREEN_E_G), "the sector tests compare two screened gradient components");
static_assert(SCREEN_TOL_S >= 2.0 * SCREEN_E_S, "the interpolation weight");

// S1+S2 fused -------------------------------------------------------------------------------
// The screen in one kernel: the separable planes never leave LDS.  One block screens the four phases of a
// 12 x 30-pixel tile; it needs |g| one grid step around it, i.e. a 14 x 32 "ext" tile, i.e. a 32 x 50 image tile.
//   row pass     thread = (image-tile row, 4 adjacent ext columns): 22 pixels in registers feed 16 accumulators
//                (G and Gx taps; integer positions with 17 and 19 taps, half-pixel positions) -> six R planes in LDS,
//                a thread's four columns of a plane as ONE 16-byte store
//   column pass  thread = (ext column, phase, 7 adjacent ext rows): 25 + 25 R values feed 14 accumulators; gx, gy stay
//                in registers, |g| goes to LDS (aliasing the R planes once every thread is past them)
//   relaxed NMS  every thread decides its own <= 7 grid points; flags and per-row candidate counts as before
// In FP32 the block needs 26.6 KB of LDS (52 KB as doubles: three blocks per CU, and the kernel spent 54 % of its wave
// time waiting at its barriers) and ~half the registers: six blocks per CU hide each other's barriers.
constexpr int FT_H = 12, FT_W = 30;           // pixels screened per block
constexpr int FE_H = FT_H + 2, FE_W = FT_W + 2; // ext tile
constexpr int FI_H = FE_H + 2 * HALO, FI_W = FE_W + 2 * HALO; // image tile 32 x 50
static_assert(FI_W + 6 == 56 && FI_H * (FE_W / 4) == 256 && FE_W * 4 * (FE_H / 7) == 256, "one work item per thread in both passes");
static_assert(FE_W == 32 && FE_H == 14, "32 ext columns per wave half, row groups 0-6 / 7-13");

constexpr int FI_P = 56; // image-tile row pitch in bytes (>= FI_W + 2, multiple of 4)
struct FusedLds
{
    uint32_t img[FI_H][FI_P / 4]; // the image tile as bytes
    union
    {
        float R[6][FI_H][FE_W]; // [0,1] 17-tap integer (G, Gx); [2,3] 19-tap integer; [4,5] half-pixel
        float M[4][FE_H][FE_W]; // |g| of the ext tile per phase ((sy << 1) | sx)
    };
    float tap[2][19][2];        // [half][tap][G, Gx]
};
static_assert(sizeof(FusedLds) <= 27306, "six blocks per CU (160 KB of LDS)");

// DIAG (ebvo_toed_screen_audit only): the screen's gx, gy, |g| of every grid point it decides are also written to three float
// planes of 2H x 2W, for the audit kernel below to compare with the exact stage's values.
typedef float v2f __attribute__((ext_vector_type(2)));

struct ScreenDiag
{
    float *plane[MAX_BATCH]; // [3][2H][2W]
};

template <bool DIAG>
__global__ __launch_bounds__(256) void toed_screen_fused_kernel(ImgBatch B, const ToedTables *__restrict__ T, int h, int w,
                                                                ScreenDiag D)
{
    __shared__ __attribute__((aligned(16))) FusedLds L;
    const uint8_t *__restrict__ img = B.img[blockIdx.z];
    const int W2 = 2 * w, H2 = 2 * h;
    const int j0 = blockIdx.x * FT_W - 1, i0 = blockIdx.y * FT_H - 1; // pixel of ext (0, 0)
    const int tid = threadIdx.x;
    if (tid < 2 * 19 * 2)
    {
        const int half = tid / 38, k = (tid % 38) >> 1, d = tid & 1;
        L.tap[half][k][d] = (float)(half ? T->tap_half[d][k] : T->tap_int[d][k]);
    }
    // image tile: ONE 8-byte load per thread (32 rows x 7 chunks = 56 bytes cover the 50 columns).  The image buffer has 64
    // readable bytes either side, rows are clamped and masked, columns masked per byte.
    if (tid < FI_H * 7)
    {
        const int r = tid / 7, k = tid - r * 7;
        const int ii = i0 + r - HALO, jc = j0 - HALO + 8 * k;
        const int ic = min(max(ii, 0), h - 1);
        unsigned long long bits;
        __builtin_memcpy(&bits, img + (size_t)ic * w + jc, 8);
        const bool rok = ii >= 0 && ii < h;
        unsigned long long masked = 0; // bytes outside the image read as 0, as the reference skips those taps
#pragma unroll
        for (int b = 0; b < 8; ++b)
        {
            const int jj = jc + b;
            if (rok && jj >= 0 && jj < w)
                masked |= bits & (0xffull << (8 * b));
        }
        L.img[r][2 * k] = (uint32_t)masked;
        L.img[r][2 * k + 1] = (uint32_t)(masked >> 32);
    }
    __syncthreads();
    // ---- row pass: R[.][r][c] = sum_q img[r][c + HALO - q] * tap[q]
    {
        const int r = tid >> 3, c0 = (tid & 7) * 4;
        float v[22];
#pragma unroll
        for (int q = 0; q < 6; ++q) // c0 is a multiple of 4: six aligned words hold the 22 pixels
        {
            const uint32_t wq = L.img[r][(c0 >> 2) + q];
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * q + b < 22) // recentred: |x| <= 127.5 halves every partial sum (error budget above)
                    v[4 * q + b] = (float)((wq >> (8 * b)) & 0xffu) - SCREEN_CENTRE;
        }
        // (G, Gx) pairs as packed floats: one v_pk_fma_f32 updates both accumulators of a column (same IEEE fused operations,
        // same order: the error budget is per component; half the instructions)
        v2f a17[4], ah[4];
#pragma unroll
        for (int c = 0; c < 4; ++c)
            a17[c] = ah[c] = (v2f){0.0f, 0.0f};
#pragma unroll
        for (int q = -8; q <= 8; ++q)
        {
            const v2f ti = *reinterpret_cast<const v2f *>(L.tap[0][q + 9]); // {G, Gx}, integer table
            const v2f th = *reinterpret_cast<const v2f *>(L.tap[1][q + 9]); // half-pixel table
#pragma unroll
            for (int c = 0; c < 4; ++c)
            {
                const float x = v[c + HALO - q];
                const v2f xx = (v2f){x, x};
                a17[c] = __builtin_elementwise_fma(xx, ti, a17[c]);
                ah[c] = __builtin_elementwise_fma(xx, th, ah[c]);
            }
        }
        float o[6][4];
        {
            const v2f ti0 = *reinterpret_cast<const v2f *>(L.tap[0][0]), ti18 = *reinterpret_cast<const v2f *>(L.tap[0][18]);
            const v2f th0 = *reinterpret_cast<const v2f *>(L.tap[1][0]), th18 = *reinterpret_cast<const v2f *>(L.tap[1][18]);
#pragma unroll
            for (int c = 0; c < 4; ++c)
            {
                const float xl = v[c + HALO + 9], xr = v[c + HALO - 9]; // taps q = -9 and q = +9
                const v2f l2 = (v2f){xl, xl}, r2 = (v2f){xr, xr};
                const v2f i19 = __builtin_elementwise_fma(r2, ti18, __builtin_elementwise_fma(l2, ti0, a17[c]));
                const v2f h19 = __builtin_elementwise_fma(r2, th18, __builtin_elementwise_fma(l2, th0, ah[c]));
                o[0][c] = a17[c].x;
                o[1][c] = a17[c].y;
                o[2][c] = i19.x;
                o[3][c] = i19.y;
                o[4][c] = h19.x;
                o[5][c] = h19.y;
            }
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) // one 16-byte store per plane (a wave: 8 rows x 8 column groups = 1 KB, eight bank passes)
            *reinterpret_cast<float4 *>(&L.R[k][r][c0]) = make_float4(o[k][0], o[k][1], o[k][2], o[k][3]);
    }
    __syncthreads();
    // ---- column pass: thread = (ext column, phase, 7 ext rows)
    const int c = tid & 31, ph = (tid >> 5) & 3, sy = ph >> 1, sx = ph & 1, e0 = (tid >> 7) * 7;
    float fx[7], fy[7], mg[7];
    {
        // x kernel: sx ? half : integer (17 taps for phase (0,0), 19 otherwise); y kernel: sy ? half : integer
        const int base = sx ? 4 : (sy ? 2 : 0);
        const int pm = (ph == 0) ? 8 : 9;
        v2f rr[25]; // {R filtered with Gx along x, R filtered with G along x}, image-tile rows e0 .. e0 + 24
#pragma unroll
        for (int k = 0; k < 25; ++k)
            rr[k] = (v2f){L.R[base + 1][e0 + k][c], L.R[base][e0 + k][c]};
        v2f acc[7];
#pragma unroll
        for (int e = 0; e < 7; ++e)
            acc[e] = (v2f){0.0f, 0.0f};
#pragma unroll
        for (int p = -9; p <= 9; ++p)
        {
            if (p < -pm || p > pm) // uniform per wave half: phase (0,0) has no +-9 taps
                continue;
            const v2f kk = *reinterpret_cast<const v2f *>(L.tap[sy][p + 9]); // {G, Gx} along y
#pragma unroll
            for (int e = 0; e < 7; ++e) // fx: Gx along x, G along y; fy: G along x, Gx along y -- one packed FMA
                acc[e] = __builtin_elementwise_fma(rr[e + HALO - p], kk, acc[e]);
        }
#pragma unroll
        for (int e = 0; e < 7; ++e)
        {
            fx[e] = acc[e].x;
            fy[e] = acc[e].y;
        }
        const float dcx = T->screen_dc[ph][0], dcy = T->screen_dc[ph][1]; // 127.5 * sum(K_row) * sum(K_col)
#pragma unroll
        for (int e = 0; e < 7; ++e)
        {
            fx[e] += dcx;
            fy[e] += dcy;
            mg[e] = __builtin_sqrtf(__builtin_fmaf(fx[e], fx[e], fy[e] * fy[e]));
        }
    }
    __syncthreads(); // every thread is done with R: M may overwrite it
#pragma unroll
    for (int e = 0; e < 7; ++e)
        L.M[ph][e0 + e][c] = mg[e];
    __syncthreads();
    // ---- relaxed NMS of this thread's grid points
    // |g| of the grid neighbours one step along the rows / columns: the thread's phase is fixed, so the LDS offsets
    // (plane, ext row, ext column) of "one grid step up / down / left / right" are three constants per axis
    const float *Mflat = &L.M[0][0][0];
    auto row_step = [&](int da) { return ((((sy + da) & 1) - sy) * 2 * FE_H + ((sy + da) >> 1)) * FE_W; };
    auto col_step = [&](int db) { return (((sx + db) & 1) - sx) * FE_H * FE_W + ((sx + db) >> 1); };
    const int rdn = row_step(-1), rup = row_step(1), cdn = col_step(-1), cup = col_step(1);
    const int lane = tid & 63;
#pragma unroll
    for (int e = 0; e < 7; ++e)
    {
        const int er = e0 + e;                     // ext row, column c
        const int i = i0 + er, j = j0 + c;         // pixel
        const int I = 2 * i + sy, J = 2 * j + sx;  // grid point
        int f = 0;
        const bool mine = er >= 1 && er <= FT_H && c >= 1 && c <= FT_W && I >= 10 && I < H2 - 10 && J >= 10 && J < W2 - 10;
        if (mine)
        {
            const float m = mg[e];
            if (m > 2.0f - SCREEN_TOL_M)
            {
                const float gx = fx[e], gy = fy[e], ax = fabsf(gx), ay = fabsf(gy);
                if (ax < SCREEN_TOL_M || ay < SCREEN_TOL_M || fabsf(ax - ay) < SCREEN_TOL_M)
                {
                    // The exact sector could differ from the screen's.  Round 3 flagged every such point (an axis-aligned
                    // synthetic image -- gy == 0 exactly -- then flags every point with |g| > 2 and overflows the candidate
                    // buffers).  Round 4: the point is tested against BOTH sectors the exact gradient can lie in.  They share
                    // one neighbour pair and differ in the other, which enters with a weight of at most w_up:
                    //   |gy| < T (or |gx| < T): the two sectors next to the x (y) axis.  Axis neighbours in common; the diagonal
                    //     is the one above or the one below; exact slope <= (T + E_G) / (|major| - E_G) <= 2 T / |major|, so
                    //     fp lies within w_up * max|diagonal - axis| of the axis neighbour;
                    //   ||gx| - |gy|| < T: the two sectors next to the diagonal.  Diagonal neighbours in common; the axis
                    //     neighbour is the horizontal or the vertical one; 1 - slope <= (T + 2 E_G) / (major - E_G) <= 2 T / major.
                    // The signs of the components the case relies on are certain (|component| >= T > E_G).  T_M covers the rest
                    // as in the unambiguous test below (two screened magnitudes, the float arithmetic).
                    const bool px = gx >= 0, py = gy >= 0;
                    const int ctr = (ph * FE_H + er) * FE_W + c;
                    const int rP = py ? rup : rdn, rM = py ? rdn : rup, cP = px ? cup : cdn, cM = px ? cdn : cup;
                    float np, nm, dp, dm, w_up; // shared neighbour (+ / - side), largest distance of the uncertain ones from it
                    if (ay < SCREEN_TOL_M || ax < SCREEN_TOL_M)
                    {
                        const bool xd = ay < SCREEN_TOL_M; // x dominates
                        const int aP = xd ? cP : rP, aM = xd ? cM : rM, o1 = xd ? rup : cup, o2 = xd ? rdn : cdn;
                        np = Mflat[ctr + aP];
                        nm = Mflat[ctr + aM];
                        dp = fmaxf(fabsf(Mflat[ctr + aP + o1] - np), fabsf(Mflat[ctr + aP + o2] - np));
                        dm = fmaxf(fabsf(Mflat[ctr + aM + o1] - nm), fabsf(Mflat[ctr + aM + o2] - nm));
                        w_up = 2.0f * SCREEN_TOL_M / (xd ? ax : ay);
                    }
                    else
                    {
                        np = Mflat[ctr + rP + cP];
                        nm = Mflat[ctr + rM + cM];
                        dp = fmaxf(fabsf(Mflat[ctr + cP] - np), fabsf(Mflat[ctr + rP] - np));
                        dm = fmaxf(fabsf(Mflat[ctr + cM] - nm), fabsf(Mflat[ctr + rM] - nm));
                        w_up = 2.0f * SCREEN_TOL_M / fmaxf(ax, ay);
                    }
                    if (m >= np - (SCREEN_TOL_M + w_up * dp) && m >= nm - (SCREEN_TOL_M + w_up * dm))
                        f = 1;
                }
                else
                {
                    // the sector table of nms_core, by selects:
                    //   quadrant (sign of gx, gy) x (which of |gx|, |gy| dominates) -> axis step (a1, b1), diagonal
                    //   step (a2, b2), slope = minor / major with the quadrant's sign convention
                    const bool px = gx >= 0, py = gy >= 0;
                    // "x dominates" exactly as the reference compares in each quadrant
                    const bool xdom = px ? (py ? gx >= gy : !(gx < ay)) : (py ? !(ax < gy) : ax >= ay);
                    const float num = xdom ? ((px == py) ? gy : -gy) : ((px == py) ? gx : -gx);
                    const float den = xdom ? gx : gy;
                    const float slope = num / den;
                    // diagonal step: sign of gy along rows, sign of gx along columns; axis step: the dominant axis only
                    // (a2, b2) = (sign gy, sign gx); (a1, b1) = (0, b2) if x dominates, (a2, 0) otherwise
                    const int ctr = (ph * FE_H + er) * FE_W + c;
                    const int rP = py ? rup : rdn, rM = py ? rdn : rup, cP = px ? cup : cdn, cM = px ? cdn : cup;
                    const float p1 = Mflat[ctr + (xdom ? cP : rP)], p2 = Mflat[ctr + rP + cP];
                    const float m1 = Mflat[ctr + (xdom ? cM : rM)], m2 = Mflat[ctr + rM + cM];
                    const float fp = p1 * (1 - slope) + p2 * slope;
                    const float fm = m1 * (1 - slope) + m2 * slope;
                    const float tp = SCREEN_TOL_M + SCREEN_TOL_S * fabsf(p2 - p1);
                    const float tm = SCREEN_TOL_M + SCREEN_TOL_S * fabsf(m2 - m1);
                    if (m >= fm - tm && m >= fp - tp)
                        f = 1;
                }
            }
            B.flag[blockIdx.z][(size_t)I * W2 + J] = (uint8_t)f;
            if (DIAG)
            {
                float *dp = D.plane[blockIdx.z];
                const size_t plane = (size_t)H2 * W2, o = (size_t)I * W2 + J;
                dp[o] = fx[e];
                dp[plane + o] = fy[e];
                dp[2 * plane + o] = mg[e];
            }
        }
        // candidates of grid row I by column parity: a wave holds 32 columns x (sx = 0, 1) of ONE sy and one row group,
        // so all its lanes share I; lanes 0-31 are even columns (sx = 0), lanes 32-63 odd
        const unsigned long long any = __ballot(f != 0);
        if (lane == 0 && any)
        {
            const int ne = __popcll(any & 0xffffffffull), no = __popcll(any >> 32);
            if (ne)
                atomicAdd(&B.row_cnt[blockIdx.z][I], ne);
            if (no)
                atomicAdd(&B.row_cnt[blockIdx.z][H2 + I], no);
        }
    }
}

// ---- word-wise list building, one wave per grid row (toed_compact_phase_kernel, toed_need_compact_kernel) ----------
// The three pieces below stay inside the wave: DPP moves within a row of 16 lanes, v_readlane between the rows.  No LDS,
// no ds_bpermute, no barrier.  All 64 lanes of the wave must call the first two.
template <int CTRL>
__device__ inline int dpp_i32(int v)
{
    return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true);
}

// a[k] := the sum of a[k] over the wave, k = 0..3, the same (scalar) value in every lane
__device__ inline void wave_sum4(int a[4])
{
#pragma unroll
    for (int k = 0; k < 4; ++k)
    {
        int v = a[k];
        v += dpp_i32<0xB1>(v);  // quad_perm:[1,0,3,2]
        v += dpp_i32<0x4E>(v);  // quad_perm:[2,3,0,1]
        v += dpp_i32<0x141>(v); // row_half_mirror
        v += dpp_i32<0x140>(v); // row_mirror: every lane holds the sum of its row of 16
        a[k] = __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
               __builtin_amdgcn_readlane(v, 48);
    }
}

// Exclusive scan over the wave of a packed pair `even | odd << 16` (the wave's sums must stay below 65,536 each: at most
// 16 set bits of a parity per lane here).  Returns the packed sums of the lanes in front; `total` is the wave's packed sum.
__device__ inline unsigned wave_excl_scan_pair(unsigned x, unsigned &total)
{
    int v = (int)x;
    v += dpp_i32<0x111>(v); // row_shr:1 (lanes without a source read 0)
    v += dpp_i32<0x112>(v); // row_shr:2
    v += dpp_i32<0x114>(v); // row_shr:4
    v += dpp_i32<0x118>(v); // row_shr:8: inclusive within the row of 16
    const int t0 = __builtin_amdgcn_readlane(v, 15), t1 = __builtin_amdgcn_readlane(v, 31),
              t2 = __builtin_amdgcn_readlane(v, 47), t3 = __builtin_amdgcn_readlane(v, 63);
    const int row = (int)(threadIdx.x & 63) >> 4;
    const int front = (row > 0 ? t0 : 0) + (row > 1 ? t1 : 0) + (row > 2 ? t2 : 0);
    total = (unsigned)(t0 + t1 + t2 + t3);
    return (unsigned)(v + front) - x;
}

// emit(b) for every set bit b of `m`, in ascending order; the loop runs as long as any lane of the wave has a bit left
template <class Emit>
__device__ inline void walk_set_bits(unsigned m, Emit emit)
{
    while (__any(m != 0u))
    {
        if (m)
        {
            const int b = __ffs((int)m) - 1;
            m &= m - 1u;
            emit(b);
        }
    }
}

// S2c: one WAVE per interpolated row: ordered compaction of the candidates (rank t -> pixel) and, in the same pass,
// the four phase lists in raster order (no atomics: every row knows its offset in its phase's list).
// Round 4: the offsets are no longer a launch of their own (toed_rowscan_phase_kernel: one block per image, ~5 us of latency
// in front of this kernel): every wave adds up the per-row counts in front of its row itself (a few hundred ints, four sums:
// row parity x column parity), and the wave of the first row also adds up ALL rows and publishes what the scan kernel did:
// counts[2] (candidates; 0 if they do not fit), counts[3] = 0, counts[4] (their real number), the lengths of the four phase
// lists, and zeroed lengths for the lists the exact stage appends to.
// Round 7: word-wise.  A block of four waves used to own a row and every lane one flag byte: ten turns for a 2482-wide row,
// each with two barriers, an LDS round trip and three serial 4-way sums, and the row sums went through 24 ds_bpermute a
// call.  Now wave w of block b owns row 10 + 4b + w, a lane takes eight flag bytes with one 8-byte load (a turn = 512
// columns), folds them into an 8-bit mask, and one packed wave scan (wave_excl_scan_pair) gives its offsets in the
// all-candidates order and in the two phase lists of the row; the lane then walks its set bits in column order.  The first
// column of a lane is even, so bit parity = column parity.  The load of a lane that owns at least one column < 2W - 10
// ends at column <= 2W - 4 of its own row: it never leaves the row, let alone the flag array; the other lanes load nothing.
// The candidate arrays hold `cap` (= max_h * max_w) entries; the screen can flag up to four times that on an image made of
// ties (a fine checkerboard).  Then counts[4] keeps the real total and every list length is published as zero: the exact
// stage runs empty, nothing is written past a buffer, and the host re-runs the image on the strict path (toed_sync,
// ebvo_stereo_wait).
__global__ __launch_bounds__(256) void toed_compact_phase_kernel(ImgBatch B, int h, int w, int cap)
{
    const int W2 = 2 * w, H2 = 2 * h;
    const int lane = threadIdx.x & 63;
    const int i = __builtin_amdgcn_readfirstlane(10 + (int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (i >= H2 - 10)
        return;
    const uint8_t *flag = B.flag[blockIdx.y] + (size_t)i * W2 + 10;
    const int32_t *cnt = B.row_cnt[blockIdx.y]; // [2][H2]: candidates of a row in even / odd columns
    int32_t *src = B.src[blockIdx.y];
    int32_t *lists = B.lists[blockIdx.y];
    // sums over the rows in front of this one (and, in the first row's wave, over all rows): [row parity][column parity]
    auto sum_rows = [&](int r_end, int out[4]) {
        int se = 0, so = 0; // the rows of a lane have the lane's parity (stride 64)
        for (int r = lane; r < r_end; r += 64)
        {
            se += cnt[r];
            so += cnt[H2 + r];
        }
        out[0] = lane & 1 ? 0 : se;
        out[1] = lane & 1 ? 0 : so;
        out[2] = lane & 1 ? se : 0;
        out[3] = lane & 1 ? so : 0;
        wave_sum4(out);
    };
    int pre[4];
    sum_rows(i, pre);
    if (i == 10)
    {
        int tot[4];
        sum_rows(H2, tot);
        if (lane == 0)
        {
            const int all = tot[0] + tot[1] + tot[2] + tot[3];
            const bool over = all > cap;
            int32_t *counts = B.counts[blockIdx.y], *lcount = B.lcount[blockIdx.y];
            counts[2] = over ? 0 : all;
            counts[3] = 0;
            counts[4] = all;
            for (int ph = 0; ph < 4; ++ph)
                lcount[ph] = over ? 0 : tot[ph]; // phase = (row parity << 1) | column parity
            for (int k = 4; k < 12; ++k)
                lcount[k] = 0;
        }
    }
    int base_all = pre[0] + pre[1] + pre[2] + pre[3];
    int base_e = pre[(i & 1) * 2], base_o = pre[(i & 1) * 2 + 1];
    int32_t *list_e = lists + (size_t)((i & 1) << 1) * cap; // the list of the odd columns follows it
    const int ncol = W2 - 20; // columns 10 .. 2W - 11
    for (int c0 = 0; c0 < ncol; c0 += 512)
    {
        const int c = c0 + 8 * lane; // the lane's first column, less 10
        unsigned mask = 0;
        if (c < ncol)
        {
            unsigned long long x;
            __builtin_memcpy(&x, flag + c, 8);
            // byte != 0 -> its top bit -> bit k of a nibble (the four products of the multiply land on distinct bits)
            const unsigned lo = (unsigned)x, hi = (unsigned)(x >> 32);
            const unsigned tl = ((((lo & 0x7f7f7f7fu) + 0x7f7f7f7fu) | lo) >> 7) & 0x01010101u;
            const unsigned th = ((((hi & 0x7f7f7f7fu) + 0x7f7f7f7fu) | hi) >> 7) & 0x01010101u;
            mask = ((tl * 0x01020408u) >> 24) | (((th * 0x01020408u) >> 24) << 4);
            if (ncol - c < 8)
                mask &= (1u << (ncol - c)) - 1u;
        }
        unsigned total;
        const unsigned front = wave_excl_scan_pair((unsigned)__popc(mask & 0x55u) | ((unsigned)__popc(mask & 0xaau) << 16), total);
        int r_all = base_all + (int)(front & 0xffffu) + (int)(front >> 16);
        int p_e = base_e + (int)(front & 0xffffu), p_o = base_o + (int)(front >> 16);
        const int o0 = i * W2 + 10 + c;
        walk_set_bits(mask, [&](int b) {
            const int par = b & 1;
            if (r_all < cap)
            {
                src[2 * r_all] = o0 + b;
                src[2 * r_all + 1] = -1;
                list_e[(par ? p_o : p_e) + (cap & -par)] = r_all;
            }
            ++r_all;
            p_o += par;
            p_e += par ^ 1;
        });
        base_all += (int)(total & 0xffffu) + (int)(total >> 16);
        base_e += (int)(total & 0xffffu);
        base_o += (int)(total >> 16);
    }
}

// ---- exact stage -------------------------------------------------------------------------------------------
// Candidates are bucketed by sub-pixel phase so that every wave works on ONE phase: the taps are scalar
// operands again (no per-lane table look-ups, no divergence between the integer phase and the others), and
// the 19 pixels of a tap row are fetched together (19 independent byte loads in flight per lane).
// What the centre kernel hands the decision kernel, one 64-byte record (one cache line) per candidate.  As six arrays
// indexed by candidate rank the stores of a wave (64 candidates of ONE phase: ranks scattered over the raster order) each
// dirtied a 64-byte line for 8 bytes -- 46.6 MB written per pair for 12.5 MB of results in the round-2 counters.
struct __attribute__((aligned(64))) CandExact
{
    double gx, gy, m, tox, toy;
    int32_t sector; // packed (a1+1) | (b1+1)<<2 | (a2+1)<<4 | (b2+1)<<6, or -1 if rejected early
    int32_t pad0;
    double pad1[2];
};
static_assert(sizeof(CandExact) == 64, "one cache line per candidate");

// The exact-|g| map holds a value at every candidate and at every marked neighbour point, i.e. along the edges: 8-byte
// accesses scattered over a 2H x 2W array.  Stored in 2 x 4 tiles of grid points (one 64-byte line each) a candidate and the
// points one grid step around it share at most four lines whatever the direction of the edge (row-major: three rows, a line
// or two each, and a vertical edge dirties a line per point).
__host__ __device__ inline size_t mag_tiles_per_row(int W2) { return (size_t)((W2 + 3) >> 2); }
__host__ __device__ inline size_t mag_map_doubles(int H2, int W2) { return (size_t)((H2 + 1) >> 1) * mag_tiles_per_row(W2) * 8; }
__host__ __device__ inline size_t mag_index(int I, int J, int W2)
{
    return ((size_t)(I >> 1) * mag_tiles_per_row(W2) + (size_t)(J >> 2)) * 8 + (size_t)(((I & 1) << 2) | (J & 3));
}

struct ExactBatch
{
    const uint8_t *img[MAX_BATCH];
    const int32_t *src[MAX_BATCH];
    const int32_t *counts[MAX_BATCH];
    int32_t *lists[MAX_BATCH];   // [12][cap]: 0-3 candidates by phase; 4-11 candidates by (phase, axis)
    int32_t *lcount[MAX_BATCH];  // [12]
    CandExact *cd[MAX_BATCH]; // [cap]
    CandRec *rec[MAX_BATCH];
    int32_t *cand_flag[MAX_BATCH];
    int2 *chunk_cnt[MAX_BATCH];  // [ceil(cap / 256)] maxima / kept maxima among the 256 candidates of a chunk (toed_exact_decide_kernel)
    // neighbour magnitudes, every distinct grid point once
    const uint8_t *flag[MAX_BATCH]; // screen flags: 1 = candidate (its own exact |g| goes to magmap)
    uint32_t *needbits[MAX_BATCH];  // [2H][ceil(2W / 32)] bit J of row I: the exact |g| of grid point (I, J) is needed
    int32_t *need_cnt[MAX_BATCH];   // [2][2H] marked points per grid row, even / odd columns
    double *magmap[MAX_BATCH];      // exact |g| at candidates and at marked points, 2 x 4 tiles (mag_index)
};

// append `value` to list `which` for the lanes with `put`, one atomic per block; returns nothing.
// All 256 threads of the block must call it.
__device__ inline void block_append(bool put, int value, int32_t *__restrict__ list, int32_t *__restrict__ counter,
                                    int *s_cnt /* [5] shared */)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const unsigned long long m = __ballot(put);
    if (lane == 0)
        s_cnt[wid] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0)
    {
        const int tot = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        s_cnt[4] = tot ? atomicAdd(counter, tot) : 0;
    }
    __syncthreads();
    if (put)
    {
        int pre = 0;
        for (int k = 0; k < wid; ++k)
            pre += s_cnt[k];
        list[s_cnt[4] + pre + __popcll(m & ((1ull << lane) - 1ull))] = value;
    }
    __syncthreads();
}

// 19 pixels of image row ii around column j, v[q + 9] = img(ii, j - q), +0.0 outside the image.
// The 19 bytes are fetched with three unaligned 8-byte loads (scattered single-byte loads cost one L1 look-up
// per lane and made this stage texture-address bound).  The image buffer has 64 readable bytes on either side,
// so the loads are always in bounds; bytes that fall outside the row are masked to zero.
struct Row24
{
    unsigned long long w0, w1, w2;
};

__device__ inline Row24 fetch_row(const uint8_t *__restrict__ img, int h, int w, int ii, int j)
{
    const int ic = min(max(ii, 0), h - 1);
    const uint8_t *p = img + (size_t)ic * w + (j - HALO);
    Row24 r;
    __builtin_memcpy(&r.w0, p, 8);
    __builtin_memcpy(&r.w1, p + 8, 8);
    __builtin_memcpy(&r.w2, p + 16, 8);
    return r;
}

// Which of the 19 bytes of a fetched run lie inside the image row: one mask per 32-bit word, once per point.
struct ColMask
{
    unsigned m[5];
};
__device__ inline ColMask column_mask(int w, int j)
{
    // byte k of the run is column j - 9 + k: valid for k in [lo, hi)
    const int lo = max(0, HALO - j), hi = min(19, w + HALO - j);
    ColMask c;
#pragma unroll
    for (int d = 0; d < 5; ++d)
    {
        const int a = min(max(lo - 4 * d, 0), 4), b = min(max(hi - 4 * d, 0), 4); // bytes [a, b) of word d
        const unsigned upto_b = b >= 4 ? 0xffffffffu : ((1u << (8 * b)) - 1u);
        const unsigned upto_a = a >= 4 ? 0xffffffffu : ((1u << (8 * a)) - 1u);
        c.m[d] = upto_b & ~upto_a;
    }
    return c;
}

// `fast`: wave-uniform promise that the whole 19 x 19 window of every lane lies inside the image (no masking).
// Otherwise the five words are masked BEFORE the bytes are taken apart (ten instructions a row): selecting per byte
// cost one instruction per pixel on both paths (the unmasked path paid them as register copies where the two paths merge).
__device__ inline void mask_row(const Row24 &r, int h, int ii, const ColMask &cm, bool fast, unsigned d[5])
{
    d[0] = (unsigned)r.w0, d[1] = (unsigned)(r.w0 >> 32), d[2] = (unsigned)r.w1, d[3] = (unsigned)(r.w1 >> 32), d[4] = (unsigned)r.w2;
    if (!fast)
    {
        const bool rok = ii >= 0 && ii < h;
#pragma unroll
        for (int k = 0; k < 5; ++k)
            d[k] = rok ? (d[k] & cm.m[k]) : 0u;
    }
}

// tap q of a masked row: byte 9 - q of the run.  The half-pixel phases take the byte apart where it is used: it goes
// straight into the low word of ONE register pair whose high word stays zero (byte_as_subnormal).  Taken apart up
// front (unpack_row) the 19 pairs of a row are live together and each gets a v_mov for its high word.
__device__ inline int row_tap(const unsigned d[5], int q)
{
    const int k = 9 - q;
    return (int)((d[k >> 2] >> (8 * (k & 3))) & 0xffu);
}

__device__ inline void unpack_row(const Row24 &r, int h, int ii, const ColMask &cm, bool fast, int v[19])
{
    unsigned d[5];
    mask_row(r, h, ii, cm, fast, d);
#pragma unroll
    for (int k = 0; k < 19; ++k) // byte k of the run is column j - 9 + k, i.e. tap q = 9 - k
        v[18 - k] = (int)((d[k >> 2] >> (8 * (k & 3))) & 0xffu);
}

__device__ inline bool window_inside(int h, int w, int i, int j)
{
    return i >= HALO && i + HALO < h && j >= HALO && j + HALO < w;
}

// all nine responses at input pixel (i, j) for the compile-time phase (SY, SX): conv_body's arithmetic
// Tap tables of the exact stage in LDS, laid out for one 16-byte broadcast read per (tap, kernel pair):
//   tap[half][k][d]   = (half ? tap_half : tap_int)[d][k]   (d = derivative order 0..3, k = tap index 0..18)
//   prod[p][q][0 / 1] = prod_fx / prod_fy                    (integer phase, src/toed/cpu_toed.cpp:207-208)
// Every lane of a wave reads the same address, so the reads are conflict-free broadcasts and the taps arrive as
// vector operands: no SGPR file pressure (76 tap doubles do not fit it; they used to come back through
// v_readlane), no scalar-load waits in the tap loop.
//
// Scaled copies for the three non-integer phases.  There a pixel enters the arithmetic only as
// (v * ck) * rk.  The byte written into the low word of a register pair whose high word is zero IS the fp64 subnormal
// v * 2^-1074, so with ctap = tap * 2^TAP_K1 and rtap = tap * 2^TAP_K2, TAP_K1 + TAP_K2 = 1074, the conversion of the
// byte goes away and every term keeps its bits: fl(v 2^-1074 * ck 2^K1) = fl(v * ck) * 2^-K2 and the second product is
// fl(fl(v * ck) * rk), exactly.  Two conditions on the split, both checked over the committed tables by
// tests/test_exact_scaled_taps.py:
//   (1) every scaled tap is finite (largest: 2.1e300 as a column tap);
//   (2) every non-zero column product v 2^-1074 * ck 2^K1 is a normal number (smallest: 1.3e-28), so that its rounding
//       sees the same 53-bit significand as fl(v * ck).
// The scaling is an exact power-of-two multiply (ldexp).  The integer phase multiplies v by prod_fx / prod_fy directly
// (prod * 2^1074 overflows): it keeps the conversion and the unscaled tables.
constexpr int TAP_K1 = 1000, TAP_K2 = 74;
static_assert(TAP_K1 + TAP_K2 == 1074, "a byte in the low word of a zero register pair is byte * 2^-1074");
struct ExactTaps
{
    // the column taps are read at constant offsets from the struct: the tables indexed that way come first, within the
    // 2040 bytes an offset field of ds_read2_b64 reaches (further back every read pays an address add)
    double ctap[2][19][4]; // tap * 2^TAP_K1: column role, non-integer phases
    double tap[2][19][4];  // integer phase: only tap[0] is read at constant offsets
    double rtap[2][19][4]; // tap * 2^TAP_K2: row role, non-integer phases
    double prod[17][17][2];
};

// a pixel byte as the fp64 subnormal byte * 2^-1074: no conversion instruction, the high word is a constant zero
__device__ inline double byte_as_subnormal(int b)
{
    return __builtin_bit_cast(double, (unsigned long long)(unsigned)b);
}

__device__ inline void load_exact_taps(ExactTaps &L, const ToedTables *__restrict__ T)
{
    for (int t = threadIdx.x; t < 2 * 19 * 4; t += blockDim.x)
    {
        const int half = t / 76, k = (t % 76) / 4, d = t & 3;
        const double v = half ? T->tap_half[d][k] : T->tap_int[d][k];
        L.tap[half][k][d] = v;
        L.ctap[half][k][d] = ldexp(v, TAP_K1);
        L.rtap[half][k][d] = ldexp(v, TAP_K2);
    }
    for (int t = threadIdx.x; t < 17 * 17; t += blockDim.x)
    {
        const int p = t / 17, q = t % 17;
        L.prod[p][q][0] = T->prod_fx[p][q];
        L.prod[p][q][1] = T->prod_fy[p][q];
    }
    __syncthreads();
}

template <int SY, int SX>
__device__ inline void exact9(const uint8_t *__restrict__ img, int h, int w, const ExactTaps &L, int i, int j,
                              double f[9])
{
    constexpr bool IP = (SY == 0 && SX == 0);
    const double(*ck)[4] = IP ? L.tap[SX] : L.ctap[SX];
    const double(*rk)[4] = IP ? L.tap[SY] : L.rtap[SY];
#pragma unroll
    for (int r = 0; r < 9; ++r)
        f[r] = 0.0;
    constexpr int PM = IP ? 8 : 9;
    const bool fast = __all(window_inside(h, w, i, j));
    const ColMask cm = column_mask(w, j);
    Row24 nxt = fetch_row(img, h, w, i + PM, j);
#pragma unroll 1
    for (int p = -PM; p <= PM; ++p)
    {
        const Row24 cur = nxt;
        nxt = fetch_row(img, h, w, i - min(p + 1, PM), j); // next row in flight while this one is accumulated
        int vb[19];
        unsigned dw[5];
        if (IP)
            unpack_row(cur, h, i - p, cm, fast, vb);
        else
            mask_row(cur, h, i - p, cm, fast, dw);
        double rr[4];
#pragma unroll
        for (int d = 0; d < 4; ++d)
            rr[d] = rk[p + 9][d];
#pragma unroll
        for (int q = -PM; q <= PM; ++q)
        {
            const double v = IP ? (double)vb[q + 9] : byte_as_subnormal(row_tap(dw, q));
            // the column taps are re-read from LDS a few taps at a time: a laundered zero offset keeps the reads in the
            // row loop (hoisted, the 76 doubles would occupy 152 VGPRs and halve the occupancy)
            int lz = 0;
            if (((q + PM) & 3) == 0)
                asm volatile("" : "+v"(lz));
            const double(*ckl)[4] = ck + lz;
            double cc[4];
#pragma unroll
            for (int d = 0; d < 4; ++d)
                cc[d] = v * ckl[q + 9][d];
            if (IP)
            {
                f[0] += v * L.prod[p + 8][q + 8][0];
                f[1] += v * L.prod[p + 8][q + 8][1];
                f[2] += cc[2] * rr[0];
                f[3] += cc[1] * rr[1];
                f[4] += cc[0] * rr[2];
                f[5] += cc[2] * rr[1];
                f[6] += cc[1] * rr[2];
                f[7] += cc[3] * rr[0];
                f[8] += cc[0] * rr[3];
            }
            else
            {
                EBVO_ACCUM9(f, cc, rr)
            }
        }
    }
}

// gradient magnitude (fx, fy only) at interpolated pixel (I, J) of compile-time phase (SY, SX)
template <int SY, int SX>
__device__ inline double exact_mag(const uint8_t *__restrict__ img, int h, int w, const ExactTaps &L, int I, int J)
{
    constexpr bool IP = (SY == 0 && SX == 0);
    const int i = I >> 1, j = J >> 1;
    const double(*ck)[4] = IP ? L.tap[SX] : L.ctap[SX];
    const double(*rk)[4] = IP ? L.tap[SY] : L.rtap[SY];
    double fx = 0.0, fy = 0.0;
    constexpr int PM = IP ? 8 : 9;
    const bool fast = __all(window_inside(h, w, i, j));
    const ColMask cm = column_mask(w, j);
    Row24 nxt = fetch_row(img, h, w, i + PM, j);
#pragma unroll 1
    for (int p = -PM; p <= PM; ++p)
    {
        const Row24 cur = nxt;
        nxt = fetch_row(img, h, w, i - min(p + 1, PM), j);
        int vb[19];
        unsigned dw[5];
        if (IP)
            unpack_row(cur, h, i - p, cm, fast, vb);
        else
            mask_row(cur, h, i - p, cm, fast, dw);
        const double r0 = rk[p + 9][0], r1 = rk[p + 9][1];
        int lz = 0;
        asm volatile("" : "+v"(lz)); // keeps the column-tap reads in the row loop (see exact9)
        const double(*ckl)[4] = ck + lz;
#pragma unroll
        for (int q = -PM; q <= PM; ++q)
        {
            const double v = IP ? (double)vb[q + 9] : byte_as_subnormal(row_tap(dw, q));
            if (IP)
            {
                fx += v * L.prod[p + 8][q + 8][0];
                fy += v * L.prod[p + 8][q + 8][1];
            }
            else
            {
                fx += (v * ckl[q + 9][1]) * r0;
                fy += (v * ckl[q + 9][0]) * r1;
            }
        }
    }
    return sqrt(fx * fx + fy * fy);
}

#ifdef EBVO_WAVE_TRACE
// developer build only (make EXTRA=-DEBVO_WAVE_TRACE): where and when every wave of an exact kernel ran
__device__ unsigned long long g_wave_trace[2][8192 * 4];
__device__ inline void wave_trace(int which, int wave, unsigned long long t0, int tasks)
{
    if ((threadIdx.x & 63) == 0 && wave < 8192)
    {
        const unsigned hw = __builtin_amdgcn_s_getreg(4 | (0 << 6) | (31 << 11));  // HW_REG_HW_ID
        const unsigned xcc = __builtin_amdgcn_s_getreg(20 | (0 << 6) | (31 << 11)); // HW_REG_XCC_ID
        unsigned long long *o = g_wave_trace[which] + (size_t)wave * 4;
        o[0] = t0;
        o[1] = __builtin_amdgcn_s_memrealtime();
        o[2] = ((unsigned long long)xcc << 32) | hw;
        o[3] = (unsigned long long)tasks;
    }
}
extern "C" int ebvo_wave_trace_read(int which, unsigned long long *dst, int n_waves)
{
    return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_wave_trace), (size_t)n_waves * 32, (size_t)which * 8192 * 32,
                                    hipMemcpyDeviceToHost);
}
#define EBVO_TRACE_BEGIN() const unsigned long long trace_t0 = __builtin_amdgcn_s_memrealtime(); int trace_n = 0
#define EBVO_TRACE_TASK() ++trace_n
#define EBVO_TRACE_END(which) wave_trace(which, wave, trace_t0, trace_n)
#else
#define EBVO_TRACE_BEGIN()
#define EBVO_TRACE_TASK()
#define EBVO_TRACE_END(which)
#endif

// Work distribution of the two exact kernels.  The (phase, image) lists are cut into runs of 64 entries -- one run is one
// wave's worth of work, and every run of a kernel costs the same -- and the runs are dealt round-robin to the waves of a
// launch that holds exactly as many blocks as the chip keeps resident: at KITTI size every SIMD receives four runs of
// exact_centre (tools/gpu_wave_trace.py: 1013 SIMDs with 4 runs, 11 with 3).  A grid sized for the list CAPACITY put the
// runs into the first half of the blocks of each (image, phase) slice and left the second half of every slice empty:
// 102.7 -> 90.6 us (centre), 82.8 -> 65.3 us (mags).  The counts live on the device, so every wave walks the (at
// most 8) list lengths itself; all of it is wave-uniform scalar work.
struct ExactTask
{
    int im, ph, k0, n;
};

__device__ inline bool exact_task(const ExactBatch &E, int n_img, int cap, int list0, int t, ExactTask &o)
{
    int base = 0;
    for (int ph = 0; ph < 4; ++ph)
        for (int im = 0; im < n_img; ++im)
        {
            const int n = min(E.lcount[im][list0 + ph], cap);
            const int c = (n + 63) >> 6;
            if (t < base + c)
            {
                o.im = im;
                o.ph = ph;
                o.k0 = (t - base) << 6;
                o.n = n;
                return true;
            }
            base += c;
        }
    return false;
}

template <int SY, int SX>
__device__ inline void centre_run(const ExactBatch &E, const ExactTaps &L, int h, int w, int cap, int im, int k, int n)
{
    const int W2 = 2 * w, H2 = 2 * h, wpr = (W2 + 31) >> 5;
    constexpr int PH = (SY << 1) | SX;
    const int32_t *__restrict__ list = E.lists[im] + (size_t)PH * cap;
    CandExact *__restrict__ cd = E.cd[im];
    const uint8_t *__restrict__ flag = E.flag[im];
    if (k < n)
    {
        const int t = list[k];
        const int o = E.src[im][2 * t];
        const int I = o / W2, J = o - I * W2;
        double f[9];
        exact9<SY, SX>(E.img[im], h, w, L, I >> 1, J >> 1, f);
        const double gx = f[0], gy = f[1];
        const double m = sqrt(gx * gx + gy * gy); // src/toed/cpu_toed.cpp:222
        NmsSector S;
        int packed = -1;
        if (nms_sector(m, gx, gy, S))
        {
            packed = (S.a1 + 1) | ((S.b1 + 1) << 2) | ((S.a2 + 1) << 4) | ((S.b2 + 1) << 6);
#pragma unroll
            for (int q = 0; q < 4; ++q)
            {
                const int da = (q & 2) ? S.a2 : S.a1, db = (q & 2) ? S.b2 : S.b1;
                const int nI = (q & 1) ? I - da : I + da, nJ = (q & 1) ? J - db : J + db;
                const int no = nI * W2 + nJ;
                // a neighbour that is a candidate itself gets its |g| from its own thread (flags exist only inside
                // the screened interior)
                const bool is_cand = nI >= 10 && nI < H2 - 10 && nJ >= 10 && nJ < W2 - 10 && flag[no] == 1;
                if (!is_cand) // fire-and-forget: rows are counted from the bitmap afterwards (toed_need_count_kernel)
                    atomicOr(&E.needbits[im][(size_t)nI * wpr + (nJ >> 5)], 1u << (nJ & 31));
            }
        }
        CandExact r;
        r.gx = gx;
        r.gy = gy;
        r.m = m;
        third_order_dir(f, r.tox, r.toy);
        r.sector = packed;
        r.pad0 = 0;
        r.pad1[0] = r.pad1[1] = 0.0;
        cd[t] = r; // the whole line
        E.magmap[im][mag_index(I, J, W2)] = m;
    }
}

// S3b: exact centre of every candidate; early NMS rejects; marks the grid points whose exact |g| the NMS of the
// candidate needs.  Adjacent candidates along a contour share two of their four neighbours and 14 % of the
// neighbours are candidates themselves (whose |g| is computed right here): marking every distinct point once in a
// bitmap (no-return atomicOr; one row of the bitmap per grid row) leaves 54 % of the neighbour evaluations.
#ifndef EBVO_CENTRE_WPS
#define EBVO_CENTRE_WPS 0 // tuning macro: waves per SIMD the centre kernel is compiled for (0 = what its registers allow: 4)
#endif
#if EBVO_CENTRE_WPS > 0
__global__ __launch_bounds__(256, EBVO_CENTRE_WPS) void toed_exact_centre_kernel(ExactBatch E, const ToedTables *__restrict__ T, int h,
#else
__global__ __launch_bounds__(256) void toed_exact_centre_kernel(ExactBatch E, const ToedTables *__restrict__ T, int h,
#endif
                                                                int w, int cap, int n_img)
{
    __shared__ ExactTaps L;
    EBVO_TRACE_BEGIN();
    load_exact_taps(L, T);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    ExactTask q;
    // (Round 4 tried to deal the runs by phase and SIMD -- five 289-tap runs cost what four 361-tap runs cost -- through two
    // run queues: the thousands of same-address atomics of a launch serialise at ~18 ns each across the XCDs, 100 -> 282 us.
    // DESIGN.md 6c.  The runs are dealt round-robin.)
    for (int t = wave; exact_task(E, n_img, cap, 0, t, q); t += gridDim.x * 4)
    {
        EBVO_TRACE_TASK();
        switch (q.ph)
        {
        case 0: centre_run<0, 0>(E, L, h, w, cap, q.im, q.k0 + lane, q.n); break;
        case 1: centre_run<0, 1>(E, L, h, w, cap, q.im, q.k0 + lane, q.n); break;
        case 2: centre_run<1, 0>(E, L, h, w, cap, q.im, q.k0 + lane, q.n); break;
        default: centre_run<1, 1>(E, L, h, w, cap, q.im, q.k0 + lane, q.n); break;
        }
    }
    EBVO_TRACE_END(0);
}

// S3c: the four neighbour magnitudes of every candidate of one (phase, axis) class.  The axis neighbours
// (+-a1, +-b1) share one phase, the diagonal neighbours (+-a2, +-b2) the opposite phase (SY^1, SX^1);
// PAIR selects which two a thread evaluates, so a launch slice has one phase throughout.
// S3c-0: marked points per grid row, even / odd columns (one wave per row)
__global__ __launch_bounds__(256) void toed_need_count_kernel(ExactBatch E, int h, int w)
{
    const int W2 = 2 * w, H2 = 2 * h, wpr = (W2 + 31) >> 5;
    const int im = blockIdx.y, I = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (I >= H2)
        return;
    const uint32_t *__restrict__ row = E.needbits[im] + (size_t)I * wpr;
    int ne = 0, no = 0;
    for (int k = lane; k < wpr; k += 64)
    {
        const uint32_t v = row[k];
        ne += __popc(v & 0x55555555u);
        no += __popc(v & 0xaaaaaaaau);
    }
    for (int d = 32; d > 0; d >>= 1)
    {
        ne += __shfl_down(ne, d);
        no += __shfl_down(no, d);
    }
    if (lane == 0)
    {
        E.need_cnt[im][I] = ne;
        E.need_cnt[im][H2 + I] = no;
    }
}

// S3c-1: one WAVE per grid row: the marked points of the row, in column order, into the list of their phase.  The row's
// offsets in the two lists (even / odd columns) of its row parity are the marked points of the rows of that parity in front
// of it -- added up here by the wave itself from toed_need_count_kernel's per-row counts (round 3: a scan launch of one
// block per image between the two).  The waves of the last two rows (one per row parity) also publish the list lengths,
// lcount[4..7], and add them to counts[3] (diagnostics: distinct neighbour points; zeroed by toed_compact_phase_kernel).
// Round 7: word-wise, like toed_compact_phase_kernel: a lane owns one 32-bit word of the row's bitmap (a turn = 2048
// columns), counts its even and odd bits, takes the packed wave scan and walks its set bits in column order.  No LDS, no
// barrier.  (Before: a block per row, one bit per lane, two barriers and an LDS round trip per 256 columns.)
__global__ __launch_bounds__(256) void toed_need_compact_kernel(ExactBatch E, int h, int w, int cap)
{
    const int W2 = 2 * w, H2 = 2 * h, wpr = (W2 + 31) >> 5;
    const int im = blockIdx.y, lane = threadIdx.x & 63;
    const int I = __builtin_amdgcn_readfirstlane((int)blockIdx.x * 4 + (int)(threadIdx.x >> 6));
    if (I >= H2)
        return;
    const int32_t *__restrict__ cnt = E.need_cnt[im];
    const bool last = I >= H2 - 2; // wave-uniform
    const int mine0 = cnt[I], mine1 = cnt[H2 + I];
    if (!last && mine0 + mine1 == 0)
        return;
    const uint32_t *__restrict__ bits = E.needbits[im] + (size_t)I * wpr;
    int a[4] = {0, 0, 0, 0}; // [2], [3] stay zero: the rows of the other parity feed other lists
    for (int r = (I & 1) + 2 * lane; r < I; r += 128)
    {
        a[0] += cnt[r];
        a[1] += cnt[H2 + r];
    }
    wave_sum4(a);
    int base_e = a[0], base_o = a[1];
    if (last && lane == 0)
    {
        const int n0 = base_e + mine0, n1 = base_o + mine1;
        E.lcount[im][4 + 2 * (I & 1) + 0] = n0; // phase (row parity I & 1, column parity 0)
        E.lcount[im][4 + 2 * (I & 1) + 1] = n1;
        atomicAdd(const_cast<int32_t *>(E.counts[im]) + 3, n0 + n1);
    }
    if (mine0 + mine1 == 0)
        return;
    int32_t *__restrict__ list_e = E.lists[im] + (size_t)(4 + ((I & 1) << 1)) * cap; // the list of the odd columns follows it
    for (int k0 = 0; k0 < wpr; k0 += 64)
    {
        const int k = k0 + lane;
        unsigned v = k < wpr ? bits[k] : 0u;
        if (W2 - 32 * k < 32) // the row's last word (or past it): columns >= 2W do not exist
            v &= W2 - 32 * k > 0 ? (1u << (W2 - 32 * k)) - 1u : 0u;
        unsigned total;
        const unsigned front = wave_excl_scan_pair((unsigned)__popc(v & 0x55555555u) | ((unsigned)__popc(v & 0xaaaaaaaau) << 16), total);
        int p_e = base_e + (int)(front & 0xffffu), p_o = base_o + (int)(front >> 16);
        const int o0 = I * W2 + 32 * k;
        walk_set_bits(v, [&](int b) {
            const int par = b & 1, pos = par ? p_o : p_e;
            if (pos < cap)
                list_e[pos + (cap & -par)] = o0 + b;
            p_o += par;
            p_e += par ^ 1;
        });
        base_e += (int)(total & 0xffffu);
        base_o += (int)(total >> 16);
    }
}

// S3c-3: exact |g| at every marked grid point, one thread per point, runs of 64 points dealt to the waves (exact_task)
template <int SY, int SX>
__device__ inline void mags_run(const ExactBatch &E, const ExactTaps &L, int h, int w, int cap, int im, int k, int n)
{
    const int W2 = 2 * w;
    constexpr int PH = (SY << 1) | SX;
    const int32_t *__restrict__ list = E.lists[im] + (size_t)(4 + PH) * cap;
    if (k < n)
    {
        const int o = list[k];
        const int I = o / W2, J = o - I * W2;
        E.magmap[im][mag_index(I, J, W2)] = exact_mag<SY, SX>(E.img[im], h, w, L, I, J);
    }
}

__global__ __launch_bounds__(256) void toed_exact_mags_kernel(ExactBatch E, const ToedTables *__restrict__ T, int h,
                                                              int w, int cap, int n_img)
{
    __shared__ ExactTaps L;
    EBVO_TRACE_BEGIN();
    load_exact_taps(L, T);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    ExactTask q;
    for (int t = wave; exact_task(E, n_img, cap, 4, t, q); t += gridDim.x * 4)
    {
        EBVO_TRACE_TASK();
        switch (q.ph)
        {
        case 0: mags_run<0, 0>(E, L, h, w, cap, q.im, q.k0 + lane, q.n); break;
        case 1: mags_run<0, 1>(E, L, h, w, cap, q.im, q.k0 + lane, q.n); break;
        case 2: mags_run<1, 0>(E, L, h, w, cap, q.im, q.k0 + lane, q.n); break;
        default: mags_run<1, 1>(E, L, h, w, cap, q.im, q.k0 + lane, q.n); break;
        }
    }
    EBVO_TRACE_END(1);
}

// S3d: the exact NMS decision of every candidate, from exact values only.  A block takes CHUNKS of 256 consecutive candidates
// and leaves, besides every candidate's record and flags, the chunk's number of maxima and of kept maxima: the ranks of the
// edges then need no scan over the 264 k flags (two launches per pair in round 3) -- toed_cand_scatter_kernel adds up the
// counts of the chunks in front of its own (at most a few hundred pairs of ints, every block for itself).
__global__ __launch_bounds__(256) void toed_exact_decide_kernel(ExactBatch E, int h, int w, int cap)
{
    __shared__ int s_cnt[4][2];
    const int im = blockIdx.y, W2 = 2 * w;
    const CandExact *__restrict__ cd = E.cd[im];
    CandRec *__restrict__ rec = E.rec[im];
    int32_t *__restrict__ ft = E.cand_flag[im], *__restrict__ fk = ft + cap;
    const int n = min(E.counts[im][2], cap);
    for (int c = blockIdx.x; c * 256 < n; c += gridDim.x)
    {
        const int t = c * 256 + threadIdx.x;
        bool is_max = false;
        int kept = 0;
        if (t < n)
        {
            const int o = E.src[im][2 * t];
            const int I = o / W2, J = o - I * W2;
            const CandExact ce = cd[t];
            const double gx = ce.gx, gy = ce.gy, m = ce.m;
            NmsSector S;
            double px = 0, py = 0, sm = 0;
            if (ce.sector >= 0 && nms_sector(m, gx, gy, S))
            {
                const double *__restrict__ mm = E.magmap[im];
                is_max = nms_finish(m, S, I, J, mm[mag_index(I + S.a1, J + S.b1, W2)], mm[mag_index(I + S.a2, J + S.b2, W2)],
                                    mm[mag_index(I - S.a1, J - S.b1, W2)], mm[mag_index(I - S.a2, J - S.b2, W2)], px, py, sm);
            }
            CandRec r;
            r.x = r.y = r.smag = 0.0;
            r.tox = ce.tox;
            r.toy = ce.toy;
            if (is_max)
            {
                r.x = (px - 1) / 2; // :538,542
                r.y = (py - 1) / 2;
                r.smag = sm;
                kept = (r.x > 10 && r.x < w - 10 && r.y > 10 && r.y < h - 10) ? 1 : 0; // :553-554
            }
            rec[t] = r;
            ft[t] = is_max ? 1 : 0;
            fk[t] = kept;
        }
        const unsigned long long bm = __ballot(is_max), bk = __ballot(kept != 0);
        if ((threadIdx.x & 63) == 0)
        {
            s_cnt[threadIdx.x >> 6][0] = __popcll(bm);
            s_cnt[threadIdx.x >> 6][1] = __popcll(bk);
        }
        __syncthreads();
        if (threadIdx.x == 0)
            E.chunk_cnt[im][c] = make_int2(s_cnt[0][0] + s_cnt[1][0] + s_cnt[2][0] + s_cnt[3][0],
                                           s_cnt[0][1] + s_cnt[1][1] + s_cnt[2][1] + s_cnt[3][1]);
        __syncthreads();
    }
}


// Audit (ebvo_toed_screen_audit): max |screen - exact| of gx, gy, |g| over the candidates, and of |g| over the distinct
// neighbour points that lie inside the screened interior -- the quantities the error budget above bounds.  Non-negative
// doubles order like their bit patterns, so the maxima are integer atomicMax on out[0..3]; out[4] counts the candidates
// whose exact sector differs from the screen's unambiguous reading (none may, by the budget), out[5] the candidates audited.
__global__ __launch_bounds__(256) void toed_screen_audit_kernel(ExactBatch E, ScreenDiag D, int h, int w, int cap, int im,
                                                                unsigned long long *out)
{
    const int W2 = 2 * w, H2 = 2 * h;
    const size_t plane = (size_t)H2 * W2;
    const float *__restrict__ dp = D.plane[im];
    const int n = min(E.counts[im][2], cap);
    double e[4] = {0, 0, 0, 0};
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n; t += gridDim.x * blockDim.x)
    {
        const int o = E.src[im][2 * t];
        const CandExact ce = E.cd[im][t];
        e[0] = fmax(e[0], fabs((double)dp[o] - ce.gx));
        e[1] = fmax(e[1], fabs((double)dp[plane + o] - ce.gy));
        e[2] = fmax(e[2], fabs((double)dp[2 * plane + o] - ce.m));
    }
    for (int ph = 0; ph < 4; ++ph)
    {
        const int32_t *__restrict__ list = E.lists[im] + (size_t)(4 + ph) * cap;
        const int np = min(E.lcount[im][4 + ph], cap);
        for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < np; k += gridDim.x * blockDim.x)
        {
            const int o = list[k];
            const int I = o / W2, J = o - I * W2;
            if (I >= 10 && I < H2 - 10 && J >= 10 && J < W2 - 10) // the screen decides (and the audit planes hold) these only
                e[3] = fmax(e[3], fabs((double)dp[2 * plane + o] - E.magmap[im][mag_index(I, J, W2)]));
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (e[k] > 0)
            atomicMax(&out[k], (unsigned long long)__double_as_longlong(e[k]));
    if (blockIdx.x == 0 && threadIdx.x == 0)
        out[5] = (unsigned long long)n;
}

// S4 ---------------------------------------------------------------------------------------
// write the edge records at their ranks (raster order is the candidate order).  The rank of a candidate = the maxima (kept
// maxima) of the chunks in front of its chunk -- summed here by every block for itself from toed_exact_decide_kernel's chunk
// counts -- plus those in front of it inside the chunk (ballots).
__global__ __launch_bounds__(256) void toed_cand_scatter_kernel(ImgBatch B, int cap)
{
    __shared__ int s_base[4][2], s_in[4][2];
    const CandRec *__restrict__ rec = B.rec[blockIdx.y];
    const int32_t *__restrict__ ftp = B.cand_flag[blockIdx.y], *__restrict__ fkp = ftp + cap;
    const int2 *__restrict__ chunk_cnt = reinterpret_cast<const int2 *>(B.cand_off[blockIdx.y]);
    ebvo_edge *__restrict__ edges = B.edges[blockIdx.y];
    double *__restrict__ all4 = B.all4[blockIdx.y];
    int32_t *counts = B.counts[blockIdx.y];
    const int n = min(counts[2], cap);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (n == 0 && blockIdx.x == 0 && threadIdx.x == 0)
    {
        counts[0] = 0;
        counts[1] = 0;
    }
    for (int c = blockIdx.x; c * 256 < n; c += gridDim.x)
    {
        int a0 = 0, a1 = 0;
        for (int k = threadIdx.x; k < c; k += 256)
        {
            const int2 v = chunk_cnt[k];
            a0 += v.x;
            a1 += v.y;
        }
        for (int d = 32; d > 0; d >>= 1)
        {
            a0 += __shfl_down(a0, d);
            a1 += __shfl_down(a1, d);
        }
        const int t = c * 256 + threadIdx.x;
        const int f_t = t < n ? ftp[t] : 0, f_k = t < n ? fkp[t] : 0;
        const unsigned long long bm = __ballot(f_t != 0), bk = __ballot(f_k != 0);
        if (lane == 0)
        {
            s_base[wid][0] = a0;
            s_base[wid][1] = a1;
            s_in[wid][0] = __popcll(bm);
            s_in[wid][1] = __popcll(bk);
        }
        __syncthreads();
        int o_t = s_base[0][0] + s_base[1][0] + s_base[2][0] + s_base[3][0];
        int o_k = s_base[0][1] + s_base[1][1] + s_base[2][1] + s_base[3][1];
        for (int k = 0; k < wid; ++k)
        {
            o_t += s_in[k][0];
            o_k += s_in[k][1];
        }
        const unsigned long long below = (1ull << lane) - 1ull;
        o_t += __popcll(bm & below);
        o_k += __popcll(bk & below);
        __syncthreads(); // (s_base / s_in are rewritten by the block's next chunk)
        if (t >= n)
            continue;
        if (t == n - 1)
        {
            counts[0] = o_t + f_t; // Total_Num_Of_TOED
            counts[1] = o_k + f_k; // toed_edges.size()
        }
        if (!f_t || (!all4 && !f_k)) // (the resident pipeline keeps no subpix_edge_pts_final, see toed_enqueue)
            continue;
        const CandRec r = rec[t];
        double TO_Ix = r.tox, TO_Iy = r.toy; // src/toed/cpu_toed.cpp:226-229
        const double TO_mag = sqrt(TO_Ix * TO_Ix + TO_Iy * TO_Iy);
        TO_Ix /= TO_mag;
        TO_Iy /= TO_mag;
        const double th = ebvo_atan2(TO_Ix, -TO_Iy);
        if (all4)
        {
            const int ra = o_t;
            all4[(size_t)ra * 4 + 0] = r.x;
            all4[(size_t)ra * 4 + 1] = r.y;
            all4[(size_t)ra * 4 + 2] = th;
            all4[(size_t)ra * 4 + 3] = r.smag;
        }
        if (f_k)
        {
            ebvo_edge e;
            e.x = r.x;
            e.y = r.y;
            e.theta = th;
            e.index = o_k;
            e.pad = 0;
            edges[e.index] = e;
        }
    }
}

} // namespace

int toed_init_constants(ebvo_ctx *ctx)
{
    static ToedTables host;
    memcpy(host.tap_int, h_TAP_INT, sizeof(h_TAP_INT));
    memcpy(host.tap_half, h_TAP_HALF, sizeof(h_TAP_HALF));
    for (int p = -8; p <= 8; ++p)
        for (int q = -8; q <= 8; ++q)
        {
            host.prod_fx[p + 8][q + 8] = h_TAP_INT[1][q + 9] * h_TAP_INT[0][p + 9];
            host.prod_fy[p + 8][q + 8] = h_TAP_INT[0][q + 9] * h_TAP_INT[1][p + 9];
        }
    // FP32 screen: the constant its recentred pixels leave out, per phase; row / column tap ranges as the kernel uses them
    // (phase (0, 0): 17 integer taps both ways; otherwise 19 taps, the half-pixel table along a shifted axis)
    for (int sy = 0; sy < 2; ++sy)
        for (int sx = 0; sx < 2; ++sx)
        {
            const int pm = (sy == 0 && sx == 0) ? 8 : 9;
            const double(*xt)[19] = sx ? h_TAP_HALF : h_TAP_INT, (*yt)[19] = sy ? h_TAP_HALF : h_TAP_INT;
            double sxg = 0, sxgx = 0, syg = 0, sygx = 0;
            for (int q = -pm; q <= pm; ++q)
            {
                sxg += xt[0][q + 9];
                sxgx += xt[1][q + 9];
                syg += yt[0][q + 9];
                sygx += yt[1][q + 9];
            }
            host.screen_dc[(sy << 1) | sx][0] = (float)(127.5 * sxgx * syg); // gx: Gx along x, G along y
            host.screen_dc[(sy << 1) | sx][1] = (float)(127.5 * sxg * sygx); // gy: G along x, Gx along y
        }
    if (ctx->device < 0 || ctx->device >= 16)
        return EBVO_ERR_ARG;
    if (!g_tables_dev[ctx->device])
    {
        ToedTables *d = nullptr;
        EBVO_HIP(ctx, hipMalloc(&d, sizeof(ToedTables)));
        EBVO_HIP(ctx, hipMemcpy(d, &host, sizeof(ToedTables), hipMemcpyHostToDevice));
        g_tables_dev[ctx->device] = d; // lives for the process; shared by every ctx on the device
    }
    return EBVO_OK;
}

// blocks of 256 threads the device keeps resident at once for the exact kernels (CUs x blocks per CU): their launches
// are exactly that large, see exact_task
static int resident_blocks(ebvo_ctx *ctx, int which)
{
    if (ctx->exact_blocks[which] > 0)
        return ctx->exact_blocks[which];
    // (two host threads with their own contexts may get here together: the value they compute is the same, the store is atomic)
    static std::atomic<int> cached[16][2];
    std::atomic<int> &slot = cached[ctx->device & 15][which];
    int c = slot.load(std::memory_order_relaxed);
    if (c == 0)
    {
        int per_cu = 0, cus = 0;
        if (which == 0)
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, toed_exact_centre_kernel, 256, 0);
        else
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, toed_exact_mags_kernel, 256, 0);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, ctx->device);
        c = (per_cu > 0 ? per_cu : 4) * (cus > 0 ? cus : 256);
        slot.store(c, std::memory_order_relaxed);
    }
    return c;
}

// where the audit of image k of the slot leaves its 8 words: behind the three audit planes
unsigned long long *toed_screen_audit_result(Slot &s, int k, int h, int w)
{
    const int H2 = 2 * h, W2 = 2 * w;
    const int need_words = H2 * ((W2 + 31) / 32);
    float *planes = (float *)((int32_t *)(s.im[k].maps + mag_map_doubles(H2, W2)) + need_words + 4 * H2);
    return (unsigned long long *)(planes + 3 * (size_t)H2 * W2);
}

void toed_screen_budget(double out[5])
{
    out[0] = SCREEN_E_G;
    out[1] = SCREEN_E_M;
    out[2] = SCREEN_E_S;
    out[3] = SCREEN_TOL_M;
    out[4] = SCREEN_TOL_S;
}

int toed_enqueue(ebvo_ctx *ctx, Slot &s, int n_img, int h, int w, hipEvent_t ev_conv_begin, hipEvent_t ev_conv_end,
                 hipEvent_t ev_end, int mode, bool want_all4)
{
    if (n_img < 1 || n_img > MAX_BATCH)
        return EBVO_ERR_ARG;
    if (mode < 0)
        mode = ctx->toed_mode;
    const int H2 = 2 * h, W2 = 2 * w;
    const int need_words = H2 * ((W2 + 31) / 32); // one bitmap row per grid row
    ImgBatch B{};
    for (int k = 0; k < n_img; ++k)
    {
        ImageWS &ws = s.im[k];
        B.img[k] = ws.img;
        B.maps[k] = ws.maps;
        B.flag[k] = ws.flag;
        B.row_cnt[k] = ws.row_cnt;
        B.row_off[k] = ws.row_off;
        B.counts[k] = ws.counts;
        B.src[k] = ws.src;
        B.edges[k] = ws.edges;
        B.all4[k] = want_all4 ? ws.all4 : nullptr; // subpix_edge_pts_final (every maximum, 32 B each): host-buffer calls only
        B.rec[k] = (CandRec *)ws.cand_rec;
        B.cand_flag[k] = ws.cand_flag;
        B.cand_off[k] = ws.cand_off;
        B.lists[k] = ws.cand_lists;
        B.lcount[k] = ws.cand_lcount;
    }
    {
        // per-row counters of every image: one launch
        int32_t *ptrs[2 * MAX_BATCH];
        int counts[2 * MAX_BATCH];
        int nc = 0;
        for (int k = 0; k < n_img; ++k)
        {
            ptrs[nc] = s.im[k].row_cnt;
            counts[nc++] = 2 * H2;
            if (mode == EBVO_TOED_HYBRID)
            {
                // need bitmap + its per-row counters live behind the |g| map in the (otherwise unused) plane buffer
                ptrs[nc] = (int32_t *)(s.im[k].maps + mag_map_doubles(H2, W2));
                counts[nc++] = need_words; // the per-row counters behind it are written by toed_need_count_kernel
            }
        }
        int rc = ebvo_clear_enqueue(ctx, s, ptrs, counts, nc);
        if (rc)
            return rc;
    }
    if (mode == EBVO_TOED_HYBRID)
    {
        const int cap = ctx->cap_edges;
        ScreenDiag D{};
        if (ev_conv_begin)
            EBVO_HIP(ctx, hipEventRecord(ev_conv_begin, s.stream));
        {
            ProfScope ps(ctx, s, K_NMS);
            const dim3 ftiles((w + FT_W - 1) / FT_W, (h + FT_H - 1) / FT_H, n_img);
            if (ctx->screen_audit)
            {
                // audit planes: behind the need bitmap and its counters in the plane buffer (free in hybrid mode)
                for (int k = 0; k < n_img; ++k)
                    D.plane[k] = (float *)((int32_t *)(s.im[k].maps + mag_map_doubles(H2, W2)) + need_words + 4 * H2);
                hipLaunchKernelGGL(toed_screen_fused_kernel<true>, ftiles, dim3(256), 0, s.stream, B,
                                   (const ToedTables *)g_tables_dev[ctx->device], h, w, D);
            }
            else
                hipLaunchKernelGGL(toed_screen_fused_kernel<false>, ftiles, dim3(256), 0, s.stream, B,
                                   (const ToedTables *)g_tables_dev[ctx->device], h, w, D);
        }
        const int stop = ctx->stop_stage; // developer key 16
        if (stop == 1)
            return EBVO_OK;
        {
            ProfScope ps(ctx, s, K_COMPACT);
            hipLaunchKernelGGL(toed_compact_phase_kernel, dim3((H2 - 20 + 3) / 4, n_img), dim3(256), 0, s.stream, B, h, w, cap);
        }
        if (stop == 2)
            return EBVO_OK;
        {
            ExactBatch E{};
            for (int k = 0; k < n_img; ++k)
            {
                ImageWS &ws = s.im[k];
                E.img[k] = ws.img;
                E.src[k] = ws.src;
                E.counts[k] = ws.counts;
                E.lists[k] = ws.cand_lists;
                E.lcount[k] = ws.cand_lcount;
                E.cd[k] = (CandExact *)ws.cand_data; // one 64-byte record per candidate
                E.rec[k] = (CandRec *)ws.cand_rec;
                E.cand_flag[k] = ws.cand_flag;
                E.chunk_cnt[k] = reinterpret_cast<int2 *>(ws.cand_off);
                // the planes of the strict path are free in hybrid mode: |g| map, need bitmap, per-row counters
                E.flag[k] = ws.flag;
                E.magmap[k] = ws.maps;
                E.needbits[k] = (uint32_t *)(ws.maps + mag_map_doubles(H2, W2));
                E.need_cnt[k] = (int32_t *)(E.needbits[k] + need_words);
            }
            const ToedTables *T = (const ToedTables *)g_tables_dev[ctx->device];
            {
                hipEvent_t k_begin, k_end; // the dominant kernel: timed by its own dispatch when the profiler is on
                if (ebvo_prof_kernel(ctx, s, K_EXACT_CENTRE, &k_begin, &k_end))
                    hipExtLaunchKernelGGL(toed_exact_centre_kernel, dim3(resident_blocks(ctx, 0)), dim3(256), 0, s.stream,
                                          k_begin, k_end, 0, E, T, h, w, cap, n_img);
                else
                    hipLaunchKernelGGL(toed_exact_centre_kernel, dim3(resident_blocks(ctx, 0)), dim3(256), 0, s.stream, E,
                                       T, h, w, cap, n_img);
                if (ctx->repeat_mask & 1)
                    hipLaunchKernelGGL(toed_exact_centre_kernel, dim3(resident_blocks(ctx, 0)), dim3(256), 0, s.stream, E,
                                       T, h, w, cap, n_img);
            }
            if (stop == 3)
                return EBVO_OK;
            {
                ProfScope ps(ctx, s, K_COMPACT); // the lists of the distinct neighbour points
                hipLaunchKernelGGL(toed_need_count_kernel, dim3((H2 + 3) / 4, n_img), dim3(256), 0, s.stream, E, h, w);
                hipLaunchKernelGGL(toed_need_compact_kernel, dim3((H2 + 3) / 4, n_img), dim3(256), 0, s.stream, E, h, w, cap);
            }
            if (stop == 4)
                return EBVO_OK;
            {
                ProfScope ps(ctx, s, K_EXACT_MAGS);
                hipLaunchKernelGGL(toed_exact_mags_kernel, dim3(resident_blocks(ctx, 1)), dim3(256), 0, s.stream, E, T, h,
                                   w, cap, n_img);
                if (ctx->repeat_mask & 2)
                    hipLaunchKernelGGL(toed_exact_mags_kernel, dim3(resident_blocks(ctx, 1)), dim3(256), 0, s.stream, E, T, h,
                                       w, cap, n_img);
                if (stop == 5)
                    return EBVO_OK;
                hipLaunchKernelGGL(toed_exact_decide_kernel, dim3(512 / (ctx->small_div > 0 ? ctx->small_div : 4), n_img), dim3(256), 0, s.stream, E, h, w, cap);
            }
            if (stop == 6)
                return EBVO_OK;
            if (ctx->screen_audit)
                for (int k = 0; k < n_img; ++k)
                {
                    unsigned long long *out = toed_screen_audit_result(s, k, h, w);
                    EBVO_HIP(ctx, hipMemsetAsync(out, 0, 8 * sizeof(unsigned long long), s.stream));
                    hipLaunchKernelGGL(toed_screen_audit_kernel, dim3(512), dim3(256), 0, s.stream, E, D, h, w, cap, k, out);
                }
        }
        if (ev_conv_end)
            EBVO_HIP(ctx, hipEventRecord(ev_conv_end, s.stream));
        {
            ProfScope ps(ctx, s, K_FINALIZE);
            hipLaunchKernelGGL(toed_cand_scatter_kernel, dim3(512 / (ctx->small_div > 0 ? ctx->small_div : 4), n_img), dim3(256), 0, s.stream, B, cap);
        }
        if (ev_end)
            EBVO_HIP(ctx, hipEventRecord(ev_end, s.stream));
        EBVO_HIP(ctx, hipGetLastError());
        return EBVO_OK;
    }
    if (ev_conv_begin)
        EBVO_HIP(ctx, hipEventRecord(ev_conv_begin, s.stream));
    {
        ProfScope ps(ctx, s, K_CONV);
        dim3 grid((w + TILE_W - 1) / TILE_W, (h + TILE_H - 1) / TILE_H, 2 * n_img);
        hipLaunchKernelGGL(toed_conv_kernel, grid, dim3(256), 0, s.stream, B,
                           (const ToedTables *)g_tables_dev[ctx->device], h, w);
    }
    if (ev_conv_end)
        EBVO_HIP(ctx, hipEventRecord(ev_conv_end, s.stream));
    {
        ProfScope ps(ctx, s, K_NMS);
        dim3 grid((W2 - 20 + 63) / 64, (H2 - 20 + 3) / 4, n_img);
        hipLaunchKernelGGL(toed_nms_kernel, grid, dim3(64, 4), 0, s.stream, B, h, w);
    }
    {
        ProfScope ps(ctx, s, K_ROWSCAN);
        hipLaunchKernelGGL(toed_rowscan_kernel, dim3(n_img), dim3(64), 0, s.stream, B, H2, 0);
    }
    {
        ProfScope ps(ctx, s, K_COMPACT);
        hipLaunchKernelGGL(toed_compact_kernel, dim3(H2 - 20, n_img), dim3(256), 0, s.stream, B, h, w, ctx->cap_edges);
    }
    {
        ProfScope ps(ctx, s, K_FINALIZE);
        hipLaunchKernelGGL(toed_finalize_kernel, dim3(512, n_img), dim3(256), 0, s.stream, B, h, w, ctx->cap_edges);
    }
    if (ev_end)
        EBVO_HIP(ctx, hipEventRecord(ev_end, s.stream));
    EBVO_HIP(ctx, hipGetLastError());
    return EBVO_OK;
}
