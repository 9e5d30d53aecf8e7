/*
 * ebvo_gn6.h -- the 6-DoF Gauss-Newton step shared by the inlier refit (pose_refit_kernels.hip) and the edge alignment
 * (align_kernels.hip): the 6 x 6 Cholesky solve on the 28 sums and R <- Exp(w) R.  The operation order is part of both
 * arithmetic contracts (include/ebvo_hip.h).  fp64, -ffp-contract=off (no FMA), IEEE division and sqrt.
 */
#ifndef EBVO_GN6_H
#define EBVO_GN6_H

#include "ebvo_math.h"

#ifdef __HIPCC__
// H d = -g by Cholesky, the pivots in order; false when a pivot is not > 0.  Straight-line code (a failed pivot only clears
// the flag, what follows it is computed and dropped), so that L stays in registers.  S: the 28 sums, H(i, j) at upper(i, j).
__device__ static constexpr int upper(int i, int j)
{
    return i * 6 - (i * (i - 1)) / 2 + (j - i);
}
__device__ static inline bool refit_solve(const double *S, double *d)
{
    double L[6][6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; ++j)
    {
        double v = S[upper(j, j)];
#pragma unroll
        for (int k = 0; k < j; ++k)
            v = v - L[j][k] * L[j][k];
        ok = ok && v > 0;
        L[j][j] = sqrt(v);
#pragma unroll
        for (int i = j + 1; i < 6; ++i)
        {
            double e = S[upper(j, i)];
#pragma unroll
            for (int k = 0; k < j; ++k)
                e = e - L[i][k] * L[j][k];
            L[i][j] = e / L[j][j];
        }
    }
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; ++i)
    {
        double v = -S[21 + i];
#pragma unroll
        for (int k = 0; k < i; ++k)
            v = v - L[i][k] * y[k];
        y[i] = v / L[i][i];
    }
#pragma unroll
    for (int i = 5; i >= 0; --i)
    {
        double v = y[i];
#pragma unroll
        for (int k = i + 1; k < 6; ++k)
            v = v - L[k][i] * d[k];
        d[i] = v / L[i][i];
    }
    return ok;
}

__device__ static inline void mm3(const double *a, const double *b, double *o)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j)
            o[i * 3 + j] = (a[i * 3] * b[j] + a[i * 3 + 1] * b[3 + j]) + a[i * 3 + 2] * b[6 + j];
}

// R <- Exp(w) R (no re-orthonormalisation)
__device__ static inline void refit_rotate(const double *w, double *R)
{
    const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    if (th2 == 0)
        return;
    const double th = sqrt(th2);
    double sn, cs, sh, ch;
    ebvo_sincos(th, &sn, &cs);
    ebvo_sincos(th * 0.5, &sh, &ch);
    const double a = sn / th, b = (2.0 * (sh * sh)) / th2;
    const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    double W2[9], E[9], Rn[9];
    mm3(W, W, W2);
#pragma unroll
    for (int i = 0; i < 9; ++i)
        E[i] = ((i % 4 == 0 ? 1.0 : 0.0) + a * W[i]) + b * W2[i];
    mm3(E, R, Rn);
#pragma unroll
    for (int i = 0; i < 9; ++i)
        R[i] = Rn[i];
}
#endif

#endif /* EBVO_GN6_H */
