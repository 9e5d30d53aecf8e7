/*
 * ebvo_gn6.h -- the 6-DoF Gauss-Newton step shared by the inlier refit (pose_refit_kernels.hip) and the edge alignment
 * (align_kernels.hip): the 6 x 6 Cholesky solve on the 28 sums, R <- Exp(w) R and the decision that follows a step's sums;
 * and the fixed-tree reductions those two, the inverse-depth filter (depth_kernels.hip) and the depth carry
 * (carry_kernels.hip) form their sums and counts with.  The operation order is part of their arithmetic contracts
 * (include/ebvo_hip.h).  fp64, -ffp-contract=off (no FMA), IEEE division and sqrt.
 */
#ifndef EBVO_GN6_H
#define EBVO_GN6_H

#include <cstdint>

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

// What follows the 28 sums of step `it` of round `rnd`: keep or take back the last step, then solve and apply the next one.
// State (RefitState in LDS, AlignState in device memory): Rt, Pv (the pose before the last step), c_first, c_last, c_prev,
// status, stop, steps, go.  It sets st.go (0 ends the round) and returns the stop reason it wrote to st.stop -- 0 the step
// was below eps, 1 the last iteration, 2 the cost rose, 3 the solve failed -- or -1 when the round goes on.
template <class State>
__device__ static inline int gn6_decide(int rnd, int it, int iterations, double eps, const double *sums, State &st)
{
    const double cost = sums[27];
    st.go = 0;
    if (it == 0)
        st.c_first = cost;
    if (it > 0 && !(cost <= st.c_prev)) // the cost rose (a NaN counts as larger): back to the pose before
    {
#pragma unroll
        for (int i = 0; i < 12; ++i)
            st.Rt[i] = st.Pv[i];
        --st.steps;
        return st.stop = 2;
    }
    st.c_last = cost;
    if (it == iterations)
        return st.stop = 1;
    double d[6];
    if (!refit_solve(sums, d))
    {
        if (rnd == 0 && it == 0)
            st.status = 2;
        return st.stop = 3;
    }
    double Rt[12];
#pragma unroll
    for (int i = 0; i < 12; ++i)
        st.Pv[i] = Rt[i] = st.Rt[i];
    st.c_prev = cost;
    refit_rotate(d, Rt);
    double m = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
        Rt[9 + i] = Rt[9 + i] + d[3 + i];
#pragma unroll
    for (int i = 0; i < 6; ++i)
    {
        const double a = fabs(d[i]);
        if (a > m)
            m = a;
    }
#pragma unroll
    for (int i = 0; i < 12; ++i)
        st.Rt[i] = Rt[i];
    ++st.steps;
    if (m < eps)
        return st.stop = 0;
    st.go = 1;
    return -1;
}

// ---- the fixed-tree reductions of the pose kernels --------------------------------------------------------------------
// Their shapes are part of the same contracts (the sums must not depend on the launch geometry): 64 consecutive virtual
// lanes per wave, then the groups of a tile, then the tiles in ascending order from +0.0 (the callers' loops).

// x of every lane of a wave -> *slot by the halving tree x[l] += x[l + s], s = 32 .. 1 (lane 0 ends with it)
__device__ static inline void wave_sum(double x, int lane, double *slot)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
        x = x + __shfl_down(x, s);
    if (lane == 0)
        *slot = x;
}

// value v of GROUPS group slots (part[j * stride + v]) by the same tree, s = GROUPS / 2 .. 1
template <int GROUPS>
__device__ static inline double group_sum(const double *part, int stride, int v)
{
    double g[GROUPS];
#pragma unroll
    for (int j = 0; j < GROUPS; ++j)
        g[j] = part[j * stride + v];
#pragma unroll
    for (int s = GROUPS / 2; s >= 1; s >>= 1)
#pragma unroll
        for (int l = 0; l < s; ++l)
            g[l] = g[l] + g[l + s];
    return g[0];
}

// the sum of the integer c over the wave, then one atomic (every lane of the wave calls this)
__device__ static inline void wave_count(int c, int lane, int32_t *slot)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
        c += __shfl_down(c, s);
    if (lane == 0 && c)
        atomicAdd(slot, c);
}
#endif

#endif /* EBVO_GN6_H */
