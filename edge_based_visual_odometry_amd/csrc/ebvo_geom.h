/*
 * ebvo_geom.h -- the stereo geometry of one (left edge, right edge) pair, shared by the finalisation rows
 * (refine_kernels.hip: finalize_pairs_kernel), the pose search (pose_kernels.hip) and the temporal ground truth
 * (tgt_kernels.hip): Gamma from
 * Utility::backproject_2D_point_to_3D_point_using_rays and T from reconstruct_3D_Tangent_through_intersection_of_planes
 * (src/utility.cpp:95-112).  The calibration inverses are formed once on the host (Eigen's cofactor inverse, restated),
 * every product / cross / normalize in Eigen's fixed-size order.  Its second half is a keyframe mate under a relative pose:
 * the reprojection, its Jacobian rows, the Huber function, the image and liveness tests and the grid cell that the pose
 * refit, the edge alignment, the inverse-depth filter, the depth carry and the temporal ground truth share.
 * Compiled with -ffp-contract=off (no FMA).
 */
#ifndef EBVO_GEOM_H
#define EBVO_GEOM_H

#include "../../include/ebvo_hip.h"
#include "ebvo_math.h"

struct FinalCalib
{
    double Kli[9], Kri[9], R21[9], T21[3];
};

#ifdef __HIPCC__
__device__ static inline void mv3(const double *m, const double *v, double *o)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
        o[i] = (m[i * 3] * v[0] + m[i * 3 + 1] * v[1]) + m[i * 3 + 2] * v[2];
}
__device__ static inline void mtv3(const double *m, const double *v, double *o)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
        o[i] = (m[i] * v[0] + m[3 + i] * v[1]) + m[6 + i] * v[2];
}
__device__ static inline void cross3(const double *a, const double *b, double *o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ static inline double dot3(const double *a, const double *b)
{
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
// Eigen's normalize() / normalized(): unchanged when the squared norm is not positive
__device__ static inline void normalize3(double *v)
{
    const double z = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    if (z > 0)
    {
        const double n = sqrt(z);
        v[0] /= n;
        v[1] /= n;
        v[2] /= n;
    }
}

// Utility::project_3D_Tangent_to_2D_Tangent (src/utility.cpp:114-119): T - T.z * gamma, normalised
__device__ static inline void project_tangent3(const double *T, const double *g, double *p)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
        p[i] = T[i] - T[2] * g[i];
    normalize3(p);
}

// Gamma (3-D point, left camera) and T (unit 3-D tangent) of one pair; g1 / g2: the two rays K^-1 (x, y, 1)
__device__ static inline void stereo_gamma_tangent(const FinalCalib &C, const ebvo_edge &l, const ebvo_edge &r, double *G,
                                                   double *T, double *g1, double *g2)
{
    const double el[3] = {l.x, l.y, 1.0}, er[3] = {r.x, r.y, 1.0};
    double Rg1[3];
    mv3(C.Kli, el, g1);
    mv3(C.Kri, er, g2);
    mv3(C.R21, g1, Rg1);
    const double numerator = C.T21[0] - C.T21[2] * g2[0]; // e1.dot(T) - e3.dot(T) * e1.dot(ray2)
    const double denominator = Rg1[2] * g2[0] - Rg1[0];
    const double rho1 = numerator / denominator;
    double sl, cl, sr, cr;
    ebvo_sincos(l.theta, &sl, &cl);
    ebvo_sincos(r.theta, &sr, &cr);
    const double t1r[3] = {cl, sl, 0.0}, t2r[3] = {cr, sr, 0.0};
    double t1[3], t2[3], n1[3], c2[3], n2[3];
    mv3(C.Kli, t1r, t1);
    mv3(C.Kri, t2r, t2);
    cross3(t1, g1, n1);
    cross3(t2, g2, c2);
    mtv3(C.R21, c2, n2);
    cross3(n1, n2, T);
    normalize3(T);
    G[0] = rho1 * g1[0];
    G[1] = rho1 * g1[1];
    G[2] = rho1 * g1[2];
}

// ---- a keyframe mate under a pose -------------------------------------------------------------------------------------
// What the inlier refit (pose_refit_kernels.hip), the edge alignment (align_kernels.hip), the inverse-depth filter
// (depth_kernels.hip), the depth carry (carry_kernels.hip) and the temporal ground truth and prior (tgt_kernels.hip) share.
// The operation order of every function is part of their arithmetic contracts (include/ebvo_hip.h): each CPU oracle
// (tests/oracle_*.py) restates it and the device matches bit for bit, so a change here changes all of them together.

// RG = R Gamma and X = RG + t: the mate in the left camera of the current frame
__device__ static inline void pose_point(const double *R, const double *t, const double *G, double *RG, double *X)
{
    mv3(R, G, RG);
#pragma unroll
    for (int i = 0; i < 3; ++i)
        X[i] = RG[i] + t[i];
}
// Y = R21 X + T21: the same point in the right camera
__device__ static inline void stereo_point(const double *R21, const double *T21, const double *X, double *Y)
{
    mv3(R21, X, Y);
#pragma unroll
    for (int i = 0; i < 3; ++i)
        Y[i] = Y[i] + T21[i];
}

// pi(Y) = (K Y)_xy / (K Y)_z; the return value is (K Y)_z, which camera_rows takes
__device__ static inline double camera_pixel(const double *K, const double *Y, double &pix, double &piy)
{
    double p[3];
    mv3(K, Y, p);
    pix = p[0] / p[2];
    piy = p[1] / p[2];
    return p[2];
}
// the two rows of d pi / d Y at that pixel, times Rs (R21 for the right camera; NULL for the identity).  A caller forms its
// residual between camera_pixel and this: the rows are not live while the residual and its weight are computed.
__device__ static inline void camera_rows(const double *K, const double *Rs, double pz, double pix, double piy, double *jx, double *jy)
{
    const double ip = 1.0 / pz;
#pragma unroll
    for (int j = 0; j < 3; ++j)
    {
        jx[j] = ip * (K[j] - pix * K[6 + j]);
        jy[j] = ip * (K[3 + j] - piy * K[6 + j]);
    }
    if (Rs)
    {
        double a[3], b[3];
        mtv3(Rs, jx, a); // row . R21
        mtv3(Rs, jy, b);
#pragma unroll
        for (int j = 0; j < 3; ++j)
        {
            jx[j] = a[j];
            jy[j] = b[j];
        }
    }
}

// Huber at delta on rho >= 0: the weight of the reweighted least squares and the cost
__device__ static inline double huber_weight(double rho, double delta) { return rho <= delta ? 1.0 : delta / rho; }
__device__ static inline double huber_cost(double rho, double delta)
{
    return rho <= delta ? (rho * rho) * 0.5 : delta * (rho - delta * 0.5);
}

// K * G, then `/= z` (src/Temporal_Matches.cpp:84-85): the three components by the z the product gave
__device__ static inline void project3(const double *K, const double *G, double *p)
{
    mv3(K, G, p);
    const double z = p[2];
    p[0] /= z;
    p[1] /= z;
    p[2] /= z;
}
// orientation_mapping (src/Temporal_Matches.cpp:294-333) from T_2: the projected point over its own z, the ray K^-1 gamma,
// the projected tangent
__device__ static inline double mapped_orientation(const double *T2, const double *p, const double *Kinv)
{
    const double g[3] = {p[0] / p[2], p[1] / p[2], p[2] / p[2]};
    double ray[3], t2d[3];
    mv3(Kinv, g, ray);
    project_tangent3(T2, ray, t2d);
    return ebvo_atan2(t2d[1], t2d[0]);
}

// strictly inside the margin (a NaN or infinite coordinate is not), and that in front of the camera
__device__ static inline bool inside_margin(double x, double y, double margin, double x_max, double y_max)
{
    return x > margin && y > margin && x < x_max && y < y_max;
}
__device__ static inline bool live_projection(double x, double y, double z, double margin, double x_max, double y_max)
{
    return inside_margin(x, y, margin, x_max, y_max) && z > 0.0;
}

__device__ static inline bool finite_value(double v) { return fabs(v) < INFINITY; }
// a mate whose depth can be refined or carried: Gamma finite and in front of the keyframe's left camera
__device__ static inline bool live_mate(const double *G)
{
    return finite_value(G[0]) && finite_value(G[1]) && finite_value(G[2]) && G[2] > 0.0;
}

// (int)v / cell inside [0, n_cells), or -1.  The comparison is made on the double, so that NaN and +-inf are in no cell and
// the cast is defined: (int)v / cell >= 0 iff v > -cell, < n_cells iff v < n_cells * cell
__device__ static inline int grid_cell(double v, int cell, int n_cells)
{
    if (!(v > -(double)cell && v < (double)n_cells * (double)cell))
        return -1;
    return (int)v / cell;
}

// the row of quad k in the CSR offsets rp [n_kf + 1]: the last i with rp[i] <= k (rp[0] = 0)
__device__ static inline int quad_row(const int32_t *__restrict__ rp, int n_kf, int k)
{
    int lo = 0, hi = n_kf - 1;
    while (lo < hi)
    {
        const int mid = (lo + hi + 1) >> 1;
        if (rp[mid] <= k)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// score_Pose_Hypothesis for one quad: cv::norm(K (R Gamma + t) / z - left centre) < thr
__device__ static inline bool pose_inlier(const double *Rt, const double *K, const double *G, double ux, double uy, double thr)
{
    double RG[3], h[3], x, y;
    pose_point(Rt, Rt + 9, G, RG, h);
    camera_pixel(K, h, x, y);
    const double dx = x - ux, dy = y - uy;
    return sqrt(dx * dx + dy * dy) < thr;
}
#endif

static inline double cof3_host(const double *m, int i, int j)
{
    const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
    return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1];
}

// Matrix3d::inverse() (Eigen/src/LU/InverseImpl.h, cofactor form), row-major
static inline void inverse3_host(const double *m, double *inv)
{
    const double c0 = cof3_host(m, 0, 0), c1 = cof3_host(m, 1, 0), c2 = cof3_host(m, 2, 0);
    const double det = (c0 * m[0] + c1 * m[3]) + c2 * m[6];
    const double invdet = 1.0 / det;
    inv[0] = c0 * invdet;
    inv[1] = c1 * invdet;
    inv[2] = c2 * invdet;
    for (int i = 1; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            inv[i * 3 + j] = cof3_host(m, j, i) * invdet;
}

// the calibration of the finalisation rows: K_left^-1, K_right^-1, R21, T21
static inline FinalCalib final_calib_host(const double *K_left, const double *K_right, const double *R21, const double *T21)
{
    FinalCalib C;
    inverse3_host(K_left, C.Kli);
    inverse3_host(K_right, C.Kri);
    for (int i = 0; i < 9; ++i)
        C.R21[i] = R21[i];
    for (int i = 0; i < 3; ++i)
        C.T21[i] = T21[i];
    return C;
}

#endif /* EBVO_GEOM_H */
