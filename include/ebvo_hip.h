/*
 * ebvo_hip.h -- C ABI of the MI355X-native edge-extraction-and-matching hot path.
 *
 * Drop-in boundary for Brown-LEMS/Edge_Based_Visual_Odometry (C++17, no FFI of its own): the
 * reference reaches this path through three C++ objects held by Pipeline
 * (include/Pipeline.h:193-195).  Each entry point below names the reference interface it
 * replaces (file:line); INTEGRATION.md shows the adapter classes a maintainer drops in.
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every buffer, the library owns the ctx;
 *   - return 0 (EBVO_OK) or a negative ebvo_status; nothing throws, nothing is retained
 *     across calls; numeric sentinels of the reference are reproduced (NaN for out-of-image
 *     or integer-coordinate bilinear samples, -1.0 for a zero-variance NCC patch);
 *   - one ctx per host thread and per GPU; a ctx is not thread-safe; calls are synchronous
 *     for the caller (internally ordered on the ctx's HIP stream);
 *   - there is NO CPU fallback: without a usable HIP device ebvo_ctx_create fails.
 *
 * Arithmetic contract: IEEE double, separate multiply and add (no FMA), the reference's
 * operation order; atan2 / sin / cos are the correctly rounding routines of
 * csrc/ebvo_math.h.  Edge positions and indices, candidate lists and match-pair IDs are
 * bit-exact against the CPU path; orientations are the correctly rounded value (glibc differs
 * from it by 1 ulp on ~0.06 % of inputs).
 */
#ifndef EBVO_HIP_H
#define EBVO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EBVO_ABI_VERSION 6 /* 2: photometric refinement, stage glue, finalisation, resident chain; 3: pinned result views,
                              undistortion, SIFT descriptors, SIFT stages of the chain; 4: the temporal chain after the
                              NCC filter (ebvo_temporal_params / _counts grew, ebvo_temporal_fetch_final); 5: the resident
                              stage-wise calls (ebvo_toed_resident, ebvo_epi_candidates_resident, ebvo_ncc_pairs_resident); 6: ebvo_toed_screen_audit, ebvo_stereo_upload_async, ebvo_host_register, ebvo_stereo_fetch_compact_begin / _end, ebvo_stereo_pushed_view;
                              still 6 with the additive pose search: ebvo_pose_params / _result, ebvo_pose_default_params,
                              ebvo_temporal_estimate_pose, ebvo_pose_from_quads, ebvo_temporal_final_size,
                              ebvo_debug_set key 20; and with the additive pose stage under ground truth:
                              ebvo_pose_from_quads_gt, ebvo_temporal_estimate_pose_gt, ebvo_pose_constraint_metrics,
                              ebvo_temporal_pose_constraint_metrics; and with the additive inlier refit:
                              ebvo_pose_refine_params / _refined, ebvo_pose_refine_default_params,
                              ebvo_pose_refine_from_quads, ebvo_temporal_refine_pose; and with the additive edge
                              alignment: ebvo_align_params, ebvo_aligned_pose, ebvo_align_default_params,
                              ebvo_pose_align_edges, ebvo_temporal_align_pose, ebvo_temporal_align_size; and with the
                              additive inverse-depth filter: ebvo_depth_params / _refined, ebvo_depth_default_params,
                              ebvo_depth_refine_edges, ebvo_temporal_refine_depth, ebvo_temporal_depth_fetch / _reset,
                              ebvo_temporal_use_depth, ebvo_pose_align_edges_depth; and with the additive handover of
                              the depths on promotion: ebvo_depth_carry_params, ebvo_depth_carried,
                              ebvo_depth_carry_default_params, ebvo_depth_carry, ebvo_temporal_promote_keyframe,
                              ebvo_temporal_depth_source; and with the additive keyframe coverage, switch policy and
                              frame step: ebvo_cover_params, ebvo_keyframe_cover, ebvo_cover_default_params,
                              ebvo_keyframe_cover_edges, ebvo_temporal_keyframe_cover, ebvo_temporal_cover_size,
                              ebvo_keyframe_policy,
                              ebvo_keyframe_policy_default, ebvo_keyframe_decide, ebvo_temporal_keyframe_pose,
                              ebvo_track_params, ebvo_tracked_frame, ebvo_track_default_params,
                              ebvo_temporal_track_frame */

typedef struct ebvo_ctx ebvo_ctx;

/* struct Edge (include/toed/cpu_toed.hpp:26-48) without the cv:: type: location, orientation,
 * index.  b_isEmpty / frame_source are filled by the adapter exactly as TOED leaves them. */
typedef struct ebvo_edge
{
    double x, y, theta;
    int32_t index;
    int32_t pad;
} ebvo_edge;

typedef enum ebvo_status
{
    EBVO_OK = 0,
    EBVO_ERR_ARG = -1,      /* null pointer, non-positive size, size above the ctx maximum */
    EBVO_ERR_CAPACITY = -2, /* an output buffer is too small; the required size is reported */
    EBVO_ERR_HIP = -3,      /* a HIP call failed; see ebvo_last_error */
    EBVO_ERR_NOMEM = -4,
    EBVO_ERR_STATE = -5     /* call made before the data it needs exists */
} ebvo_status;

/* stage_mask bits of ebvo_epi_candidates */
enum
{
    EBVO_STAGE_EPIPOLAR = 1,    /* apply_Epipolar_Line_Distance_Filtering, src/Stereo_Matches.cpp:381-419 */
    EBVO_STAGE_DISPARITY = 2,   /* apply_Disparity_Filtering, :534-553 */
    EBVO_STAGE_ORIENTATION = 4, /* apply_orientation_filter, :863-915 */
    EBVO_STAGE_ALL = 7
};

/* Defaults = the reference's compile-time macros (include/definitions.h:17-24). */
#define EBVO_EPIPOLAR_LINE_DIST_THRESH 0.5
#define EBVO_MAX_DISPARITY 25.0
#define EBVO_ORIENT_THRESH_DEG 10.0
#define EBVO_NCC_THRESH 0.6
#define EBVO_NCC_THRESH_TEMPORAL 0.8
#define EBVO_PATCH_SIZE 7
#define EBVO_PATCH_ELEMS 49

const char *ebvo_strerror(int status);
const char *ebvo_last_error(const ebvo_ctx *ctx); /* text of the last HIP failure, "" if none */
int ebvo_abi_version(void);

/* Replaces ThirdOrderEdgeDetectionCPU::ThirdOrderEdgeDetectionCPU(int H, int W) and its
 * destructor (src/toed/cpu_toed.cpp:24-64, :649-663): device workspace for images up to
 * max_h x max_w on HIP device `device`. */
int ebvo_ctx_create(int device, int max_h, int max_w, ebvo_ctx **out);
void ebvo_ctx_destroy(ebvo_ctx *ctx);

/* How the third-order detector reaches its (identical) result:
 *   EBVO_TOED_STRICT  the reference's direct-form convolution at every pixel (27.6 k fp64 operations per pixel);
 *   EBVO_TOED_HYBRID  a separable fp32 screen selects a superset of the NMS maxima (tolerances 1.9 - 2.3 x the screen's
 *                     WORST-CASE rounding-error bound, which tools/screen_error_bound.py derives from the tap tables and
 *                     toed_kernels.hip asserts at compile time; two orders of magnitude above the error observed on
 *                     images, see ebvo_toed_screen_audit), and only those pixels are evaluated in the
 *                     reference's exact arithmetic.  Same bits out, ~3x less work; see toed_kernels.hip.  An image on
 *                     which the screen flags more grid points than the context's max_h * max_w (possible only when
 *                     most of the image is exact ties, e.g. a one-pixel checkerboard) is re-run on the strict path by
 *                     the library; ebvo_toed_fallbacks counts those.
 * The default is EBVO_TOED_HYBRID unless the environment variable EBVO_TOED_MODE is "strict". */
enum
{
    EBVO_TOED_STRICT = 0,
    EBVO_TOED_HYBRID = 1
};
int ebvo_set_toed_mode(ebvo_ctx *ctx, int mode);
int ebvo_get_toed_mode(const ebvo_ctx *ctx);
int64_t ebvo_toed_fallbacks(const ebvo_ctx *ctx); /* hybrid runs the library repeated on the strict path so far */
/* ebvo_stereo_submit captures the 18 launches of a pair into a hipGraph at the THIRD submission of a slot with unchanged
 * size, parameters and buffers, and launches that graph afterwards (environment EBVO_GRAPHS=0 or ebvo_debug_set(ctx, 10, 0):
 * direct launches).  Number of pairs submitted as a graph launch so far: */
int64_t ebvo_graph_launches(const ebvo_ctx *ctx);
/* diagnostics of the last TOED run on a slot: per image {all NMS maxima, kept edges, screened candidates (hybrid),
 * distinct neighbour grid points whose exact magnitude was evaluated (hybrid)} */
int ebvo_toed_stats(ebvo_ctx *ctx, int slot, int32_t out[8]);

/* Diagnostic of the hybrid detector's FP32 screen (not on any hot path): runs the detector on one image with a variant of the
 * screen kernel that keeps its gx, gy, |g|, and compares them with the exact stage's values at every candidate (and |g| at
 * every neighbour grid point of the screened interior).  The superset property of the screen (hybrid == strict, bit for bit:
 * src/toed/cpu_toed.cpp:406-483 decided from exact values only) rests on max_err_* <= bound_*; tests assert it on full-size
 * images.  Returns EBVO_ERR_CAPACITY when the screen flagged more grid points than the context holds (nothing to audit). */
typedef struct ebvo_screen_audit
{
    int32_t n_candidates;       /* grid points the screen selected */
    int32_t n_maxima;           /* ... of which the exact NMS accepted (Total_Num_Of_TOED) */
    int32_t n_kept;             /* ... inside the 10-px border (toed_edges.size()) */
    int32_t n_neighbour_points; /* distinct neighbour grid points evaluated exactly */
    double max_err_gx, max_err_gy, max_err_mag; /* over the candidates: |screen - exact| */
    double max_err_mag_neighbours;              /* over the neighbour points */
    double bound_g, bound_mag, bound_slope;     /* worst-case budget E_G, E_M, E_S (tools/screen_error_bound.py) */
    double tol_mag, tol_slope;                  /* the relaxed test's tolerances TOL_M, TOL_S */
} ebvo_screen_audit;
int ebvo_toed_screen_audit(ebvo_ctx *ctx, const uint8_t *img, int h, int w, ptrdiff_t stride, ebvo_screen_audit *out);

/*
 * Replaces ThirdOrderEdgeDetectionCPU::get_Third_Order_Edges(cv::Mat)
 * (src/toed/cpu_toed.cpp:66-77: preprocessing + convolve_img + non_maximum_suppresion), called
 * by Pipeline::ProcessEdges (src/Pipeline.cpp:24-29).
 *   img/h/w/stride : CV_8UC1 image (stride in bytes)
 *   out/cap        : toed_edges -- edges inside the 10-px border, raster order, index = position
 *   n_kept         : toed_edges.size();  n_total : Total_Num_Of_TOED (all NMS maxima)
 *   all4/cap_all   : optional subpix_edge_pts_final rows (x, y, theta, sub-pixel magnitude)
 *   t_conv/t_nms   : optional time_conv / time_nms in seconds (device time)
 * On EBVO_ERR_CAPACITY n_kept / n_total hold the required sizes.
 */
int ebvo_toed(ebvo_ctx *ctx, const uint8_t *img, int h, int w, ptrdiff_t stride, ebvo_edge *out, int cap,
              int *n_kept, int *n_total, double *all4, int cap_all, double *t_conv, double *t_nms);

/* Two images of one size in one launch (left + right of a stereo frame, src/Pipeline.cpp:93,97). */
int ebvo_toed_pair(ebvo_ctx *ctx, const uint8_t *img_left, const uint8_t *img_right, int h, int w,
                   ptrdiff_t stride_left, ptrdiff_t stride_right, ebvo_edge *out_left, ebvo_edge *out_right,
                   int cap, int n_kept[2], int n_total[2]);

/* Replaces Stereo_Matches::CalculateEpipolarLine (src/Stereo_Matches.cpp:10-20): l = F (x, y, 1),
 * F row-major, evaluated (F_i0*x + F_i1*y) + F_i2.  Host-side helper (3 flops per line); the
 * adapter may instead pass the lines Eigen produced. */
int ebvo_epipolar_lines(const double F[9], const ebvo_edge *edges, int n, double *lines /* n x 3 */);

/*
 * Replaces extract_Epipolar_Edge_Indices + apply_Epipolar_Line_Distance_Filtering
 * (src/Stereo_Matches.cpp:91-109, :381-419), apply_Disparity_Filtering (:534-553) and
 * apply_orientation_filter (:863-915); stage_mask selects which predicates apply, so the
 * adapter can expose the three stages separately or fused.
 *   L/nL, R/nR : focused (left) edges and candidate (right) edges
 *   lines      : nL x 3 epipolar line coefficients (a, b, c) of the left edges
 *   row_ptr    : nL + 1 CSR offsets;  col_idx/cap : right-edge indices, ascending per row
 *   n_pairs    : number of pairs (required cap on EBVO_ERR_CAPACITY)
 * col_idx may be NULL with cap 0 to size the output.
 */
int ebvo_epi_candidates(ebvo_ctx *ctx, const ebvo_edge *L, int nL, const ebvo_edge *R, int nR,
                        const double *lines, double epi_thr, double max_disp, double orient_thr_deg,
                        int stage_mask, int32_t *row_ptr, int32_t *col_idx, int64_t cap, int64_t *n_pairs);

/* The three geometric stages for a stage-wise caller from ONE device search: the list under the epipolar AND disparity
 * predicates (apply_Epipolar_Line_Distance_Filtering + apply_Disparity_Filtering, :381-419, :534-553) plus one flag per
 * listed pair, orient_ok[k] = the pair passes apply_orientation_filter (:863-915).  The pairs with the flag, in order, are
 * exactly the list ebvo_epi_candidates returns for EBVO_STAGE_ALL; the epipolar-only list (hundreds of candidates per
 * edge) is never formed.  Same calling convention as ebvo_epi_candidates (cap = 0 sizes the list). */
int ebvo_epi_candidates_staged(ebvo_ctx *ctx, const ebvo_edge *L, int nL, const ebvo_edge *R, int nR, const double *lines,
                               double epi_thr, double max_disp, double orient_thr_deg, int32_t *row_ptr, int32_t *col_idx,
                               uint8_t *orient_ok, int64_t cap, int64_t *n_pairs);

/*
 * The same three stages for a caller that runs them ONE AFTER THE OTHER on what the previous stage returned -- main_VO as it
 * is: Pipeline::ProcessEdges x 2 (src/Pipeline.cpp:24-29, :93-97), then apply_Epipolar_Line_Distance_Filtering /
 * apply_Disparity_Filtering / apply_orientation_filter (src/Stereo_Matches.cpp:1374-1399), then apply_NCC_Filtering (:1427).
 * What a stage produced STAYS on the device under a tag; the next stage names it by tag instead of uploading it again, and
 * every result is returned as pointers into page-locked memory owned by the context (valid until the next call of the
 * same function on this context; nothing to free).  The tags of the two most recent ebvo_toed_resident results (one per
 * `which`) are valid until that workspace receives another edge list (ebvo_toed_resident on it, ebvo_toed, ebvo_toed_pair,
 * a pair uploaded into slot 0); the other host-buffer entry points leave them valid, so the SIFT / Best-Nearly-Best /
 * refinement calls get_Stereo_Edge_Pairs makes between the stages do not cost the residency.  A stale tag gives
 * EBVO_ERR_STATE and the caller falls back to the host-buffer entry points above (include/ebvo/adapters.hpp does).
 * Results are bit-identical to ebvo_toed / ebvo_epi_candidates(_staged) / ebvo_ncc_pairs on the same inputs.
 */
typedef struct ebvo_toed_view
{
    const ebvo_edge *edges; /* toed_edges: n_kept records */
    const double *all4;     /* subpix_edge_pts_final: n_total x 4, NULL unless asked for */
    int32_t n_kept, n_total;
    uint64_t tag;           /* names this result in the calls below; never 0 */
    double t_conv, t_nms;   /* seconds of device time */
} ebvo_toed_view;
/* ThirdOrderEdgeDetectionCPU::get_Third_Order_Edges (src/toed/cpu_toed.cpp:66-77) into workspace `which` (0 or 1): the
 * image is uploaded, the edges are detected, copied to page-locked memory AND kept on the device. */
int ebvo_toed_resident(ebvo_ctx *ctx, int which, const uint8_t *img, int h, int w, ptrdiff_t stride, int want_all4,
                       ebvo_toed_view *view);

typedef struct ebvo_candidates_view
{
    const int32_t *row_ptr;   /* n_left + 1 */
    const int32_t *col_idx;   /* n_pairs right-edge indices, ascending per row */
    const uint8_t *orient_ok; /* n_pairs flags (see ebvo_epi_candidates_staged), NULL unless asked for */
    int64_t n_pairs;
    /* with the flags also the list they select, i.e. the lists after apply_orientation_filter (= ebvo_epi_candidates with
     * EBVO_STAGE_ALL): what the next stage takes as its row_ptr / col_idx */
    const int32_t *row_ptr_final; /* n_left + 1 */
    const int32_t *col_idx_final; /* n_final */
    int64_t n_final;
} ebvo_candidates_view;
/* ebvo_epi_candidates / ebvo_epi_candidates_staged on two resident edge lists (left and right may sit in either
 * workspace); only the nL x 3 line coefficients travel to the device. */
int ebvo_epi_candidates_resident(ebvo_ctx *ctx, uint64_t tag_left, uint64_t tag_right, const double *lines, double epi_thr,
                                 double max_disp, double orient_thr_deg, int stage_mask, int want_orient_flags,
                                 ebvo_candidates_view *view);

enum
{
    EBVO_NCC_WANT_LEFT_PATCHES = 1, /* left_edge_patches (src/Stereo_Matches.cpp:578): n_left x 2 x 49 floats */
    EBVO_NCC_WANT_SIMS = 2          /* the four scores of every pair (:592-595) */
};
typedef struct ebvo_ncc_view
{
    const float *left_patches; /* n_left x 98 */
    const double *sims;        /* n_pairs x 4 */
    const double *best;        /* n_pairs: final_SIM_score (:596) */
    const uint8_t *keep;       /* n_pairs: best > thr (:597) */
    int32_t n_left;
    int64_t n_pairs;
} ebvo_ncc_view;
/* apply_NCC_Filtering in its FIRST pass (:1427), where every candidate is a right TOED edge: the pairs are given as CSR
 * indices into the resident right edge list (contributing_edges_toed_indices[0], :413) instead of 32-byte edge records.
 * imgL / imgR are the RAW images (:562-563); they are uploaded (0.5 MB each), the edges are not. */
int ebvo_ncc_pairs_resident(ebvo_ctx *ctx, uint64_t tag_left, uint64_t tag_right, const uint8_t *imgL, const uint8_t *imgR,
                            int h, int w, ptrdiff_t strideL, ptrdiff_t strideR, const int32_t *row_ptr,
                            const int32_t *col_idx, double thr, int want, ebvo_ncc_view *view);

/*
 * Replaces Stereo_Matches::apply_NCC_Filtering (src/Stereo_Matches.cpp:555-616) and under it
 * Utility::get_edge_patches / get_patch_similarity (src/utility.cpp:182-212, :163-180).
 *   imgL/imgR     : the raw left / right CV_8UC1 images (:562-563)
 *   L/nL          : left edges;  row_ptr : nL + 1 CSR offsets into the pair arrays
 *   Rc            : one explicit candidate edge per pair (a TOED edge in the first pass, a
 *                   cluster centre in the second, :588)
 *   left_patches  : optional nL x 2 x 49 floats (plus, minus) -- left_edge_patches (:578)
 *   sims          : optional n_pairs x 4 doubles (pp, nn, pn, np) (:592-595)
 *   best          : optional n_pairs doubles, std::max of the four (:596)
 *   keep          : optional n_pairs bytes, best > thr (:597)
 */
int ebvo_ncc_pairs(ebvo_ctx *ctx, const uint8_t *imgL, const uint8_t *imgR, int h, int w,
                   ptrdiff_t strideL, ptrdiff_t strideR, const ebvo_edge *L, int nL, const ebvo_edge *Rc,
                   const int32_t *row_ptr, double thr, float *left_patches, double *sims, double *best,
                   uint8_t *keep);

/* ---- input side (OpenCV is not part of the reference tree: parity unpinned) -------------- */

/* cv::undistort(img, out, K, dist) as Pipeline::prepare_Stereo_Images calls it (src/Pipeline.cpp:78-79: no new camera
 * matrix; K = fx fy cx cy of include/Dataset.h get_*_calib_matrix_cvMat, dist = k1 k2 p1 p2 [k3], n_dist = 4 or 5,
 * include/Dataset.h:396-397).  OpenCV 4.x restated: stripe-wise maps with 5 fractional bits, fixed-point bilinear
 * remap, constant-0 border.  Zero distortion returns the input image. */
int ebvo_undistort(ebvo_ctx *ctx, const uint8_t *img, int h, int w, ptrdiff_t stride, const double K[4], const double *dist,
                   int n_dist, uint8_t *out, ptrdiff_t out_stride);

/* The resident pipeline undistorts the uploaded pair itself: TOED, the refinement and the output geometry then run on the
 * undistorted images while the NCC passes sample the RAW ones, exactly as the reference does (src/Pipeline.cpp:93-97 vs
 * src/Stereo_Matches.cpp:562-563).  p = NULL switches it off (KITTI, ETH3D: zero distortion, same result either way). */
typedef struct ebvo_undistort_params
{
    double K_left[4], K_right[4];       /* fx fy cx cy */
    double dist_left[5], dist_right[5]; /* k1 k2 p1 p2 k3 */
    int n_dist;                         /* 4 or 5 */
    int reserved;
} ebvo_undistort_params;
int ebvo_stereo_set_undistort(ebvo_ctx *ctx, const ebvo_undistort_params *p);

/* ---- fixed-scale SIFT descriptors (cv::SIFT is third-party: parity unpinned) --------------- */

#define EBVO_SIFT_THRESHOLD 500.0 /* include/definitions.h:40 */
#define EBVO_SIFT_DESC_LEN 128

/*
 * Replaces the cv::SIFT::create()->compute(image, {kp1, kp2}, desc) calls of Stereo_Matches::augment_Edge_Data
 * (src/Stereo_Matches.cpp:655-689), apply_SIFT_filtering (:716-727) and finalize_stereo_edge_mates (:1627-1635): the
 * descriptors at the two points 8 px either side of every edge (get_Orthogonal_Shifted_Points(edge, 8)), keypoint size 1,
 * angle 180 / pi * theta.  OpenCV 4.x restated: first pyramid level = GaussianBlur(sigma sqrt(1.6^2 - 0.5^2)) of the
 * image, formed ONCE per call instead of once per edge; 4 x 4 x 8 histogram over an 11 x 11 window; values 0 .. 255
 * stored as floats like cv::SIFT's CV_32F descriptors.
 *   img : the undistorted CV_8UC1 image;  desc : n x 2 x 128 floats (plus point, minus point)
 */
int ebvo_sift_descriptors(ebvo_ctx *ctx, const uint8_t *img, int h, int w, ptrdiff_t stride, const ebvo_edge *edges, int n,
                          float *desc);

/* The score of Stereo_Matches::apply_SIFT_filtering (:736-740): per candidate pair the smallest of the four L2 distances
 * between the two descriptors of the left edge and the two of the candidate.  left_desc: nL x 2 x 128, cand_desc: one
 * descriptor pair per PAIR (n_pairs x 2 x 128, the order of the CSR lists); dist: n_pairs doubles.  The filter keeps
 * dist < EBVO_SIFT_THRESHOLD and stores dist as refine_confidences (:752-757). */
int ebvo_sift_min_distances(ebvo_ctx *ctx, const float *left_desc, int nL, const float *cand_desc, const int32_t *row_ptr,
                            double *dist);

/* ---- photometric refinement (no fixture of the reference pins it) -------------------- */

/* Defaults of Stereo_Matches::min_Edge_Photometric_Residual_by_Gauss_Newton_along_EpipolarLine
 * (include/Stereo_Matches.h:79-84). */
#define EBVO_GN_MAX_ITER 20
#define EBVO_GN_TOL 1e-3
#define EBVO_GN_HUBER_DELTA 3.0

typedef struct
{
    int max_iter;       /* >= 1 */
    double tol;         /* |delta| below which the iteration stops */
    double huber_delta; /* Huber threshold; outlier if rms > 2 * huber_delta */
} ebvo_gn_params;

void ebvo_gn_default_params(ebvo_gn_params *p);

/* util_compute_Img_Gradients (include/utility.h:131-141; called from src/Pipeline.cpp:83-84): cv::Sobel 3x3 with
 * scale 1/8 and OpenCV's default border (reflect-101) of the CV_8UC1 image converted to CV_32F.
 * gx, gy: h x w floats, tightly packed. */
int ebvo_sobel_gradients(ebvo_ctx *ctx, const uint8_t *img, int h, int w, ptrdiff_t stride, float *gx, float *gy);

/*
 * Replaces the per-candidate body of Stereo_Matches::refine_edge_disparity (src/Stereo_Matches.cpp:1290-1358) and
 * under it min_Edge_Photometric_Residual_by_Gauss_Newton_along_EpipolarLine (:1159-1288): 1-D Gauss-Newton on the
 * photometric residual of the two 7x7 side patches, the right patch pair sliding along the epipolar direction
 * (-b, a)/|(-b, a)| of the left edge's line (:1331-1336), Huber weights, init_alpha 0.
 *   imgL/imgR   : the undistorted left / right CV_8UC1 images (the reference converts them to CV_32F, :1292-1294;
 *                 pass them swapped for is_left = false).  The gradients of imgR are formed internally.
 *   L/nL, lines : left edges and their nL x 3 line coefficients (epip_line_coeffs_of_left_edges)
 *   row_ptr     : nL + 1 CSR offsets into the pair arrays;  cand_xy : n_pairs x 2 candidate locations
 *                 (EdgeCluster::center_edge.location)
 * Outputs, one per pair: alpha (refined_alpha), score (refine_final_scores: final RMS), confidence
 * (refine_confidences: exp(-rms / huber_delta)), validity (refine_validities: 0 / 1), iters (iterations
 * executed) and refined_xy (the updated centre location, :1349-1351).  validity = 2 marks the case the reference
 * leaves undefined: it stops on H < 1e-8 without assigning its outputs (:1255); score and confidence are NaN there.
 */
int ebvo_gn_refine_stereo(ebvo_ctx *ctx, const uint8_t *imgL, const uint8_t *imgR, int h, int w, ptrdiff_t strideL,
                          ptrdiff_t strideR, const ebvo_edge *L, int nL, const double *lines, const int32_t *row_ptr,
                          const double *cand_xy, const ebvo_gn_params *params, double *alpha, double *score,
                          double *confidence, uint8_t *validity, int32_t *iters, double *refined_xy);

/*
 * Replaces Temporal_Matches::min_Edge_Photometric_Residual_by_Gauss_Newton (src/Temporal_Matches.cpp:735-851) as
 * apply_photometric_refinement_quads calls it (:572-634, once for the left and once for the right image of a quad):
 * 2-D Gauss-Newton on the photometric residual between the keyframe edge's side patches and the current-frame edge's,
 * the current-frame patch pair (oriented by the CURRENT-frame edge) placed at kf.location - d.
 *   imgKF / imgCF : undistorted keyframe / current-frame CV_8UC1 images of one camera; gradients of imgCF are formed
 *                   internally (current_frame.*_image_gradients_*)
 *   kf, cf, init_disp : n keyframe edges, n current-frame edges, n x 2 initial disparities (kf.location - cf.location)
 * Outputs per item: disp (refined_disparity, n x 2), score (final RMS), validity (0 / 1), iters.  The update solves the
 * 2x2 system with Eigen 3.4's pivoted LDL^T as published (H.ldlt().solve(b), :818).
 */
int ebvo_gn_refine_temporal(ebvo_ctx *ctx, const uint8_t *imgKF, const uint8_t *imgCF, int h, int w, ptrdiff_t strideKF,
                            ptrdiff_t strideCF, const ebvo_edge *kf, const ebvo_edge *cf, const double *init_disp, int n,
                            const ebvo_gn_params *params, double *disp, double *score, uint8_t *validity, int32_t *iters);

/* ---- stage glue on CSR candidate lists (no fixture of the reference pins it) ----------- */

#define EBVO_BNB_NCC 0.9  /* include/definitions.h:34 */
#define EBVO_BNB_SIFT 0.4 /* :33 */

/*
 * Stereo_Matches::apply_Best_Nearly_Best_Test (src/Stereo_Matches.cpp:789-862) on every row of a CSR list.
 *   scores           : one per pair -- refine_final_scores with higher_is_better = 1 (is_NCC), refine_confidences
 *                      (SIFT distances) with higher_is_better = 0
 *   new_count[nL]    : survivors per row;  order[n_pairs] : order[row_ptr[i] + k] = pair index of the k-th survivor of
 *                      row i (k < new_count[i]), in the order the reference leaves them: by score when something was
 *                      dropped, untouched otherwise (:840).  The order among equal scores is std::sort's, i.e. libstdc++'s
 *                      introsort restated move for move (csrc/ebvo_sort.h): original position for rows of at most 16
 *                      candidates, wherever its partitioning leaves them for longer rows.
 */
int ebvo_bnb_test(ebvo_ctx *ctx, const int32_t *row_ptr, int nL, const double *scores, double ratio_thr,
                  int higher_is_better, int32_t *new_count, int32_t *order);

/* Stereo_Matches::apply_Lowe_Ratio_Test as written (:916-964): only the best-scoring candidate of each row survives
 * (the first one on ties; candidate 0 if no score exceeds -1).  Same outputs as ebvo_bnb_test. */
int ebvo_keep_best(ebvo_ctx *ctx, const int32_t *row_ptr, int nL, const double *scores, int32_t *new_count,
                   int32_t *order);

/*
 * Stereo_Matches::shift_Edge_to_Epipolar_Line (:26-89) for every candidate of every row, i.e. the shift-only pass of
 * consolidate_redundant_edge_hypothesis (:976-996): cand / shifted hold n_pairs edges (x, y, theta; index is returned
 * 0 like the reference's Edge{loc, theta, false, 0}), lines the nL x 3 epipolar coefficients of the left edges.
 * tan(theta) is formed as sin / cos of the library's correctly rounded pair, pow(x, 2) as x * x.
 */
int ebvo_epipolar_shift(ebvo_ctx *ctx, const ebvo_edge *cand, const double *lines, const int32_t *row_ptr, int nL,
                        ebvo_edge *shifted);

/*
 * EdgeClusterer::performClustering (src/EdgeClusterer.cpp:119-302) on every row of a CSR list, as the clustering pass of
 * consolidate_redundant_edge_hypothesis runs it (src/Stereo_Matches.cpp:1006-1034): single-linkage merging of the
 * candidates' locations below CLUSTER_DIST_THRESH = 1 px (and |dtheta| < 20 deg if by_orientation), clusters capped at
 * MAX_CLUSTER_SIZE = 10, one Gaussian-weighted average edge per cluster.  skip_single = 1 leaves rows with one
 * candidate untouched (the cluster-only call, :998-999).
 *   new_count[nL]      : clusters per row
 *   centres[n_pairs]   : centres[row_ptr[i] + c] = centre edge of cluster c of row i (c < new_count[i]); the rest of a
 *                        row's slots is unspecified
 *   cluster_of[n_pairs]: cluster index (0 .. new_count[i] - 1) of every input candidate: its contributing_edges
 * Merging decisions are exact; the centres carry the device exp() in their weights (within 1e-12 px of glibc's).
 */
int ebvo_cluster_rows(ebvo_ctx *ctx, const ebvo_edge *cand, const int32_t *row_ptr, int nL, int by_orientation,
                      int skip_single, int32_t *new_count, ebvo_edge *centres, int32_t *cluster_of);

/* ---- finalisation geometry (what the output file holds) ----------------- */

typedef struct
{
    double K_left[9], K_right[9]; /* row-major 3x3 calibration matrices (Dataset::get_left/right_calib_matrix) */
    double R21[9], T21[3];        /* get_relative_rot_left_to_right / get_relative_transl_left_to_right */
} ebvo_stereo_calib;

/*
 * The numeric body of Stereo_Matches::write_finalized_stereo_edge_pairs_to_file (src/Stereo_Matches.cpp:1656-1699)
 * with Utility::backproject_2D_point_to_3D_point_using_rays, reconstruct_3D_Tangent_through_intersection_of_planes
 * and project_3D_Tangent_to_2D_Tangent (src/utility.cpp:95-119): per final (left edge, right edge) pair the 16
 * numbers of one output row, out16[k] = {lx, ly, ltheta, rx, ry, rtheta, Gamma.x, .y, .z, T.x, .y, .z,
 * projected_T_1.x, .y, projected_T_2.x, .y}.  The text itself (header line, 6 significant digits, spaces) is written
 * by the caller (ebvo::write_finalized_stereo_edge_pairs in include/ebvo/adapters.hpp uses the reference's iostream
 * calls).
 */
int ebvo_finalize_pairs(ebvo_ctx *ctx, const ebvo_stereo_calib *calib, const ebvo_edge *left, const ebvo_edge *right,
                        int n, double *out16);

/*
 * The same refinement on the pair resident in `slot` after ebvo_stereo_run / ebvo_stereo_wait, without leaving the
 * device: every candidate pair the NCC filter kept (keep[k] = 1) is refined against its right TOED edge, using the
 * pipeline's own edge lists, lines and images.  Outputs are indexed like sims / keep (n_pairs entries); pairs that
 * were not kept get validity 255, alpha 0 and their unrefined location.  Any output pointer may be NULL.
 */
int ebvo_stereo_refine(ebvo_ctx *ctx, int slot, const ebvo_gn_params *params);
int ebvo_stereo_fetch_refined(ebvo_ctx *ctx, int slot, double *alpha, double *score, double *confidence,
                              uint8_t *validity, int32_t *iters, double *refined_xy);

/*
 * The stages of get_Stereo_Edge_Pairs after the NCC pass (src/Stereo_Matches.cpp:1418-1481), without SIFT, on the pair
 * resident in `slot` and without the candidate lists leaving the device:
 *   [SIFT filter ->] kept NCC matches -> apply_Best_Nearly_Best_Test(BNB_NCC) [-> (BNB_SIFT)] -> epipolar shift ->
 *   refine_edge_disparity -> epipolar shift + clustering by orientation (:1483 as its arguments bind) ->
 *   apply_NCC_Filtering on the cluster centres -> best candidate per row -> rows with a match
 * and, if calib is given, the 16 numbers of the output file per final pair.  Each stage is the kernel behind the
 * corresponding host-buffer entry point (ebvo_bnb_test, ebvo_epipolar_shift, ebvo_gn_refine_stereo,
 * ebvo_cluster_rows, ebvo_ncc_pairs, ebvo_keep_best, ebvo_finalize_pairs), so the result equals chaining those calls
 * on the fetched data.  With use_sift the SIFT filter (:1414) and the BNB test on the SIFT distances (:1452) run too
 * (ebvo_sift_descriptors / ebvo_sift_min_distances on the resident pair): the chain is then get_Stereo_Edge_Pairs stage for
 * stage.  (The NCC of a pair does not depend on which other pairs survive, so filtering by SIFT after the first NCC pass
 * of ebvo_stereo_run selects the same pairs, with the same scores, as the reference's SIFT-then-NCC order.)
 */
typedef struct
{
    double bnb_ratio; /* EBVO_BNB_NCC */
    double ncc_thr;   /* EBVO_NCC_THRESH, second pass */
    ebvo_gn_params gn;
    int use_sift;     /* 1: SIFT filter (:1414) and Best-Nearly-Best on the SIFT distances (:1452) are part of the chain */
    int reserved;
    double sift_thr;  /* EBVO_SIFT_THRESHOLD */
    double bnb_sift;  /* EBVO_BNB_SIFT */
} ebvo_finalize_params;

typedef struct
{
    int32_t n_ncc, n_bnb, n_clusters, n_ncc2, n_final; /* candidates surviving each stage (n_ncc: SIFT and NCC filter) */
    int32_t n_sift;                                    /* candidates passing the SIFT filter alone (use_sift) */
} ebvo_finalize_counts;

void ebvo_finalize_default_params(ebvo_finalize_params *p); /* the reference's constants, use_sift = 0 */
int ebvo_stereo_finalize(ebvo_ctx *ctx, int slot, const ebvo_finalize_params *params, const ebvo_stereo_calib *calib,
                         ebvo_finalize_counts *counts);
/* The same chain without blocking the caller: _submit ENQUEUES every stage on the slot's stream (the stage totals stay on
 * the device; no count is read back in between) and returns; _wait blocks until the chain has run and returns the
 * counts.  A frame loop keeps several slots in flight: the chains of different slots run concurrently on the device.
 * Between the two calls the slot accepts no other call (EBVO_ERR_STATE). */
int ebvo_stereo_finalize_submit(ebvo_ctx *ctx, int slot, const ebvo_finalize_params *p, const ebvo_stereo_calib *calib);
int ebvo_stereo_finalize_wait(ebvo_ctx *ctx, int slot, ebvo_finalize_counts *counts);
/* n_final entries each: index of the left TOED edge, the matched right centre edge, its NCC score, and (if calib was
 * given) the 16 numbers of the output row.  Any pointer may be NULL. */
int ebvo_stereo_fetch_final(ebvo_ctx *ctx, int slot, int32_t *left_index, ebvo_edge *right_edge, double *ncc_score,
                            double *out16);

/* Utility::get_edge_patches for n edges on one image: patches = n x 2 x 49 floats
 * (src/utility.cpp:182-212; used again by finalize_stereo_edge_mates, src/Stereo_Matches.cpp:1622). */
int ebvo_edge_patches(ebvo_ctx *ctx, const uint8_t *img, int h, int w, ptrdiff_t stride,
                      const ebvo_edge *edges, int n, float *patches);

/* Utility::get_patch_similarity over n explicit pairs of stored 7x7 float patches
 * (src/utility.cpp:163-180); also the MatlabNCCComputer::computeNCC-shaped entry
 * (include/MatlabNCCComputer.h:41): sim[k] = ncc(A[k], B[k]). */
int ebvo_ncc_patches(ebvo_ctx *ctx, const float *A, const float *B, int n, double *sim);

/* Replaces the scoring loop of Temporal_Matches::apply_NCC_filtering_quads
 * (src/Temporal_Matches.cpp:426-468): per quad k, stored (plus, minus) patches of the keyframe
 * mate and the current-frame mate on the left and on the right (n x 2 x 49 floats each);
 * sim_left / sim_right = max of the four NCCs in the order (:441-450); keep = both > thr. */
int ebvo_ncc_quads(ebvo_ctx *ctx, const float *kfL, const float *kfR, const float *cfL, const float *cfR,
                   int n, double thr, double *sim_left, double *sim_right, uint8_t *keep);

/* ---- temporal quads on the resident pairs (Temporal_Matches; BASELINE configs[2]) -------------------------------- */
/* The part of Temporal_Matches::get_Temporal_Edge_Pairs_from_Quads (src/Temporal_Matches.cpp:168-218) that does not
 * need ground-truth poses: for every stereo mate of the keyframe the candidate mates of the current frame
 * (apply_spatial_grid_filtering_quads :335-383: left edge within +-ceil(radius / cell) grid cells of the keyframe
 * mate's left edge AND right edge likewise, whole cells as SpatialGrid::getCandidatesWithinRadius returns them;
 * apply_orientation_filtering_quads :385-414: both orientation differences within the threshold) and
 * apply_NCC_filtering_quads (:416-469) on the mates' stored patches: left_edge_patches from the raw left image, right
 * patches from the undistorted right image at the final right edge (src/Stereo_Matches.cpp:1621-1622).
 * Mates = the final pairs of ebvo_stereo_finalize on a slot.  The candidates of a keyframe mate are listed in the order
 * of the reference's `left_candidates`: neighbour cell by neighbour cell (dy outer, dx inner), ascending mate index
 * within a cell (include/Dataset.h:92-113).
 * Accepted ranges (anything else: EBVO_ERR_ARG from ebvo_temporal_match(_submit), nothing touched): cell_size >= 1;
 * grid_radius finite and >= 0 (a radius wider than the grid selects the whole grid and costs no more); orient_thr_deg >= 0;
 * stages 0 or 1; with stages = 1 also sift_thr > 0, bnb_ncc >= 0, bnb_sift >= 0, gn.max_iter >= 1, gn.tol >= 0,
 * gn.huber_delta > 0.  ebvo_finalize_params: bnb_ratio >= 0, ncc_thr not NaN, the same gn ranges, and with use_sift
 * sift_thr > 0 and bnb_sift >= 0. */
typedef struct ebvo_temporal_params
{
    int cell_size;         /* GRID_SIZE 15, include/definitions.h:45 */
    int stages;            /* 0: through the NCC filter (src/Temporal_Matches.cpp:184-192);
                              1: the rest of get_Temporal_Edge_Pairs_from_Quads as well (:196-215): SIFT filter, Best-Nearly-Best
                                 on the NCC and on the SIFT scores, photometric refinement of both cameras, edge clustering */
    double grid_radius;    /* 30, src/Temporal_Matches.cpp:184 */
    double orient_thr_deg; /* 10, :188 */
    double ncc_thr;        /* EBVO_NCC_THRESH_TEMPORAL 0.8, :192 */
    double sift_thr;       /* 200, :196: both min-of-four descriptor distances (left and right camera) below it */
    double bnb_ncc;        /* 0.8, :200 */
    double bnb_sift;       /* 0.8, :204 */
    ebvo_gn_params gn;     /* 20 iterations, 1e-3, Huber 3.0, :612-617 */
} ebvo_temporal_params;
typedef struct ebvo_temporal_counts
{
    int32_t n_kf, n_cf;   /* keyframe / current-frame mates */
    int64_t n_candidates; /* quads after the grid and orientation filters */
    int64_t n_kept;       /* quads with both NCC maxima above the threshold */
    int64_t n_sift, n_bnb_ncc, n_bnb_sift; /* stages = 1: quads surviving each later filter */
    int64_t n_refined_valid;               /* quads whose refinement is valid in both cameras (they all stay, :618) */
    int64_t n_final;                       /* quads after the edge clustering */
} ebvo_temporal_counts;
void ebvo_temporal_default_params(ebvo_temporal_params *p);
/* the final mates of `slot` (after ebvo_stereo_finalize) become the keyframe (src/Pipeline.cpp:133-138: frame 0).
 * The context holds ONE keyframe, and a submitted match reads it until its _wait has returned: while ANY slot of the
 * context has a temporal match in flight the call returns EBVO_ERR_STATE and the stored keyframe stays as it is. */
int ebvo_temporal_set_keyframe(ebvo_ctx *ctx, int slot);
/* quads of the keyframe against the final mates of `slot`.
 * The keyframe and the current frame may differ in size with stages = 0 (the candidate search runs on the current frame's
 * grid, the NCC on stored patches).  stages = 1 refines every quad on the keyframe's and the current frame's images with
 * one shape: a current frame of another size than the keyframe's is refused with EBVO_ERR_STATE (ebvo_last_error says
 * so) before anything of the slot changes -- its earlier quads and final list stay fetchable. */
int ebvo_temporal_match(ebvo_ctx *ctx, int slot, const ebvo_temporal_params *p, ebvo_temporal_counts *counts);
/* The same without blocking the caller (see ebvo_stereo_finalize_submit): _submit enqueues the candidate search and the NCC
 * of the stored patches on the slot's stream and returns, _wait returns the counts (and, for stages = 1, runs the rest of
 * the chain).  Frames in different slots overlap on the device. */
int ebvo_temporal_match_submit(ebvo_ctx *ctx, int slot, const ebvo_temporal_params *p);
int ebvo_temporal_match_wait(ebvo_ctx *ctx, int slot, ebvo_temporal_counts *counts);
/* The quads that leave the whole chain (stages = 1), CSR over the keyframe mates: row_ptr n_kf + 1; per final quad the
 * current-frame mate it is copied from (`best_idx` of :713), the left cluster centre (EdgeClusterer's weighted average, or
 * the refined left edge of an unclustered quad), the right centre (the mean of the members' refined right edges), the left
 * NCC and SIFT scores, the final residuals of both refinements and refine_validity.  Any pointer may be NULL. */
int ebvo_temporal_fetch_final(ebvo_ctx *ctx, int slot, int32_t *row_ptr, int32_t *cf_index, ebvo_edge *left, ebvo_edge *right,
                              double *ncc_left, double *sift_left, double *score_left, double *score_right, uint8_t *valid);
/* row_ptr: n_kf + 1; col_idx / sim_left / sim_right / keep: n_candidates.  Any pointer may be NULL. */
int ebvo_temporal_fetch(ebvo_ctx *ctx, int slot, int32_t *row_ptr, int32_t *col_idx, double *sim_left, double *sim_right,
                        uint8_t *keep);

/* ---- relative pose from the temporal quads (MotionTracker::estimate_Relative_Pose_From_Quad_Pairs) ----------------- */
/* RANSAC over pairs of final quads (src/MotionTracker.cpp:175-253, Ransac_Options / Ransac_State of include/MotionTracker.h,
 * TAU_C1..C4 of include/definitions.h), restated literally:
 *   - per quad (KF mate i, candidate j) Gamma / T from the keyframe mate and Gamma_bar / T_bar from the quad's left and right
 *     cluster centres (get_Gammas_and_Tangents_From_Quads :28-66): columns 6-11 of ebvo_finalize_pairs with K_right := K_left
 *     (the reference uses get_left_calib_matrix() for both cameras here; K_right of `cal` is not read);
 *   - rank order (:90-103): ascending row length of the KF mate, then KF index, then candidate index; every quad is kept
 *     (the has_gt() filter on the keyframe mates is not applied here: ebvo_pose_from_quads_gt /
 *     ebvo_temporal_estimate_pose_gt below apply it, and ebvo_pose_constraint_metrics reads b_is_veridical);
 *     top_n = (size_t)(top_rank_fraction * n_quads);
 *   - the loop: termination test at its top (iterations > min_iterations && iterations > dynamic_max_iter), two indices
 *     rand() % top_n redrawn together while equal, the length / T1 / T2 / tangent constraints (:108-134; a rejected draw
 *     sets iterations = iterations > 0 ? iterations - 1 : 0, so a rejection at iteration 0 still advances it to 1), the pose
 *     R = B_bar B^T, t = Gamma_bar_1 - R Gamma_1 (:136-153), the score over ALL quads (sqrt(dx^2 + dy^2) < max_reproj_error
 *     of K_left (R Gamma + t) against the quad's left centre, :155-173), the best hypothesis replaced only by a strictly
 *     larger count, and dynamic_max_iter from the three branches (>= 0.95 / <= 0.05 / ceil(log(1 - success_prob) /
 *     log(1 - ratio^2) * dyn_num_trials_mult)).
 *   - the random stream is glibc's rand() (TYPE_3 additive generator) restated per context: rand_seed is the srand() value
 *     (1 = the never-seeded rand() of main_VO; Ransac_Options::seed is dead code in the reference).  libc rand() is never
 *     called.  continue_stream = 1 continues the context's generator where the previous pose call left it (one
 *     process-global rand() across frames); the first call of a context seeds it with rand_seed.
 * Deliberate divergences, where the reference has undefined behaviour or never returns:
 *   - fewer than 2 quads or top_n < 2 (rand() % 0, or an endless redraw of idx1 == idx2): status 1, identity pose, nothing
 *     launched and no random number drawn (quads_by_kf.size() < 2 of the reference counts GT-veridical KF mates only, which
 *     the pose search does not read; this rule replaces it);
 *   - at most max_draws index pairs (idx1 != idx2) are drawn: when the loop still needs one more, status 2 (the reference
 *     loops forever when no pair passes the constraints);
 *   - the ceil(...) of the third branch is clamped to [0, 2^62] before its conversion to an integer.
 * Accepted ranges (anything else: EBVO_ERR_ARG, nothing touched): no NaN anywhere; 0 < success_prob < 1;
 * 0 < top_rank_fraction <= 1; max_reproj_error and the four taus >= 0 (+inf allowed); max_iterations, min_iterations >= 0;
 * max_draws >= 1; dyn_num_trials_mult > 0. */
typedef struct ebvo_pose_params /* defaults (ebvo_pose_default_params) = Ransac_Options + TAU_C1..4 */
{
    int32_t max_iterations, min_iterations;         /* 5000, 1000 */
    double dyn_num_trials_mult, success_prob;       /* 3.0, 0.97 */
    double max_reproj_error, top_rank_fraction;     /* 1.5 px, 0.7 */
    double tau_length, tau_t1, tau_t2, tau_tangent; /* 0.13 0.12 0.12 0.32 */
    uint32_t rand_seed;      /* srand() value (0 acts as 1, as in glibc); default 1 = the never-seeded rand() of main_VO */
    int32_t continue_stream; /* 1: continue this ctx's generator from the previous pose call (a process-global rand()) */
                             /* The generator is ONE per context, shared by its slots: pose calls on one context from several
                                threads race on it (a context is not thread-safe), and with continue_stream = 1 calls on
                                different slots continue one stream in call order, as one process-global rand() would. */
    int64_t max_draws;       /* index pairs drawn at most (reference: unbounded); default 1 << 22 */
} ebvo_pose_params;
typedef struct ebvo_pose_result
{
    double R[9], t[3];        /* row-major; identity / 0 if no hypothesis beat 0 inliers */
    int32_t status, found;    /* 0 ok / 1 insufficient quads / 2 draw cap reached; found = best_inliers > 0 */
    int64_t n_quads, top_n;
    int64_t iterations;       /* Ransac_State::iterations when the loop ended */
    int64_t draws;            /* index pairs (idx1 != idx2) the loop consumed */
    int64_t hypotheses;       /* ... of them passing the four constraints (scored) */
    int64_t best_inliers;     /* best_minimal_inlier_count */
    int64_t dynamic_max_iter;
    double inlier_ratio;
    int32_t best_q1, best_q2; /* positions in the rank order of the best hypothesis' pair; -1 if none */
} ebvo_pose_result;
void ebvo_pose_default_params(ebvo_pose_params *p);
/* On the slot's final quads (after ebvo_temporal_match with stages = 1) and the ctx's keyframe mates.  EBVO_ERR_STATE when
 * the slot has no final quads, a pair, finalisation or temporal stage of it is in flight, or the keyframe was replaced since
 * the quads were matched.  inlier (may be NULL): n_final bytes in the CSR order of ebvo_temporal_fetch_final, 1 = inlier of
 * the best hypothesis.  The slot's results (ebvo_temporal_fetch_final / ebvo_temporal_fetch) are not changed. */
int ebvo_temporal_estimate_pose(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_pose_params *p,
                                ebvo_pose_result *res, uint8_t *inlier);
/* The sizes of the slot's final quads (what ebvo_temporal_fetch_final returns and `inlier` above needs): keyframe mates and
 * quads.  EBVO_ERR_STATE when the slot has none or a pair or temporal stage of it is in flight. */
int ebvo_temporal_final_size(ebvo_ctx *ctx, int slot, int32_t *n_kf, int64_t *n_final);
/* The same on host arrays: KF mates per row (n_kf), CSR row_ptr (n_kf + 1, row_ptr[0] = 0, non-decreasing), the CF left / right
 * centres per quad (row_ptr[n_kf]).  quad_geom (may be NULL): n x 12 = Gamma, Gamma_bar, T, T_bar in CSR order; rank_order
 * (may be NULL): n, the CSR index at each rank position.  Both are left untouched when status = 1.  Runs on slot 0's
 * stream (EBVO_ERR_STATE while work of slot 0 is in flight) without touching slot 0's results. */
int ebvo_pose_from_quads(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf, const int32_t *row_ptr,
                         const ebvo_edge *cf_left, const ebvo_edge *cf_right, const ebvo_stereo_calib *cal,
                         const ebvo_pose_params *p, ebvo_pose_result *res, uint8_t *inlier, double *quad_geom,
                         int32_t *rank_order);

/* ---- the pose stage under ground truth (the has_gt() == true branch of src/MotionTracker.cpp:68-106, :255-381) -------- */
/* Selected quads.  Under ground truth the reference's quads_by_kf holds the keyframe mates with at least one veridical quad
 * (the LISTED rows, row_listed), and get_Quad_for_Pose_Solution skips the rows whose keyframe mate is not a true positive
 * (kf_is_tp, :78).  The selected quads are all quads of the rows that are listed and TP; the rank order is (row length, KF
 * index, candidate index) restricted to them, top_n = (size_t)(top_rank_fraction * n_selected), and n_selected is the
 * denominator of the inlier ratio.  The selected rows are compacted on the device and the search of ebvo_pose_from_quads
 * runs on the compacted arrays.
 * Status 1 (identity pose, no search kernel launched, no random number drawn): fewer than 2 listed rows (the reference's own
 * quads_by_kf.size() < 2, :177), fewer than 2 selected quads, or top_n < 2.
 * row_listed / kf_is_tp: n_kf bytes each, NULL = all set.  res->n_quads is the selected count; best_q1 / best_q2 are positions
 * in the selected rank order.  inlier (n bytes) and quad_geom (n x 12) are in the full CSR order, zero on quads not selected;
 * rank_order (n) holds full-CSR indices in rank order, -1 beyond n_selected.  quad_geom and rank_order are left untouched
 * when status = 1.  With both masks NULL every output equals ebvo_pose_from_quads bit for bit.  Slot 0's stream, as there. */
int ebvo_pose_from_quads_gt(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf, const int32_t *row_ptr,
                            const ebvo_edge *cf_left, const ebvo_edge *cf_right, const uint8_t *row_listed, const uint8_t *kf_is_tp,
                            const ebvo_stereo_calib *cal, const ebvo_pose_params *p, ebvo_pose_result *res, uint8_t *inlier,
                            double *quad_geom, int32_t *rank_order);
/* The same on a slot armed by ebvo_temporal_set_gt after a match with stages = 1: the slot's final quads, its device row_on
 * (a veridical quad and kf_is_tp) and its count of listed rows.  EBVO_ERR_STATE when the slot is not armed, has no final
 * quads, has anything in flight, or the keyframe was replaced.  inlier (may be NULL): n_final bytes.  The slot's results, its
 * armed state and ebvo_temporal_gt_metrics are unchanged. */
int ebvo_temporal_estimate_pose_gt(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_pose_params *p,
                                   ebvo_pose_result *res, uint8_t *inlier);

/* Solution_Constraints_Application (:255-381): recall and precision of the four quad-pair constraints over sampled pairs of
 * the selected quads.  Per run exactly max_iterations index pairs are drawn with the loop's
 * do { rand() % top_n; rand() % top_n } while (equal) -- no termination test, no iteration adjustment -- from the context's
 * generator under the rand_seed / continue_stream rules of the search; run k + 1 continues where run k stopped.
 * "Baseline": veridical = the pairs with both quads veridical, precision = veridical / max_iterations, recall = 1.0.  The
 * Length, T1, T2 and Tangent constraints are applied progressively to the survivors of the stage before:
 * recall = veridical / Baseline's veridical (0 / 0 is the NaN it is), precision = surviving == 0 ? 0 : veridical / surviving.
 * The doubles are formed on the host from the device's integer counts.  A pair of zero length fails the Length constraint.
 * Insufficient quads (the three rules above): every run has status 1, zero counts and doubles, draws = 0; draw_idx and
 * draw_stage are left untouched. */
enum
{
    EBVO_PC_BASELINE = 0, /* "Baseline" */
    EBVO_PC_LENGTH,       /* "Normalized Length Constraint" */
    EBVO_PC_T1,           /* "T1 Angle Similarity Constraint" */
    EBVO_PC_T2,           /* "T2 Angle Similarity Constraint" */
    EBVO_PC_TANGENT,      /* "Tangent Angle Similarity Constraint" */
    EBVO_PC_NUM_STAGES
};
typedef struct ebvo_pose_cascade_stage
{
    int32_t stage, reserved;
    int64_t surviving, veridical; /* pairs that passed every constraint up to this stage; ... with both quads veridical */
    double recall, precision;
} ebvo_pose_cascade_stage;
typedef struct ebvo_pose_cascade_run
{
    int32_t status, reserved; /* 0 ok / 1 insufficient quads */
    int64_t n_quads, top_n, draws;
    ebvo_pose_cascade_stage stages[EBVO_PC_NUM_STAGES];
} ebvo_pose_cascade_run;
/* On host arrays (as ebvo_pose_from_quads_gt).  quad_is_tp: per quad in CSR order (Quad_for_Pose_Solution::b_is_veridical),
 * NULL = none veridical.  runs[n_runs]: one record per run.  draw_idx (may be NULL): n_runs x max_iterations x 2 positions in
 * the selected rank order; draw_stage (may be NULL): n_runs x max_iterations bytes, bits 0-2 the number of constraints the
 * pair passed (0-4), bit 7 set when both quads are veridical.  The ranges of ebvo_pose_params apply, n_runs >= 1 and
 * n_runs x max_iterations <= 1 << 24 (else EBVO_ERR_ARG, nothing touched). */
int ebvo_pose_constraint_metrics(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf, const int32_t *row_ptr,
                                 const ebvo_edge *cf_left, const ebvo_edge *cf_right, const uint8_t *row_listed,
                                 const uint8_t *kf_is_tp, const uint8_t *quad_is_tp, const ebvo_stereo_calib *cal,
                                 const ebvo_pose_params *p, int n_runs, ebvo_pose_cascade_run *runs, int32_t *draw_idx,
                                 uint8_t *draw_stage);
/* The resident twin on an armed slot (as ebvo_temporal_estimate_pose_gt): b_is_veridical is the slot's EBVO_TGT_CLUSTER flag
 * (what ebvo_temporal_gt_flags returns). */
int ebvo_temporal_pose_constraint_metrics(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_pose_params *p,
                                          int n_runs, ebvo_pose_cascade_run *runs, int32_t *draw_idx, uint8_t *draw_stage);

/* ---- inlier refit of the relative pose (this project's own: the reference never fits its best minimal hypothesis) ---- */
/* Gauss-Newton on the reprojection error of BOTH cameras over the inliers of a start pose (usually the search's R, t).  This
 * comment is the arithmetic contract; tests/oracle_pose_refit.py restates it and the device matches it bit for bit.  fp64,
 * no FMA, IEEE division and sqrt; mv3 / dot3 / cross3 are those of csrc/ebvo_geom.h, (a b + c d) + e f.
 * Inputs: the selected quads in CSR order (every quad, or the quads of the rows that are listed and TP, compacted as the
 *   search compacts them), k = 0 .. n - 1; per quad Gamma_k (the keyframe mate's 3-D point, as the search forms it), the CF left
 *   centre u_k and the CF right centre ub_k; the start pose; the calibration with K_right := K_left (K below).
 * Model: RG = mv3(R, Gamma), X = RG + t.  Camera 0: Y = X, A = I, centre u.  Camera 1: Y = mv3(R21, X) + T21, A = R21, centre ub.
 *   p = mv3(K, Y), pi = (p0 / p2, p1 / p2), r = pi - centre, rho = sqrt(rx rx + ry ry).
 *   Huber, delta = huber_px: rho <= delta: w = 1, cost (rho rho) 0.5; else w = delta / rho, cost delta (rho - delta 0.5).
 *   ip = 1 / p2, jx_j = ip (K_0j - pi_x K_2j), jy_j = ip (K_1j - pi_y K_2j); camera 1: jx_j <- (jx_0 A_0j + jx_1 A_1j) + jx_2 A_2j,
 *   the same for jy.  Jacobian rows under R <- Exp(w) R, t <- t + v: Jx = [cross3(RG, jx) | jx], Jy = [cross3(RG, jy) | jy].
 *   The 28 terms of a camera: w (Jx_i Jx_j + Jy_i Jy_j) for i <= j row-major (21), w (Jx_i rx + Jy_i ry) (6), the cost.  A
 *   camera whose rho is not < +inf contributes +0.0 to all 28.  A quad's term is left + right.
 * Sums: virtual lane v = k mod 1024 adds its quads' terms in ascending k from +0.0 (a quad outside the fit set adds +0.0);
 *   within each group of 64 consecutive lanes x[l] += x[l + s], l < s, s = 32 .. 1; the 16 group sums by the same tree,
 *   s = 8 .. 1.  The result depends on no launch geometry.
 * A round: the fit set S = the quads the search's own inlier test accepts under the current pose (max_reproj_error of `p`,
 *   camera 0 only); |S| < 3 ends the refit with stop reason 4.  For it = 0 .. iterations: the 28 sums over S; if it > 0 and
 *   not cost <= cost_prev (NaN included) the previous pose is restored, stop reason 2; if it == iterations, stop reason 1;
 *   H d = -g by Cholesky (L_jj = sqrt(H_jj - sum_k L_jk L_jk), the subtractions in ascending k, a pivot not > 0: stop
 *   reason 3 and the pose is kept; L_ij = (H_ij - sum_k L_ik L_jk) / L_jj; forward and back substitution the same way, k
 *   ascending); R <- Exp(d_0..2) R by the 3 x 3 product in mv3 order with no re-orthonormalisation, t <- t + d_3..5;
 *   max |d| < step_eps: stop reason 0.  `rounds` rounds are run, each re-selecting S under the current pose.
 * Exp(w): th2 = (w0 w0 + w1 w1) + w2 w2; th2 == 0: I.  Else th = sqrt(th2), a = sin(th) / th, sh = sin(th 0.5),
 *   b = (2 (sh sh)) / th2, E = (I + a W) + b (W W) with W = [w]x; both sines from ebvo_sincos (csrc/ebvo_math.h).
 * block_threads is a developer switch: a block of 256 or 512 threads owns virtual lanes v, v + block_threads, ...; same bits. */
typedef struct ebvo_pose_refine_params
{
    int32_t rounds, iterations;    /* 2, 10 */
    double huber_px, step_eps;     /* 1.5 (+inf = least squares), 1e-10 */
    int32_t block_threads, reserved; /* 0 (= 1024), 256, 512 or 1024 */
} ebvo_pose_refine_params;
typedef struct ebvo_pose_refined
{
    double R[9], t[3];
    int32_t status;      /* 0 refined / 1 nothing to fit (fewer than 2 selected quads: nothing launched; or |S| < 3 under the
                            start pose) / 2 the first solve had a non-positive pivot; 1 and 2 return the start pose */
    int32_t stop_reason; /* of the last round run: 0 eps, 1 step cap, 2 cost rose, 3 pivot, 4 |S| < 3 */
    int32_t rounds_run, steps_kept; /* steps applied and not taken back */
    int64_t n_quads, fit_quads /* |S| of the last round */, inliers /* under the returned pose; 0 when nothing was launched */;
    double cost_first, cost_last; /* of the last round that formed its sums: at its first pose and at the last pose it kept */
} ebvo_pose_refined;
void ebvo_pose_refine_default_params(ebvo_pose_refine_params *p);
/* On host arrays, as ebvo_pose_from_quads_gt (row_listed / kf_is_tp: n_kf bytes each, NULL = all set).  `p`: only
 * max_reproj_error is read, the ranges of ebvo_pose_params apply to all of it.  Accepted: 1 <= rounds <= 16,
 * 0 <= iterations <= 100, huber_px > 0 (+inf allowed), step_eps >= 0, no NaN, R0 and t0 finite, block_threads in its set;
 * anything else: EBVO_ERR_ARG, nothing touched.  inlier (may be NULL): n bytes in the full CSR order, 1 = inlier of the
 * returned pose, zero on quads not selected.  Slot 0's stream without touching slot 0's results; the context's rand() stream
 * is not touched. */
int ebvo_pose_refine_from_quads(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf, const int32_t *row_ptr,
                                const ebvo_edge *cf_left, const ebvo_edge *cf_right, const uint8_t *row_listed, const uint8_t *kf_is_tp,
                                const ebvo_stereo_calib *cal, const ebvo_pose_params *p, const ebvo_pose_refine_params *rp,
                                const double R0[9], const double t0[3], ebvo_pose_refined *out, uint8_t *inlier);
/* On the slot's final quads: gt_rows = 0 every quad (the state rules of ebvo_temporal_estimate_pose), gt_rows = 1 the
 * ground-truth rows of an armed slot (those of ebvo_temporal_estimate_pose_gt).  inlier (may be NULL): n_final bytes.  The
 * slot's results, its armed state, ebvo_temporal_gt_metrics and the rand() stream are unchanged. */
int ebvo_temporal_refine_pose(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_pose_params *p,
                              const ebvo_pose_refine_params *rp, const double R0[9], const double t0[3], int gt_rows,
                              ebvo_pose_refined *out, uint8_t *inlier);

/* ---- alignment of the pose to the current frame's TOED edges by normal distance (this project's own stage) ---------- */
/* ICP on curves: the keyframe mates' 3-D points are projected under the pose, each projection is associated with the
 * nearest current-frame TOED edge of compatible orientation, and the distance ALONG THAT EDGE'S NORMAL is minimised over the
 * pose, re-associating as the pose moves.  It needs no quad: only the keyframe mates and the TOED edge lists of the current
 * frame.  This comment is the arithmetic contract; tests/oracle_align.py restates it and the device matches it bit for bit.
 * fp64, no FMA, IEEE division and sqrt; mv3 / cross3 of csrc/ebvo_geom.h; sines and cosines through ebvo_sincos, atan2
 * through ebvo_atan2 (csrc/ebvo_math.h).
 * Inputs: the keyframe mates kf_left[i], kf_right[i], i < n_kf; the calibration; the kept TOED edges of the current frame's
 *   left image E0[j], j < n0, and (cameras = 2) of its right image E1[j], j < n1; the frame's size w x h; a start pose in the
 *   convention of the pose search (Gc = R Gamma + t in the left camera).
 * Cameras: camera 0 is K_left; camera 1 sits at (R21, T21) with the TRUE K_right of `cal`.  This is the projection of the
 *   pose prior (ebvo_temporal_set_prior) and NOT the pose search's and the refit's K_right := K_left: the residuals are taken
 *   against real right-image TOED edges, which lie where the true right camera saw them.
 * Per mate: Gamma and the unit 3-D tangent T1 from stereo_gamma_tangent under (K_left^-1, K_right^-1, R21, T21), as the
 *   prior's projection forms them.
 * Association of a round under the pose (R, t), per mate i and camera c: Gc = mv3(R, Gamma) + t; camera 0: Y = Gc, M = R;
 *   camera 1: Y = mv3(R21, Gc) + T21, M = R21 R (3 x 3 product in mv3 order).  p = mv3(K_c, Y), q = (p0 / p2, p1 / p2),
 *   g = (q0, q1, p2 / p2) with q taken over its own third component as the prior does, ray = mv3(K_c^-1, g), T2 = mv3(M, T1),
 *   t2 = T2 - T2_z ray normalised when its squared norm is > 0, o = ebvo_atan2(t2_y, t2_x).  The term is LIVE iff
 *   img_margin < q_x < w - img_margin, img_margin < q_y < h - img_margin and Y_z > 0 (NaN, +-inf: not live) -- per camera,
 *   not jointly.  Grid: gw = ceil(w / cell_size), gh = ceil(h / cell_size); edge e is in cell ((int)e.x / cell_size,
 *   (int)e.y / cell_size) iff both lie in [0, gw) x [0, gh) (C division: e.x in (-cell_size, 0) is column 0; NaN and +-inf are
 *   in no cell).  sr = ceil(radius / cell_size).  A live term's candidates are the edges e of E_c in the cells within sr of
 *   q's cell (clipped to the grid) with orient_close(o, e.theta, orient_thr_deg) (|o - theta| in degrees folded at 180, within
 *   the threshold of 0 or 180) and d2 = dx dx + dy dy <= radius radius, dx = e.x - q_x, dy = e.y - q_y.  It takes the
 *   candidate with the smallest (d2, j) in lexicographic order -- no traversal order enters -- or is not associated.
 * Residual of an associated term: (sn, cs) = ebvo_sincos(e.theta), n = (sn, -cs) (the reference's patch-shift normal,
 *   src/utility.cpp:82-93); with pi, ip, jx, jy and Jx, Jy as the refit above forms them for that camera under K_c:
 *   r = n0 (pi_x - e.x) + n1 (pi_y - e.y); rho = |r|; Huber with delta = huber_px by the refit's formulas; J_k = n0 Jx_k +
 *   n1 Jy_k.  The 28 terms: w (J_i J_j), i <= j row-major (21), w (J_i r) (6), the cost.  A term that is not associated, or
 *   whose rho is not < +inf, is +0.0 in all 28.  A mate's term is camera 0 + camera 1.
 * Sums: mates are cut into tiles of 1024 consecutive indices; in a tile lane l holds +0.0 + the term of mate 1024 tile + l
 *   (+0.0 past n_kf); each group of 64 lanes by the halving tree x[l] += x[l + s], s = 32 .. 1, the 16 group sums by the same
 *   tree, s = 8 .. 1; the tile sums are added in ascending tile index from +0.0.  No launch geometry or arrival order enters.
 * A round: associate under the current pose; A = the associated terms of both cameras.  A < min_terms: stop reason 4, pose
 *   kept, the call ends.  Else, with the associations FIXED, the refit's loop: for it = 0 .. iterations the sums; it > 0 and
 *   not cost <= cost_prev: previous pose restored, stop reason 2; it == iterations: stop reason 1; Cholesky as in the refit, a
 *   pivot not > 0: stop reason 3, pose kept, the call ends; R <- Exp(d_0..2) R, t <- t + d_3..5; max |d| < step_eps: stop
 *   reason 0.  `rounds` rounds are run, each re-associating; reasons 0, 1, 2 go on to the next round.
 * After the last round one more association under the returned pose gives assoc_left / assoc_right (edge index or -1),
 *   n_assoc, inliers (associated terms with |r| < inlier_px) and rms_normal = sqrt(S / (n_assoc[0] + n_assoc[1])), S the sum
 *   of r r (camera 0 + camera 1 per mate, +0.0 for a term that is not associated or whose rho is not < +inf) through the same tile trees; 0 when nothing
 *   is associated.
 * block_threads is a developer switch as in the refit: 256 or 512 threads own lanes l, l + block_threads, ...; same bits. */
typedef struct ebvo_align_params
{
    int32_t rounds, iterations;      /* 4, 10 */
    double radius;                   /* 4.0 px: association radius */
    int32_t cell_size, min_terms;    /* 4 px; 12 associated terms at least */
    double orient_thr_deg;           /* 10 */
    double huber_px, inlier_px;      /* 1.0 (+inf = least squares), 1.0 */
    double step_eps;                 /* 1e-10 */
    double img_margin;               /* 10: TOED keeps nothing nearer than 10 px to the border */
    int32_t cameras, block_threads;  /* 2 (1 = left image only); 0 (= 1024), 256, 512 or 1024 */
} ebvo_align_params;
typedef struct ebvo_aligned_pose
{
    double R[9], t[3];
    int32_t status;      /* 0 aligned / 1 nothing to fit (n_kf = 0, no edges: nothing launched; or A < min_terms under the
                            start pose) / 2 the first solve hit a non-positive pivot; 1 and 2 return the start pose */
    int32_t stop_reason; /* of the last round run: 0 eps, 1 step cap, 2 cost rose, 3 pivot, 4 A < min_terms */
    int32_t rounds_run, steps_kept;
    int32_t n_kf, fit_terms; /* fit_terms: A of the last round run */
    int32_t n_assoc[2];      /* associated terms per camera under the returned pose */
    int64_t inliers;
    double cost_first, cost_last; /* of the last round that formed its sums */
    double rms_normal;
} ebvo_aligned_pose;
void ebvo_align_default_params(ebvo_align_params *p);
/* On host arrays.  cf_edges_right may be NULL with cameras = 1 (it and n1 are then ignored).  Accepted: 1 <= rounds <= 16,
 * 0 <= iterations <= 100, radius finite and > 0, cell_size >= 1 with ceil(radius / cell_size) <= 8, orient_thr_deg >= 0,
 * huber_px > 0 (+inf allowed), inlier_px >= 0, step_eps >= 0, min_terms >= 6, img_margin >= 0, cameras 1 or 2, block_threads
 * in its set, no NaN, R0 and t0 finite, img_w, img_h >= 1 with a grid of at most 2^26 cells; anything else: EBVO_ERR_ARG,
 * nothing touched.  assoc_left / assoc_right (may be NULL): n_kf int32 each (assoc_right all -1 with cameras = 1).  Runs on
 * slot 0's stream without touching slot 0's results; EBVO_ERR_STATE while slot 0 has work in flight.  The inputs are copied
 * before the call returns. */
int ebvo_pose_align_edges(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf, const ebvo_edge *cf_edges_left,
                          int n0, const ebvo_edge *cf_edges_right, int n1, int img_w, int img_h, const ebvo_stereo_calib *cal,
                          const ebvo_align_params *params, const double R0[9], const double t0[3], ebvo_aligned_pose *out,
                          int32_t *assoc_left, int32_t *assoc_right);
/* The context's keyframe mates against the kept TOED edge lists the slot's pair left resident.  Needs a keyframe and a pair
 * on the slot whose ebvo_stereo_wait has returned -- neither finalisation nor a temporal match; EBVO_ERR_STATE otherwise, or
 * while anything of the slot is in flight.  The slot's pair, final mates, quads, ground-truth state, prior and the context's
 * rand() stream are unchanged. */
int ebvo_temporal_align_pose(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_align_params *params,
                             const double R0[9], const double t0[3], ebvo_aligned_pose *out, int32_t *assoc_left,
                             int32_t *assoc_right);
/* What that call would work on: the keyframe's mates (the length assoc_left / assoc_right need) and the slot's kept TOED
 * edges per image.  The same state rules. */
int ebvo_temporal_align_size(ebvo_ctx *ctx, int slot, int32_t *n_kf, int32_t *n_left, int32_t *n_right);

/* ---- refinement of the keyframe mates' depths from aligned frames: inverse-depth filter (this project's own stage) --- */
/* Every frame aligned to the keyframe sees the keyframe's curve points again: its left camera at a temporal baseline, its
 * right camera at the rig's.  Per keyframe mate one scalar is filtered: lambda, the ratio of the triangulated depth to the
 * refined one, so that the refined point is Gamma / lambda.  This comment is the arithmetic contract; tests/oracle_depth.py
 * restates it and the device matches it bit for bit.  fp64, no FMA, IEEE division and sqrt; mv3 / mtv3 / dot3 of
 * csrc/ebvo_geom.h; sines and cosines through ebvo_sincos.  Additive: the ABI version stays 6.
 * State per mate i: lambda_i (1.0 at the prior), info_i (1 / variance of lambda_i), n_obs_i (int32: frames fused),
 *   flags_i (uint8, written by every update: EBVO_DEPTH_* of that update alone).
 * Per mate: Gamma and T1 exactly as the alignment's align_prepare_kernel forms them (stereo_gamma_tangent under K_left^-1,
 *   K_right^-1, R21, T21).  A mate is DEAD iff a component of Gamma is not finite or Gamma_z is not > 0: flag DEAD, counted in
 *   n_dead and in nothing else; its state passes through unchanged (from the prior: lambda 1.0, info +0.0, n_obs 0).
 * Prior of a live mate (used when no in-state is given): b = sqrt(dot3(T21, T21)), s = (sigma_disp_px Gamma_z) / (K_left[0] b),
 *   info0 = 1.0 / (s s); lambda 1.0, n_obs 0.
 * Refined point: Gs = (Gamma_x / lambda, Gamma_y / lambda, Gamma_z / lambda), three divisions.
 * One camera's term at lambda under the pose (R, t), for the edge e = E_c[a] the association a names (0 <= a < n_c; any
 *   other value, a NULL association array, or camera 1 with cameras = 1: no term): RG = mv3(R, Gs), X = RG + t; camera 0:
 *   Y = X, K = K_left; camera 1: Y = mv3(R21, X) + T21, K = the TRUE K_right (as the alignment).  p = mv3(K, Y), pi = (p0 / p2,
 *   p1 / p2), ip = 1.0 / p2, jx_k = ip (K[k] - pi_x K[6 + k]), jy_k = ip (K[3 + k] - pi_y K[6 + k]), k < 3; camera 1:
 *   jx <- mtv3(R21, jx), jy <- mtv3(R21, jy).  (sn, cs) = ebvo_sincos(e.theta), n = (sn, -cs).
 *   r = n0 (pi_x - e.x) + n1 (pi_y - e.y); m_k = n0 jx_k + n1 jy_k; j = -(dot3(m, RG) / lambda): d r / d lambda, because
 *   d Gs / d lambda = -Gs / lambda.
 * One update of a live mate with the incoming (lambda_in, info_in, n_obs_in):
 *   1. both terms at lambda_in.  A term is LIVE iff it exists and img_margin < pi_x < w - img_margin, img_margin < pi_y <
 *      h - img_margin and Y_z > 0 (per camera; NaN: not live).  A term that is not live is no term.
 *   2. gate: a live term SURVIVES iff |r| <= gate_px and |r| < +inf; otherwise it is dropped for the whole update, counted in
 *      n_gated[c], flag GATED_LEFT / GATED_RIGHT.  The set of surviving terms is fixed here.  n_terms[c] counts them.
 *   3. lambda = lambda_in; iv = 1.0 / (sigma_normal_px sigma_normal_px).  For it = 0 .. iterations: the surviving terms at
 *      lambda; rho = |r|, w = 1.0 if rho <= huber_px else huber_px / rho (the refit's Huber weight); Sh = +0.0, Sg = +0.0; camera 0
 *      then camera 1, surviving only: Sh = Sh + w (j j), Sg = Sg + w (j r); h = info_in + Sh iv; if it == iterations: stop;
 *      g = info_in (lambda - lambda_in) + Sg iv; lambda = lambda - g / h.  (iterations + 1 evaluations; the last forms h and
 *      the outgoing residuals only.  iterations = 0 updates info alone.)
 *   4. accept iff lambda is finite, lambda_min <= lambda <= lambda_max, at least one term survived and h is finite:
 *      lambda_i = lambda, info_i = min(h, info_max) (h if it is the smaller, else info_max), n_obs_i = n_obs_in + 1, flag
 *      UPDATED, n_updated.  Otherwise the incoming state is written back, flag RESTORED, n_restored.
 * rms_before = sqrt(Sb / (n_terms[0] + n_terms[1])), Sb the sum over the mates of +0.0 + ((r0 r0 or +0.0) + (r1 r1 or +0.0)),
 *   the surviving terms' residuals at lambda_in (+0.0 for a dead mate), through the alignment's tile trees: tiles of 1024
 *   mates, a 64-lane halving tree, the 16 group sums by the same tree, tiles added in ascending order from +0.0.  rms_after:
 *   the same with the residuals at the outgoing lambda (an accepted mate: the last evaluation; a restored one: those at
 *   lambda_in).  Both 0.0 when no term survived.  No launch geometry enters; the counts are integers.
 * block_threads is the alignment's developer switch. */
#define EBVO_DEPTH_DEAD 1u
#define EBVO_DEPTH_UPDATED 2u
#define EBVO_DEPTH_RESTORED 4u
#define EBVO_DEPTH_GATED_LEFT 8u
#define EBVO_DEPTH_GATED_RIGHT 16u
typedef struct ebvo_depth_params
{
    double sigma_disp_px;            /* 0.25 px: the disparity noise the prior stands for */
    double sigma_normal_px;          /* 0.5 px: noise of one normal residual */
    double huber_px, gate_px;        /* 1.0 (+inf = least squares), 3.0 (+inf = only non-finite residuals are dropped) */
    int32_t iterations, cameras;     /* 3; 2 (1 = left image only) */
    double lambda_min, lambda_max;   /* 0.25, 4.0 */
    double info_max;                 /* 1e6: sigma(lambda) never below 1e-3 (+inf = no clip) */
    double img_margin;               /* 10, as the alignment */
    int32_t block_threads, reserved; /* 0 (= 1024), 256, 512 or 1024; 0 */
} ebvo_depth_params;
typedef struct ebvo_depth_refined
{
    int32_t n_kf, n_dead, n_updated, n_restored;
    int32_t n_terms[2], n_gated[2];
    double rms_before, rms_after;
} ebvo_depth_refined;
void ebvo_depth_default_params(ebvo_depth_params *p);
/* One update on host arrays.  assoc_left / assoc_right: n_kf int32 each as ebvo_pose_align_edges returns them (assoc_right
 * and cf_edges_right may be NULL with cameras = 1, either association array may be NULL: no term in that camera).
 * lambda_in / info_in / n_obs_in: the incoming state, all three or none (none: the prior).  lambda / info / n_obs / flags: the
 * outgoing state, all four required when n_kf > 0; they may be the incoming arrays.  Accepted: sigma_disp_px, sigma_normal_px
 * finite and > 0, huber_px > 0 and gate_px > 0 (+inf allowed), 0 <= iterations <= 16, 0 < lambda_min <= lambda_max finite,
 * info_max > 0 (+inf allowed), img_margin >= 0, cameras 1 or 2, block_threads in its set, reserved 0, no NaN, R and t finite,
 * img_w, img_h >= 1; anything else: EBVO_ERR_ARG, nothing touched.  n_kf = 0: nothing launched, a zero record.  Runs on slot
 * 0's stream under the state rules of ebvo_pose_align_edges; the inputs are copied before the call returns. */
int ebvo_depth_refine_edges(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf, const ebvo_edge *cf_edges_left,
                            int n0, const ebvo_edge *cf_edges_right, int n1, const int32_t *assoc_left, const int32_t *assoc_right,
                            int img_w, int img_h, const ebvo_stereo_calib *cal, const ebvo_depth_params *params, const double R[9],
                            const double t[3], const double *lambda_in, const double *info_in, const int32_t *n_obs_in, double *lambda,
                            double *info, int32_t *n_obs, uint8_t *flags, ebvo_depth_refined *out);
/* Resident: the keyframe's mates are associated under (R, t) with the slot's kept TOED edge lists by the alignment's own grid
 * and association (radius, cell_size, orient_thr_deg, img_margin of align_params; its other fields are checked and not used;
 * cameras is depth_params'), on Gamma / lambda with the keyframe's CURRENT lambda whether ebvo_temporal_use_depth is on or
 * not (the update linearises there); then one update of the keyframe's resident state.  Everything is enqueued up front.  The
 * state rules of ebvo_temporal_align_pose; the slot's pair, quads, prior, ground-truth state and the rand() stream are
 * unchanged. */
int ebvo_temporal_refine_depth(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_align_params *align_params,
                               const ebvo_depth_params *depth_params, const double R[9], const double t[3], ebvo_depth_refined *out);
/* The keyframe's state: n_kf values each (any pointer may be NULL).  A keyframe that has fused no frame is AT THE PRIOR and
 * reads lambda 1.0, info +0.0 (info0 is formed by the first update, from its parameters), n_obs 0, flags 0.
 * EBVO_ERR_STATE without a keyframe. */
int ebvo_temporal_depth_fetch(ebvo_ctx *ctx, double *lambda, double *info, int32_t *n_obs, uint8_t *flags);
/* Back to the prior.  ebvo_temporal_set_keyframe does the same, and no other call does. */
int ebvo_temporal_depth_reset(ebvo_ctx *ctx);
/* on != 0: ebvo_temporal_align_pose works on Gamma / lambda of the live mates (one small launch over the prepared planes; a
 * keyframe at the prior is lambda = 1 and the launch is left out).  Default off: the existing calls enqueue exactly what they
 * enqueue without this stage.  The pose search, the refit and the prior's projection never read lambda. */
int ebvo_temporal_use_depth(ebvo_ctx *ctx, int on);
/* ebvo_pose_align_edges on Gamma / lambda: lambda [n_kf] (NULL: the bits of ebvo_pose_align_edges). */
int ebvo_pose_align_edges_depth(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, const double *lambda, int n_kf,
                                const ebvo_edge *cf_edges_left, int n0, const ebvo_edge *cf_edges_right, int n1, int img_w, int img_h,
                                const ebvo_stereo_calib *cal, const ebvo_align_params *params, const double R0[9], const double t0[3],
                                ebvo_aligned_pose *out, int32_t *assoc_left, int32_t *assoc_right);

/* ---- handover of the refined depths to the next keyframe on promotion (this project's own stage) -------------------- */
/* When the current frame becomes the keyframe, the old keyframe's refined depths are carried to the new keyframe's mates
 * through the known relative pose: each old mate is projected into the new frame, each new mate GATHERS the nearest old
 * projection of compatible orientation, and the depth it predicts is fused, as a second independent measurement, with the
 * new mate's own triangulation prior.  This comment is the arithmetic contract; tests/oracle_carry.py restates it and the
 * device matches it bit for bit.  fp64, no FMA, IEEE division and sqrt; mv3 / dot3 of csrc/ebvo_geom.h; ebvo_sincos and
 * ebvo_atan2 of csrc/ebvo_math.h.  Additive: the ABI version stays 6.
 * Inputs: the old keyframe's mates kf_left[i], kf_right[i], i < n_old, with their state (lambda_i, info_i, n_obs_i); the new
 *   keyframe's mates new_left[m], new_right[m], m < n_new (the final mates of the frame being promoted); that frame's size
 *   w x h; the calibration; the pose (R, t) from the old keyframe to the new frame in the convention of the pose search
 *   (Gc = R Gamma + t in the left camera).
 * Old mate i: Gamma and T1 exactly as the alignment's align_prepare_kernel forms them.  It is a SOURCE iff every component of
 *   Gamma is finite and Gamma_z > 0, lambda_i is finite and > 0, info_i > 0 and n_obs_i >= min_obs.  Of a source, in this
 *   order: Gs = Gamma / lambda_i (three divisions); RG = mv3(R, Gs); X = RG + t; q and o: the projection and the mapped
 *   orientation by the alignment's camera-0 formulas (p = mv3(K_left, X), q = p / p2, ray = mv3(K_left^-1, (q0 / q2, q1 / q2,
 *   q2 / q2)), T2 = mv3(R, T1), t2 = T2 - T2_z ray normalised when its squared norm is > 0, o = ebvo_atan2(t2_y, t2_x));
 *   zp = X_z; a = RG_z / (zp lambda_i).  A source is LIVE by the alignment's camera-0 test against the new frame's size:
 *   img_margin < q_x < w - img_margin, img_margin < q_y < h - img_margin and zp > 0 (NaN, +-inf: not live).
 * New mate m: Gamma' by the same geometry.  It is DEAD by the filter's rule (a component of Gamma' not finite, or Gamma'_z not
 *   > 0): lambda 1.0, info +0.0, n_obs 0, flag EBVO_DEPTH_DEAD, src_index -1.  A live mate's prior is the filter's:
 *   b = sqrt(dot3(T21, T21)), s' = (sigma_disp_px Gamma'_z) / (K_left[0] b), info0' = 1.0 / (s' s').
 * Association (a gather: the new mate looks for old projections, so no two sources ever write the same state).  The grid is
 *   the alignment's (cell_size; a projection is in cell ((int)q_x / cell_size, (int)q_y / cell_size) by grid_cell's rule),
 *   built over the live sources' projections.  With e = new_left[m]: the candidates of a live mate m are the live sources i
 *   in the cells within ceil(radius / cell_size) of e's cell (by the same rule; a mate whose e.x or e.y is in no cell has no
 *   candidate), clipped to the grid, with
 *   orient_close(o_i, e.theta, orient_thr_deg) and d2 = dx dx + dy dy <= radius radius, dx = q_x - e.x, dy = q_y - e.y.
 *   The mate takes the smallest (d2, i) in lexicographic order -- no traversal order enters -- or none.  src_index[m] = i,
 *   or -1.
 * Fusion of an associated live mate: lm = Gamma'_z / zp_i (the ratio of the new triangulated depth to the one the old
 *   keyframe predicts: the new mate's lambda as the old keyframe measures it); c = lm a_i (d lm / d lambda_i up to sign);
 *   im = (carry info_i) / (c c).  If im is not finite or not > 0 the mate is treated as gated.  Gate: d = lm - 1.0,
 *   v = 1.0 / info0' + 1.0 / im; accepted iff lambda_min <= lm <= lambda_max and d d <= (gate_sigmas gate_sigmas) v.
 *   Accepted: h = info0' + im; lambda' = (info0' + im lm) / h; info' = min(h, info_max) (h if it is the smaller, else
 *   info_max); n_obs' = n_obs_i; flag EBVO_DEPTH_CARRIED.  Gated: the prior (1.0, info0', 0), flag EBVO_DEPTH_CARRY_GATED.
 *   Not associated: the prior, flags 0.
 * The record counts: n_sources, n_live (of the old mates; both 0 when no association is launched), n_dead (new mates),
 *   n_assoc = n_carried + n_gated.  Integers only; no launch geometry enters anything. */
#define EBVO_DEPTH_CARRIED 32u
#define EBVO_DEPTH_CARRY_GATED 64u
typedef struct ebvo_depth_carry_params
{
    double sigma_disp_px;          /* 0.25 px: the disparity noise the new mate's prior stands for (the filter's) */
    double radius;                 /* 1.5 px: an old projection further from the new mate's left edge is another curve point */
    int32_t cell_size, min_obs;    /* 4 px; 1: an old mate that fused fewer frames has nothing to hand over (>= 0) */
    double orient_thr_deg;         /* 10 */
    double carry;                  /* 0.5, in (0, 1]: discount of the carried information for pose and association error */
    double gate_sigmas;            /* 3 (> 0, +inf = no chi gate) */
    double lambda_min, lambda_max; /* 0.25, 4.0 */
    double info_max;               /* 1e6 (+inf = no clip) */
    double img_margin;             /* 10, as the alignment */
    int32_t reserved, pad;         /* 0, 0 */
} ebvo_depth_carry_params;
typedef struct ebvo_depth_carried
{
    int32_t n_old, n_sources, n_live, n_new, n_dead, n_assoc, n_carried, n_gated;
} ebvo_depth_carried;
void ebvo_depth_carry_default_params(ebvo_depth_carry_params *p);
/* On host arrays.  lambda_in / info_in / n_obs_in: the old mates' state, all three or none.  lambda / info / n_obs / flags /
 * src_index: n_new values each, all five required when n_new > 0.  A NULL in-state, n_old = 0 or n_new = 0 launches no
 * association: every live new mate is at its prior.  Accepted: sigma_disp_px and radius finite and > 0, cell_size >= 1 with
 * ceil(radius / cell_size) <= 8, orient_thr_deg >= 0, 0 < carry <= 1, gate_sigmas > 0 (+inf allowed), min_obs >= 0,
 * 0 < lambda_min <= lambda_max finite, info_max > 0 (+inf allowed), img_margin >= 0, reserved 0, no NaN, R and t finite,
 * img_w, img_h >= 1 with a grid of at most 2^26 cells; anything else: EBVO_ERR_ARG, nothing touched.  Runs on slot 0's stream
 * under the state rules of ebvo_pose_align_edges; the inputs are copied before the call returns. */
int ebvo_depth_carry(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_old, const double *lambda_in,
                     const double *info_in, const int32_t *n_obs_in, const ebvo_edge *new_left, const ebvo_edge *new_right, int n_new,
                     int img_w, int img_h, const ebvo_stereo_calib *cal, const ebvo_depth_carry_params *params, const double R[9],
                     const double t[3], double *lambda, double *info, int32_t *n_obs, uint8_t *flags, int32_t *src_index,
                     ebvo_depth_carried *out);
/* The slot's finalised pair becomes the keyframe and inherits the old keyframe's refined depths: the carried state is
 * computed first, into buffers of the call's own, from the old keyframe's mates, its resident state and the slot's final
 * mates; then the slot is installed as ebvo_temporal_set_keyframe installs it (the same store, the same bits); then the
 * carried state is installed, so that the new keyframe is NOT at the prior.  Needs a keyframe besides what
 * ebvo_temporal_set_keyframe needs; its refusals otherwise: EBVO_ERR_STATE while the CALLED slot has work in flight (a pair,
 * a finalisation or a match) and while ANY slot has a temporal match in flight.  A stereo pair or a finalisation in flight in
 * another slot does not refuse it: a frame loop promotes while the next pair's chain runs.  An old keyframe still at the prior
 * has nothing to carry: the call then is ebvo_temporal_set_keyframe, the record holds n_old and n_new and zeros, and the new
 * keyframe is at the prior.  On any refusal the old keyframe and its state stay as they were.  Pending priors are dropped and
 * the keyframe generation is bumped, as by ebvo_temporal_set_keyframe.  The decision to switch stays the caller's. */
int ebvo_temporal_promote_keyframe(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_depth_carry_params *params,
                                   const double R[9], const double t[3], ebvo_depth_carried *out);
/* src_index of the last promotion: n_kf int32 (all -1 when the old keyframe had nothing to carry).  EBVO_ERR_STATE when the
 * keyframe was not installed by a promotion. */
int ebvo_temporal_depth_source(ebvo_ctx *ctx, int32_t *src_index);

/* ---- keyframe coverage, a switch policy and a frame step (this project's own stage) ---------------------------------- */
/* How much of the keyframe still explains the current frame, and how much of the current frame the keyframe does not
 * explain: the measurement a caller needs to decide when to switch keyframes.  This comment is the arithmetic contract;
 * tests/oracle_cover.py restates it and the device matches it bit for bit.  fp64, no FMA, IEEE division and sqrt; mv3 of
 * csrc/ebvo_geom.h; ebvo_sincos and ebvo_atan2 of csrc/ebvo_math.h.  Camera 0 only: a keyframe decision is about the left
 * image.  Additive: the ABI version stays 6.
 * Inputs: the keyframe's mates kf_left[i], kf_right[i], i < n_kf; lambda [n_kf] or NULL (NULL: the triangulated Gamma, as
 *   ebvo_pose_align_edges_depth treats it); the current frame's kept LEFT edge list E0[j], j < n0; its size w x h; the
 *   calibration; a pose (R, t) in the convention of the pose search (Gc = R Gamma + t in the left camera).
 * Mate i: Gamma exactly as the alignment's align_prepare_kernel forms it.  The mate is DEAD by the filter's rule (a component
 *   of Gamma not finite, or Gamma_z not > 0): flags EBVO_COVER_DEAD alone, assoc -1, disp NaN, and nothing below applies to
 *   it.  Of a live mate, with lambda given, Gs = Gamma / lambda_i (three divisions, the rule of the filter's scaling step),
 *   else Gs = Gamma; RG = mv3(R, Gs); X = RG + t; p = mv3(K_left, X), q = p / p2.  It is IN FRAME by the alignment's camera-0
 *   test: img_margin < q_x < w - img_margin, img_margin < q_y < h - img_margin and X_z > 0 (NaN, +-inf: not in frame).
 * Association: the alignment's own, camera 0, under (R, t), with radius, cell_size, orient_thr_deg and img_margin: the mapped
 *   orientation, the grid over E0, the candidates and the pick of the smallest (d2, j) are those of ebvo_pose_align_edges
 *   (one association, no step).  assoc[i] = j or -1; only a mate in frame can be associated.
 * Residual of an associated mate, as the alignment forms it: (sn, cs) = ebvo_sincos(E0[j].theta), n = (sn, -cs),
 *   r = n_0 (q_x - E0[j].x) + n_1 (q_y - E0[j].y).  It is an INLIER iff |r| < inlier_px (strict; NaN: not).
 * Displacement of a mate in frame from its keyframe position: dx = q_x - kf_left[i].x, dy = q_y - kf_left[i].y,
 *   d = sqrt(dx dx + dy dy); disp[i] = d (NaN for a mate that is not in frame).  b = d / bin_px; the mate counts in bin 63 of
 *   hist if b >= 63.0, else in bin (int)b.  disp_median_bin is the smallest b with 2 (hist[0] + .. + hist[b]) >= n_in_frame,
 *   or -1 when n_in_frame = 0.
 * Current edge j: explained[j] = 1 iff some (live) mate's association is j, else 0; n_explained counts them (two mates on
 *   one edge count once).
 * Coarse cells: cw = ceil(w / cover_cell), ch = ceil(h / cover_cell); edge j is in cell ((int)x / cover_cell,
 *   (int)y / cover_cell) by grid_cell's rule (x in (-cover_cell, cw cover_cell), likewise y; NaN and +-inf are in no cell).
 *   cell_edges[c] counts the edges of E0 in cell c = cy cw + cx, cell_explained[c] the explained ones.  n_cells_cur: cells
 *   with cell_edges >= min_cell_edges; n_cells_covered: those of them with cell_explained >= min_cell_explained.
 * n_kf = 0 or n0 = 0 launches nothing: the record is zero except n_kf, n_edges, cw, ch, with disp_median_bin = -1; flags 0,
 *   assoc -1, disp NaN, explained and both cell planes 0.
 * Everything in the record is an integer: no launch geometry or arrival order enters anything. */
#define EBVO_COVER_DEAD 1u
#define EBVO_COVER_IN_FRAME 2u
#define EBVO_COVER_ASSOCIATED 4u
#define EBVO_COVER_INLIER 8u
#define EBVO_COVER_BINS 64
typedef struct ebvo_cover_params
{
    double radius;         /* 4.0 px: the alignment's value and rule */
    double orient_thr_deg; /* 10: the alignment's */
    double img_margin;     /* 10: the alignment's */
    double inlier_px;      /* 1.0 (>= 0, +inf allowed) */
    double bin_px;         /* 1.0 px per displacement bin (finite, > 0) */
    int32_t cell_size;     /* 4 px: the alignment's grid */
    int32_t cover_cell;    /* 32 px: the coarse cells (>= 1, at most 2^26 of them) */
    int32_t min_cell_edges, min_cell_explained; /* 4, 2 (>= 1 each) */
    int32_t reserved, pad; /* 0, 0 */
} ebvo_cover_params;
typedef struct ebvo_keyframe_cover
{
    int32_t n_kf, n_dead, n_in_frame, n_assoc, n_inliers;
    int32_t n_edges, n_explained;
    int32_t cw, ch, n_cells_cur, n_cells_covered;
    int32_t disp_median_bin;
    int32_t hist[EBVO_COVER_BINS];
} ebvo_keyframe_cover;
void ebvo_cover_default_params(ebvo_cover_params *p);
/* On host arrays.  flags (uint8) / assoc (int32) / disp (double): n_kf values each; explained (uint8): n0; cell_edges /
 * cell_explained (int32): cw ch each; every one of the six may be NULL.  Accepted: radius finite and > 0, cell_size >= 1
 * with ceil(radius / cell_size) <= 8, orient_thr_deg >= 0, img_margin >= 0, inlier_px >= 0 (+inf allowed), bin_px finite and
 * > 0, cover_cell >= 1, min_cell_edges >= 1, min_cell_explained >= 1, reserved and pad 0, no NaN, R and t finite, img_w,
 * img_h >= 1 with at most 2^26 cells in either grid; anything else: EBVO_ERR_ARG, nothing touched.  Runs on slot 0's stream
 * under the state rules of ebvo_pose_align_edges; the inputs are copied before the call returns. */
int ebvo_keyframe_cover_edges(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, const double *lambda, int n_kf,
                              const ebvo_edge *cf_edges_left, int n0, int img_w, int img_h, const ebvo_stereo_calib *cal,
                              const ebvo_cover_params *params, const double R[9], const double t[3], ebvo_keyframe_cover *out,
                              uint8_t *flags, int32_t *assoc, double *disp, uint8_t *explained, int32_t *cell_edges,
                              int32_t *cell_explained);
/* The same on the context's keyframe and the slot's resident kept left edge list, with the keyframe's current lambda iff
 * ebvo_temporal_use_depth is on (a keyframe at the prior: NULL, the same bits).  State rules: ebvo_temporal_align_pose's.
 * The slot's pair, final mates, quads, prior, ground-truth state, the depth state and the rand() stream are unchanged. */
int ebvo_temporal_keyframe_cover(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_cover_params *params,
                                 const double R[9], const double t[3], ebvo_keyframe_cover *out, uint8_t *flags, int32_t *assoc,
                                 double *disp, uint8_t *explained, int32_t *cell_edges, int32_t *cell_explained);
/* The sizes of that call's arrays: n_kf mates, n0 kept left edges, cw x ch coarse cells (params: cover_cell >= 1 is read). */
int ebvo_temporal_cover_size(ebvo_ctx *ctx, int slot, const ebvo_cover_params *params, int32_t *n_kf, int32_t *n0, int32_t *cw,
                             int32_t *ch);

/* The policy: a pure host function of the record's integers.  Each reason is the stated comparison, the share products
 * formed as (double)a < share * (double)b:
 *   EBVO_KF_LOST         n_assoc < min_assoc
 *   EBVO_KF_LOW_OVERLAP  n_in_frame < min_in_frame_share (n_kf - n_dead)
 *   EBVO_KF_LOW_ASSOC    n_assoc < min_assoc_share n_in_frame
 *   EBVO_KF_NEW_CONTENT  n_cells_covered < min_cell_cover n_cells_cur
 *   EBVO_KF_PARALLAX     disp_median_bin >= max_disp_bins
 * Returns 2 (lost) if EBVO_KF_LOST is set, else 1 (switch) if any other bit is set, else 0 (keep); EBVO_ERR_ARG for a NULL
 * record or policy.  *reasons (may be NULL) receives the bits.  The defaults are design choices, not measurements. */
#define EBVO_KF_LOST 1u
#define EBVO_KF_LOW_OVERLAP 2u
#define EBVO_KF_LOW_ASSOC 4u
#define EBVO_KF_NEW_CONTENT 8u
#define EBVO_KF_PARALLAX 16u
typedef struct ebvo_keyframe_policy
{
    int32_t min_assoc;         /* 50 */
    int32_t max_disp_bins;     /* 30 */
    double min_in_frame_share; /* 0.7 */
    double min_assoc_share;    /* 0.5 */
    double min_cell_cover;     /* 0.6 */
} ebvo_keyframe_policy;
void ebvo_keyframe_policy_default(ebvo_keyframe_policy *p);
int ebvo_keyframe_decide(const ebvo_keyframe_cover *cover, const ebvo_keyframe_policy *policy, uint32_t *reasons);

/* The keyframe's pose in the sequence frame, (Rk, tk) with X_kf = Rk X_seq + tk: host state of the context.
 * ebvo_temporal_set_keyframe puts it to the identity (the sequence frame is the last keyframe that was SET rather than
 * promoted); every successful ebvo_temporal_promote_keyframe under (R, t) makes Rk <- R Rk and tk <- mv3(R, tk) + t.  Every
 * entry of the 3 x 3 product is (R_i0 Rk_0j + R_i1 Rk_1j) + R_i2 Rk_2j, one rounding per operation, no FMA: mv3's order per
 * column.  EBVO_ERR_STATE without a keyframe. */
int ebvo_temporal_keyframe_pose(ebvo_ctx *ctx, double R[9], double t[3]);

/* The frame step on a slot whose ebvo_stereo_wait has returned, from the public calls in this order:
 *   (a) ebvo_temporal_align_pose from (R0, t0); a status != 0 ends the step: tracked = 0, decision 2;
 *   (b) with refine_depth, ebvo_temporal_refine_depth under the aligned pose;
 *   (c) ebvo_temporal_keyframe_cover under the aligned pose; (d) ebvo_keyframe_decide;
 *   (e) on decision 1 only: ebvo_stereo_finalize of the slot (with the calibration), then ebvo_temporal_promote_keyframe
 *       under the aligned pose; switched = 1.
 * R_seq = R Rk, t_seq = mv3(R, tk) + t with (R, t) the aligned pose and (Rk, tk) as they were before any switch: the frame's
 * pose in the sequence frame.  A refusal at any stage returns that stage's status and names the stage in failed_stage
 * (EBVO_TRACK_STAGE_*); a failed promotion leaves the old keyframe in place. */
enum
{
    EBVO_TRACK_STAGE_NONE = 0,
    EBVO_TRACK_STAGE_ALIGN = 1,
    EBVO_TRACK_STAGE_DEPTH = 2,
    EBVO_TRACK_STAGE_COVER = 3,
    EBVO_TRACK_STAGE_FINALIZE = 4,
    EBVO_TRACK_STAGE_PROMOTE = 5
};
typedef struct ebvo_track_params
{
    ebvo_align_params align;
    ebvo_depth_params depth;
    ebvo_cover_params cover;
    ebvo_depth_carry_params carry;
    ebvo_finalize_params finalize;
    ebvo_keyframe_policy policy;
    int32_t refine_depth; /* 1 */
    int32_t reserved;     /* 0 */
} ebvo_track_params;
typedef struct ebvo_tracked_frame
{
    ebvo_aligned_pose pose;
    ebvo_depth_refined depth;
    ebvo_keyframe_cover cover;
    ebvo_depth_carried carried;
    ebvo_finalize_counts finalized;
    double R_seq[9], t_seq[3];
    uint32_t reasons;
    int32_t decision, switched, tracked, failed_stage, pad;
} ebvo_tracked_frame;
void ebvo_track_default_params(ebvo_track_params *p);
int ebvo_temporal_track_frame(ebvo_ctx *ctx, int slot, const ebvo_stereo_calib *cal, const ebvo_track_params *params,
                              const double R0[9], const double t0[3], ebvo_tracked_frame *out);

/* ---- ground-truth evaluation from a disparity map (the reference's has_gt() == true branch, is_left = true) ------- */
/* Find_Stereo_GT_Locations (src/Stereo_Matches.cpp:133-200), get_Stereo_Edge_GT_Pairs (:202-268) and
 * Evaluate_Stereo_Edge_Correspondences (:270-379) after every stage of get_Stereo_Edge_Pairs (:1377-1536).
 * Two quirks of the reference are kept: Bilinear_Interpolation<float> (include/utility.h:81-104) divides 0 by 0 at an
 * integer x or y, so such an edge has a NaN disparity and is skipped; and both rays of the GT 3-D point use the LEFT
 * calibration inverse (:179-180).  The pool tests are strict (< pool_dist, :120), the true-positive test is not
 * (<= tp_dist, :305).  Accepted ranges: every tolerance >= 0 and not NaN (+inf allowed); anything else EBVO_ERR_ARG. */
typedef struct ebvo_gt_params
{
    double orient_gate_deg; /* 4.0: edges within it of 0, 180 or -180 degrees are skipped (:146) */
    double pool_epi_thr;    /* 0.5 px to the epipolar line (:227) */
    double pool_dist;       /* 1.0 px to the GT location (:228) */
    double pool_orient_deg; /* 5.0 degrees between the orientations, no wrap-around (:124) */
    double tp_dist;         /* DIST_TO_GT_THRESH 1.0 (include/definitions.h:42) */
} ebvo_gt_params;
void ebvo_gt_default_params(ebvo_gt_params *p);

/* the stages in the reference's order (:1382-1535) with the names it gives them in Frame_Evaluation_Metrics */
enum
{
    EBVO_GT_EPIPOLAR = 0, /* "Epipolar Proximity" */
    EBVO_GT_DISPARITY,    /* "Location Proximity" */
    EBVO_GT_ORIENTATION,  /* "Orientation" */
    EBVO_GT_SIFT,         /* "SIFT" */
    EBVO_GT_NCC,          /* "NCC" */
    EBVO_GT_BNB_NCC,      /* "BNB-NCC" */
    EBVO_GT_BNB_SIFT,     /* "BNB-SIFT" */
    EBVO_GT_REFINE,       /* "Photometric Refinement" */
    EBVO_GT_CLUSTER,      /* "Edge Clustering" */
    EBVO_GT_NCC2,         /* "NCC" (post-clustering) */
    EBVO_GT_BEST,         /* "Best" */
    EBVO_GT_FINAL,        /* "Final": Best after remove_empty_clusters (:1526) */
    EBVO_GT_NUM_STAGES
};
typedef struct ebvo_gt_stage
{
    int32_t stage, present;   /* present = 0: the chain did not run this stage (or not since arming); the rest is zero */
    int64_t rows, nonempty, rows_with_tp, sum_tp, sum_n; /* exact integer totals over the focused rows */
    /* :365-368, summed in row order like std::accumulate; 0 / 0 is reported as the NaN it is */
    double recall, precision, precision_pair, ambiguity;
} ebvo_gt_stage;

/* Arms `slot` (its pair has run and nothing of it is in flight): uploads the float32 disparity map (h x w as the pair,
 * stride_elems >= w floats per row), finds the GT locations of all left edges, builds the veridical pool, counts the three
 * geometric stages and the NCC stage of a chain without SIFT.  ebvo_stereo_finalize on an armed slot evaluates every
 * later stage as well; the chain's own results do not change.  A new upload or run of the slot disarms it.  Every
 * argument is checked before any state changes (EBVO_ERR_ARG / EBVO_ERR_STATE leave the slot as it was). */
int ebvo_stereo_set_gt(ebvo_ctx *ctx, int slot, const float *disp, int h, int w, ptrdiff_t stride_elems,
                       const ebvo_stereo_calib *calib, const ebvo_gt_params *params);
int ebvo_stereo_gt_size(ebvo_ctx *ctx, int slot, int32_t *n_valid, int32_t *n_focused, int64_t *n_pool);
/* What Stereo_Edge_Pairs holds after :253-267, compacted to the focused rows in left-index order: focused_index
 * [n_focused], gt_xy [n_focused][2], gamma_left / gamma_right [n_focused][3], pool_row_ptr [n_focused + 1], pool_idx
 * [n_pool] (right edge indices, ascending per row).  Any pointer may be NULL. */
int ebvo_stereo_gt_fetch(ebvo_ctx *ctx, int slot, int32_t *focused_index, double *gt_xy, double *gamma_left,
                         double *gamma_right, int32_t *pool_row_ptr, int32_t *pool_idx);
/* stages[EBVO_GT_NUM_STAGES], indexed by stage id; returns the stage count (> 0) or a negative status */
int ebvo_stereo_gt_metrics(ebvo_ctx *ctx, int slot, ebvo_gt_stage *stages);
/* per-row (n, tp) of a stage of the armed slot: rows_n_tp [n_left][2], zero on rows that are not focused.  cap_rows: the
 * rows the caller's array holds; fewer than the slot's left edges: EBVO_ERR_CAPACITY, nothing written. */
int ebvo_stereo_gt_stage_rows(ebvo_ctx *ctx, int slot, int stage, int32_t *rows_n_tp, int32_t cap_rows);
/* The kernels behind it on host arrays.  ebvo_gt_locate: per edge valid [n], gt_xy [n][2] ((-1, -1) when skipped),
 * gamma_left / gamma_right [n][3].  ebvo_gt_evaluate_rows: a CSR list of candidate edges per left edge, focused [nL]
 * bytes, gt_xy [nL][2]; n_tp [nL][2] (may be NULL) and the stage record.  Both run on slot 0's stream (EBVO_ERR_STATE
 * while work of slot 0 is in flight) with a buffer of their own: slot 0's pair, its results and its armed state are not
 * touched. */
int ebvo_gt_locate(ebvo_ctx *ctx, const ebvo_edge *edges, int n, const float *disp, int h, int w, ptrdiff_t stride_elems,
                   const ebvo_stereo_calib *calib, const ebvo_gt_params *params, uint8_t *valid, double *gt_xy,
                   double *gamma_left, double *gamma_right);
int ebvo_gt_evaluate_rows(ebvo_ctx *ctx, const int32_t *row_ptr, const ebvo_edge *cand_edges, int nL, const uint8_t *focused,
                          const double *gt_xy, double tp_dist, int32_t *n_tp, ebvo_gt_stage *stage_out);

/* ---- temporal ground truth from a relative pose (the has_gt() == true branch of the temporal chain) ---------------- */
/* Temporal_Matches::build_Veridical_Quads (src/Temporal_Matches.cpp:57-166) with orientation_mapping (:294-333) and
 * Evaluate_Temporal_Edge_Pairs_on_Quads (:220-292), on what a slot holds after ebvo_temporal_match.  Nothing of the chain
 * is run again and nothing the slot holds is written.
 *   - Per keyframe mate: Gamma_CF = R Gamma_KF + t, its projections into the left and the right camera of the current frame,
 *     the keyframe mate's 3-D tangent carried along and projected (both orientations), and the margin test (:100-105; BOTH
 *     cameras against the LEFT width and height, as written).  (R_stereo * rel_pose.R) * T_1 of :321 is formed as it binds:
 *     the 3x3 product first.
 *   - Veridical quads of a keyframe mate inside the image: the current-frame mates in the whole grid cells of
 *     getCandidatesWithinRadius(projection, search_radius) of BOTH grids (include/Dataset.h:92-113), in the order of
 *     `left_candidates`, with both distances < tp_dist and both orientation differences (mod 180 degrees) < orient_thr_deg,
 *     all strict (:122-137).  The grid is the current-frame grid of the slot's match (its cell_size).
 *   - Rows of the evaluation: keyframe mates with at least one veridical quad whose b_is_TP holds (:233).  The reference
 *     runs the temporal chain over the mates with a veridical quad only; every temporal stage acts row by row, so the
 *     chain on all rows restricted to those rows is the same lists.
 *   - A quad is a true positive when both its centres lie < tp_dist from the projections (strict, :248).  Per row
 *     recall = (tp >= 1), precision = tp / n (0 for an empty row), ambiguity = n; recall is averaged over the rows,
 *     precision and ambiguity over the non-empty rows, ambiguity minus 1 (:280-282); precision_pair = precision.
 *     No rows, or no non-empty row: the four zeros of :274-278, not NaN.
 *   - The four doubles are summed on the host from the per-row integers in KEYFRAME INDEX ORDER.  The reference's order is
 *     that of its `out` vector, which depends on OpenMP scheduling (:71-165); index order is its one-thread order.
 * Two deliberate departures, for datasets that have poses but no disparity map: kf_gamma = NULL uses the triangulated
 * Gamma of the keyframe mates (columns 6-8 of ebvo_finalize_pairs) where the reference uses the GT 3-D point of the
 * disparity map (src/Stereo_Matches.cpp:186, :1638: gamma_left of ebvo_stereo_gt_fetch at the mate's left index), and
 * kf_is_tp = NULL takes every keyframe mate as a true positive (:1645).
 * Accepted ranges: every value >= 0 and not NaN (+inf allowed); anything else EBVO_ERR_ARG, nothing touched. */
typedef struct ebvo_tgt_params
{
    double orient_thr_deg; /* 10.0 (:67) */
    double tp_dist;        /* DIST_TO_GT_THRESH_QUADS 2.0 (include/definitions.h): veridical test and true-positive test */
    double search_radius;  /* 20.0 = 15 + DIST_TO_GT_THRESH_QUADS + 3 (:68) */
    double img_margin;     /* 10 (:69) */
} ebvo_tgt_params;
void ebvo_tgt_default_params(ebvo_tgt_params *p);

/* the stages in the reference's order with the names it gives them (:186-215) */
enum
{
    EBVO_TGT_GRID = 0,    /* "Location Proximity" */
    EBVO_TGT_ORIENTATION, /* "Orientation": the resident candidate lists */
    EBVO_TGT_NCC,         /* "NCC": the candidates with keep */
    EBVO_TGT_SIFT,        /* "SIFT" */
    EBVO_TGT_BNB_NCC,     /* "BNB-NCC" */
    EBVO_TGT_BNB_SIFT,    /* "BNB-SIFT" */
    EBVO_TGT_REFINE,      /* "Photometric Refinement" */
    EBVO_TGT_CLUSTER,     /* "Edge Clustering": the final quads of stages = 1, centres as ebvo_temporal_fetch_final returns them */
    EBVO_TGT_NUM_STAGES
};

/* Arms `slot`, whose temporal match has completed.  R (row-major), t: the relative pose keyframe -> current frame as
 * Utility::get_Relative_Pose returns it (R = R_cf R_kf^T, t = -R t_kf + t_cf).  kf_gamma: n_kf x 3 doubles or NULL,
 * kf_is_tp: n_kf bytes or NULL (see above).  EBVO_ERR_STATE if the slot has no match, anything of it is in flight, or the
 * keyframe was replaced since the match.  A new match, upload or run of the slot disarms it.  Every argument is checked
 * before any state changes: a refused call leaves the slot, armed or not, as it was. */
int ebvo_temporal_set_gt(ebvo_ctx *ctx, int slot, const double R[9], const double t[3], const ebvo_stereo_calib *calib,
                         const ebvo_tgt_params *params, const double *kf_gamma, const uint8_t *kf_is_tp);
/* keyframe mates, those with a veridical quad, veridical quads */
int ebvo_temporal_gt_size(ebvo_ctx *ctx, int slot, int32_t *n_kf, int32_t *n_rows, int64_t *n_veridical);
/* per keyframe mate: in_image [n_kf] (both projections inside the margin), proj_left / proj_right [n_kf][2],
 * orient_left / orient_right [n_kf] (computed for every mate, as the reference does before its margin test), and the
 * veridical quads as a CSR over the keyframe mates: ver_row_ptr [n_kf + 1], ver_idx [n_veridical] (current-frame mate
 * indices).  Any pointer may be NULL. */
int ebvo_temporal_gt_fetch(ebvo_ctx *ctx, int slot, uint8_t *in_image, double *proj_left, double *proj_right,
                           double *orient_left, double *orient_right, int32_t *ver_row_ptr, int32_t *ver_idx);
/* stages[EBVO_TGT_NUM_STAGES], indexed by stage id: ORIENTATION, NCC and (after stages = 1) CLUSTER are filled for every
 * match; a match that kept its stage trail (ebvo_temporal_keep_stages below) fills GRID as well and, after stages = 1, SIFT,
 * BNB_NCC, BNB_SIFT and REFINE: all eight.  Every other stage has present = 0.  Returns the stage count (> 0) or a negative
 * status. */
int ebvo_temporal_gt_metrics(ebvo_ctx *ctx, int slot, ebvo_gt_stage *stages);
/* per-quad b_is_TP of a present stage in that stage's CSR order (ORIENTATION: ebvo_temporal_fetch's candidates; NCC: those
 * with keep; SIFT, BNB_NCC, BNB_SIFT, REFINE: ebvo_temporal_fetch_stage's quads; CLUSTER: ebvo_temporal_fetch_final's quads);
 * 0 on rows outside the evaluation.  What Quad_for_Pose_Solution::b_is_veridical reads.  A stage that is not present, and
 * GRID, which keeps no list of quads: EBVO_ERR_STATE. */
int ebvo_temporal_gt_flags(ebvo_ctx *ctx, int slot, int stage, uint8_t *is_tp);
/* per-row (n, tp) of a present stage of the armed slot: rows_n_tp [n_kf][2], zero on rows outside the evaluation.  cap_rows:
 * the rows the caller's array holds; fewer than the slot's keyframe mates: EBVO_ERR_CAPACITY, nothing written. */
int ebvo_temporal_gt_stage_rows(ebvo_ctx *ctx, int slot, int stage, int32_t *rows_n_tp, int32_t cap_rows);

/* The stage trail.  ebvo_temporal_keep_stages sets a per-slot switch (default 0) that the NEXT ebvo_temporal_match /
 * _submit of the slot reads; the slot's present match and armed state are not touched (EBVO_ERR_STATE while a match of the
 * slot is in flight).  A match submitted with the switch on leaves, besides its own results (which are the same bits either
 * way), what the ground-truth evaluation of the remaining stages needs: with stages = 1 the lists after the SIFT filter,
 * after either best-nearly-best test and after the refinement -- one device-to-device copy of the SIFT-stage list, the
 * others stay where the chain left them -- and the grid stage is counted by ebvo_temporal_set_gt on the match's own grid
 * without forming its list (about ten quads per candidate).  A stage the chain did not reach because an earlier one left
 * nothing is an empty list.  A new match, upload, run or finalisation of the slot drops the trail.
 * ebvo_temporal_stage_size / ebvo_temporal_fetch_stage: stage = EBVO_TGT_SIFT, _BNB_NCC, _BNB_SIFT or _REFINE (any other:
 * EBVO_ERR_ARG, the last error names the call that returns that stage's list) of a match that kept its trail with stages = 1
 * (otherwise EBVO_ERR_STATE); no ground truth is needed.  row_ptr [n_kf + 1] over the keyframe mates in the chain's own
 * order (the best-nearly-best tests sort a row by score), cf_index [n] the current-frame mate of every quad, left / right
 * [n] the centres the evaluation reads: the mate's edges before REFINE, the refined centres at REFINE.  Any pointer may be
 * NULL. */
int ebvo_temporal_keep_stages(ebvo_ctx *ctx, int slot, int on);
int ebvo_temporal_stage_size(ebvo_ctx *ctx, int slot, int stage, int64_t *n);
int ebvo_temporal_fetch_stage(ebvo_ctx *ctx, int slot, int stage, int32_t *row_ptr, int32_t *cf_index, ebvo_edge *left,
                              ebvo_edge *right);
/* The kernels behind it on host arrays, on slot 0's stream (EBVO_ERR_STATE while work of slot 0 is in flight) with buffers
 * of their own: slot 0's results and armed state are not touched.  ebvo_tgt_veridical: keyframe mates (kf_gamma may be
 * NULL) and current-frame mates in, the arrays of ebvo_temporal_gt_fetch out (any may be NULL); the grid of the
 * current-frame mates (img_w x img_h, cell_size >= 1) is built in the call's buffer.  ver_idx holds cap entries; more
 * veridical quads than that: EBVO_ERR_CAPACITY with *n_veridical set.  ebvo_tgt_evaluate_rows: a CSR list of quad centres
 * per keyframe mate, row_on [n_kf] (NULL: all), the projections; n_tp [n_kf][2], is_tp per quad (both may be NULL). */
int ebvo_tgt_veridical(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, const double *kf_gamma, int n_kf,
                       const ebvo_edge *cf_left, const ebvo_edge *cf_right, int n_cf, int img_w, int img_h, int cell_size,
                       const double R[9], const double t[3], const ebvo_stereo_calib *calib, const ebvo_tgt_params *params,
                       uint8_t *in_image, double *proj_left, double *proj_right, double *orient_left, double *orient_right,
                       int32_t *ver_row_ptr, int32_t *ver_idx, int64_t cap, int64_t *n_veridical);
int ebvo_tgt_evaluate_rows(ebvo_ctx *ctx, const int32_t *row_ptr, const ebvo_edge *left_centres, const ebvo_edge *right_centres,
                           int n_kf, const uint8_t *row_on, const double *proj_left, const double *proj_right, double tp_dist,
                           int32_t *n_tp, uint8_t *is_tp, ebvo_gt_stage *stage_out);
/* The grid stage ("Location Proximity") on host arrays, under the same rules: per keyframe mate whose row is on (row_on
 * NULL: all) the current-frame mates that apply_spatial_grid_filtering_quads (src/Temporal_Matches.cpp:335-383) pairs with
 * it -- in the grid cells within ceil(grid_radius / cell_size) cells of the mate's own left AND right cell -- are counted,
 * and those with both edges < tp_dist from the row's projections are the true positives; no list is formed.  n_tp
 * [n_kf][2] (may be NULL) and the stage record.  cell_size >= 1; grid_radius finite and >= 0; tp_dist >= 0 and not NaN. */
int ebvo_tgt_grid_rows(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf, const ebvo_edge *cf_left,
                       const ebvo_edge *cf_right, int n_cf, int img_w, int img_h, int cell_size, double grid_radius,
                       const uint8_t *row_on, const double *proj_left, const double *proj_right, double tp_dist, int32_t *n_tp,
                       ebvo_gt_stage *stage_out);

/* ---- temporal matching under a pose prior (this project's own; the reference searches around the keyframe position) ---
 * A relative pose (R, t) keyframe -> current frame in the convention of the ground truth above and of the pose search
 * (Gc = R * Gamma + t in the left camera) moves the search of every keyframe mate to where the pose predicts it: the mate
 * is triangulated, projected into both cameras and its orientation mapped (the arithmetic of the ground truth's
 * projection, bit for bit), and the grid walk and the orientation test of the candidate stage take the projections (and,
 * with use_orientation, the mapped orientations) as their query in place of the mate's own edges.  A mate is LIVE iff its
 * four projected coordinates lie strictly inside (img_margin, w - img_margin) x (img_margin, h - img_margin) of the
 * CURRENT frame (both cameras against that one size; NaN and infinite coordinates are outside) and its depth is positive in
 * both cameras; a mate that is not live has an empty row.  Rows keep the order of an unprimed match (dy outer, dx inner,
 * ascending mate index within a cell), and every later stage is the unprimed chain on the candidate list.
 *
 * The setter is a per-slot, ONE-SHOT switch and does no device work: the next successful match / _submit call of the slot
 * consumes the pose, a refused one leaves it pending; setting a keyframe drops the pending priors of every slot, the clear
 * call drops the slot's (no error when there is none).  EBVO_ERR_STATE while a match of the slot is in flight;
 * EBVO_ERR_ARG, with nothing changed, for a NaN or infinite entry of R or t, a calibration the ground truth would refuse,
 * or an img_margin that is negative or not finite.  params NULL: the defaults.
 * The fetch returns the arrays of the slot's match -- live [n_kf], proj_* [n_kf][2], orient_* [n_kf]; any pointer may be
 * NULL -- which stay until the match is replaced; EBVO_ERR_STATE when the match was made without a prior.  On a match that
 * kept its stage trail, the ground truth's EBVO_TGT_GRID row counts the cells the match searched: the prior's query
 * points, nothing for a mate that is not live.
 * The candidates call is the stage on host arrays, under the rules of the host-array calls above (slot 0's stream, buffers
 * of its own, EBVO_ERR_STATE while slot 0 has work in flight): the arrays of the fetch plus row_ptr [n_kf + 1] and col_idx
 * (cap entries; more candidates: EBVO_ERR_CAPACITY with *n_candidates set).  Any output pointer may be NULL. */
typedef struct ebvo_tprior_params
{
    double img_margin;       /* 0 */
    int32_t use_orientation; /* 1 */
} ebvo_tprior_params;
void ebvo_tprior_default_params(ebvo_tprior_params *p);
int ebvo_temporal_set_prior(ebvo_ctx *ctx, int slot, const double R[9], const double t[3], const ebvo_stereo_calib *calib,
                            const ebvo_tprior_params *params);
int ebvo_temporal_clear_prior(ebvo_ctx *ctx, int slot);
int ebvo_temporal_prior_fetch(ebvo_ctx *ctx, int slot, uint8_t *live, double *proj_left, double *proj_right, double *orient_left,
                              double *orient_right);
int ebvo_tprior_candidates(ebvo_ctx *ctx, const ebvo_edge *kf_left, const ebvo_edge *kf_right, int n_kf, const ebvo_edge *cf_left,
                           const ebvo_edge *cf_right, int n_cf, int img_w, int img_h, int cell_size, double grid_radius,
                           double orient_thr_deg, const double R[9], const double t[3], const ebvo_stereo_calib *calib,
                           const ebvo_tprior_params *params, uint8_t *live, double *proj_left, double *proj_right,
                           double *orient_left, double *orient_right, int32_t *row_ptr, int32_t *col_idx, int64_t cap,
                           int64_t *n_candidates);

/* ---------------------------------------------------------------------------------------- */
/* Device-resident stereo pipeline: TOED(left) + TOED(right) + candidates + NCC of one pair,  */
/* images and every intermediate in HBM.  This is what bench.py times.                        */
/* ---------------------------------------------------------------------------------------- */

/* Accepted ranges.  epi_thr, max_disp, orient_thr_deg: >= 0, +inf allowed (the predicate then bounds nothing); ncc_thr: any
 * value but NaN (keep = best > ncc_thr).  stage_mask: 1 ... 7.  ebvo_stereo_submit / ebvo_stereo_run and every
 * ebvo_epi_candidates* call refuse a NaN threshold or a negative epi_thr / max_disp / orient_thr_deg with EBVO_ERR_ARG
 * before touching any state: the slot keeps its pair and its results (a negative max_disp would otherwise need its own
 * rule: the reference's sqrt(0) <= max_disp rejects even coincident points). */
typedef struct ebvo_stereo_params
{
    double F21[9]; /* row-major fundamental matrix, Dataset::get_fund_mat_21 */
    double epi_thr, max_disp, orient_thr_deg, ncc_thr;
    int stage_mask;
    int reserved; /* flags: 0, or EBVO_PAIR_NO_SIMS | EBVO_PAIR_PUSH / EBVO_PAIR_PACK | EBVO_PAIR_PUSH_THETA */
} ebvo_stereo_params;
/* ebvo_stereo_params.reserved = EBVO_PAIR_NO_SIMS: the resident pipeline stores, per candidate pair, the final score (the
 * maximum of the four similarities: what the reference keeps, refine_final_scores, src/Stereo_Matches.cpp:596-600) and the
 * keep flag, not the four similarities themselves (32 of the 41 bytes the NCC stage writes per pair).  The arithmetic is the
 * same; asking for `sims` of such a pair is EBVO_ERR_STATE. */
#define EBVO_PAIR_NO_SIMS 1
/* EBVO_PAIR_PUSH: the pair's chain ENDS with a kernel that writes the compact results (the arrays of
 * ebvo_stereo_fetch_compact_begin's default selection; + EBVO_PAIR_PUSH_THETA: the orientations too) straight into a page-locked
 * arena of the slot, over PCIe: when ebvo_stereo_wait returns they are in host memory -- no copy call, no second stream, no event.
 * ebvo_stereo_pushed_view hands out the pointers; they stay valid until the slot's next submission.  What a frame loop that
 * consumes the first NCC pass on the host wants (src/Stereo_Matches.cpp:1427 onwards run there). */
#define EBVO_PAIR_PUSH 2
#define EBVO_PAIR_PUSH_THETA 4
/* EBVO_PAIR_PACK: the chain ends with the same kernel, writing the block into DEVICE staging; ebvo_stereo_fetch_compact_begin is
 * then ONE device-to-host copy of exactly the bytes the pair produced (the copy engine moves a contiguous block ~1.3x faster than
 * a kernel's stores cross PCIe on the boxes measured).  Exclusive with EBVO_PAIR_PUSH; EBVO_PAIR_PUSH_THETA adds the orientations. */
#define EBVO_PAIR_PACK 8

typedef struct ebvo_stereo_counts
{
    int32_t n_left, n_right;             /* toed_edges.size() of each image */
    int32_t n_total_left, n_total_right; /* Total_Num_Of_TOED of each image */
    int64_t n_pairs;                     /* candidates after the geometric filters */
    int64_t n_matches;                   /* pairs with max NCC > ncc_thr */
} ebvo_stereo_counts;

void ebvo_stereo_default_params(ebvo_stereo_params *p);
/* copy one stereo pair into HBM (not part of the timed region) */
int ebvo_stereo_upload(ebvo_ctx *ctx, const uint8_t *img_left, const uint8_t *img_right, int h, int w,
                       ptrdiff_t stride_left, ptrdiff_t stride_right);
/* run the whole hot path on the resident pair (= submit + wait on slot 0) */
int ebvo_stereo_run(ebvo_ctx *ctx, const ebvo_stereo_params *p, ebvo_stereo_counts *counts);
/* fetch the results of the last ebvo_stereo_run; any pointer may be NULL */
int ebvo_stereo_fetch(ebvo_ctx *ctx, ebvo_edge *left, ebvo_edge *right, int32_t *row_ptr, int32_t *col_idx,
                      double *sims, double *best, uint8_t *keep, float *left_patches);

/* Several pairs in flight from one host thread: a slot is a stereo pair's workspace plus its own HIP stream.
 * ebvo_stereo_submit enqueues the whole hot path of the slot's resident pair WITHOUT any host synchronisation
 * (every size stays in device memory; launches are sized by capacities) and returns at once; ebvo_stereo_wait
 * blocks until that pair is done and returns its counts.  Kernels of different slots overlap on the GPU.
 * Slot 0 always exists and is the one the host-buffer entry points above use. */
int ebvo_stereo_set_slots(ebvo_ctx *ctx, int n_slots);
int ebvo_stereo_upload_slot(ebvo_ctx *ctx, int slot, const uint8_t *img_left, const uint8_t *img_right, int h, int w,
                            ptrdiff_t stride_left, ptrdiff_t stride_right);
/* The same upload without blocking the caller (round 4), for a frame loop that reads frame k + 1 while frame k is matched
 * (src/Pipeline.cpp:77-99, cmd/main_VO.cpp:99-113).
 * PULL FORM (both images inside a range registered with ebvo_host_register -- the caller's frame ring, registered once;
 * memory that is page-locked already, hipHostMalloc, may be registered too): the call only records where the images lie (no
 * runtime call, < 1 us) and the pair's own chain starts with a kernel that READS them from the caller's memory -- no copy
 * engine, no second stream, no event.  The images must stay unchanged until the pair's ebvo_stereo_wait has returned, and
 * registered as long as the slot is submitted with them.  Images anywhere else (pageable memory) are copied into the slot's
 * own page-locked staging BEFORE the call returns -- the caller may free or overwrite them at once -- and go up from there on
 * the context's upload stream (ebvo_ingest_stats tells which form the calls took).
 * Both uploads check every argument (slot, pointers, size, both strides) and the slot's state before they touch it: a refused
 * call leaves the slot's resident pair and its results as they were. */
int ebvo_stereo_upload_async(ebvo_ctx *ctx, int slot, const uint8_t *img_left, const uint8_t *img_right, int h, int w,
                             ptrdiff_t stride_left, ptrdiff_t stride_right);
/* page-lock / release caller memory (hipHostRegister / hipHostUnregister): no HIP header needed on the host side */
int ebvo_host_register(ebvo_ctx *ctx, void *p, size_t bytes);
int ebvo_host_unregister(ebvo_ctx *ctx, void *p);
/* diagnostics: ebvo_stereo_upload_async calls so far that took {the pull form, the upload stream} */
int ebvo_ingest_stats(const ebvo_ctx *ctx, int64_t out[2]);
int ebvo_stereo_submit(ebvo_ctx *ctx, int slot, const ebvo_stereo_params *p);
int ebvo_stereo_wait(ebvo_ctx *ctx, int slot, ebvo_stereo_counts *counts);
int ebvo_stereo_fetch_slot(ebvo_ctx *ctx, int slot, ebvo_edge *left, ebvo_edge *right, int32_t *row_ptr,
                           int32_t *col_idx, double *sims, double *best, uint8_t *keep, float *left_patches);

/* Results of a finished pair WITHOUT a staging copy on the host: ebvo_stereo_fetch_begin enqueues the device-to-host copies
 * of the selected arrays into page-locked memory owned by the slot and returns at once (the copy engine works while
 * other slots compute); ebvo_stereo_fetch_end waits for them and hands out read-only pointers, valid until the next
 * upload / submit / host-buffer call on that slot.  What the stage-wise reference code consumes per pair is the default
 * selection (both edge lists, the CSR candidate lists, best score and keep flag per pair: ~16 MB at 126 k edges per
 * image); the four individual scores are another 32 bytes per pair. */
enum
{
    EBVO_FETCH_EDGES = 1, /* left, right */
    EBVO_FETCH_CSR = 2,   /* row_ptr, col_idx */
    EBVO_FETCH_BEST = 4,
    EBVO_FETCH_KEEP = 8,
    EBVO_FETCH_SIMS = 16,
    EBVO_FETCH_DEFAULT = 15,
    EBVO_FETCH_ALL = 31
};
typedef struct ebvo_stereo_view
{
    const ebvo_edge *left, *right; /* n_left, n_right */
    const int32_t *row_ptr;        /* n_left + 1 */
    const int32_t *col_idx;        /* n_pairs */
    const double *sims;            /* n_pairs x 4 (pp, nn, pn, np) */
    const double *best;            /* n_pairs */
    const uint8_t *keep;           /* n_pairs */
    int32_t n_left, n_right;
    int64_t n_pairs;
} ebvo_stereo_view; /* pointers of arrays that were not selected are NULL */
int ebvo_stereo_fetch_begin(ebvo_ctx *ctx, int slot, int what);
int ebvo_stereo_fetch_end(ebvo_ctx *ctx, int slot, ebvo_stereo_view *view);

/* The same results in fewer bytes (round 4): (x, y) of every edge as 16 bytes (an edge's index is its position in the list),
 * the orientations as separate arrays on demand, the keep flag of pair k as bit k & 31 of word k >> 5; best stays fp64.
 * 11.6 MB instead of 16.2 MB per KITTI pair for the default selection.  Same protocol as ebvo_stereo_fetch_begin / _end (the two
 * share the slot's page-locked arena: one selection at a time). */
enum
{
    EBVO_COMPACT_XY = 1,
    EBVO_COMPACT_THETA = 2,
    EBVO_COMPACT_CSR = 4,
    EBVO_COMPACT_BEST = 8,
    EBVO_COMPACT_KEEP_BITS = 16,
    EBVO_COMPACT_DEFAULT = 1 | 4 | 8 | 16,
    EBVO_COMPACT_ALL = 31
};
typedef struct ebvo_stereo_compact_view
{
    const double *left_xy, *right_xy;       /* n_left x 2, n_right x 2 */
    const double *left_theta, *right_theta; /* n_left, n_right */
    const int32_t *row_ptr;                 /* n_left + 1 */
    const int32_t *col_idx;                 /* n_pairs */
    const double *best;                     /* n_pairs */
    const uint32_t *keep_bits;              /* 2 * ceil(n_pairs / 64) words */
    int32_t n_left, n_right;
    int64_t n_pairs, n_matches;
} ebvo_stereo_compact_view; /* pointers of arrays that were not selected are NULL */
int ebvo_stereo_pushed_view(ebvo_ctx *ctx, int slot, ebvo_stereo_compact_view *view); /* after a pair submitted with EBVO_PAIR_PUSH */
int ebvo_stereo_fetch_compact_begin(ebvo_ctx *ctx, int slot, int what);
int ebvo_stereo_fetch_compact_end(ebvo_ctx *ctx, int slot, ebvo_stereo_compact_view *view);

/* Per-kernel device timing (HIP events on the slots' streams, accumulated). */
#define EBVO_MAX_KERNELS 32 /* >= the number of kernel ids (ebvo_internal.h) */
typedef struct ebvo_kernel_time
{
    const char *name;
    double ms;        /* accumulated */
    int64_t launches; /* accumulated */
} ebvo_kernel_time;
/* on = 0: off; 1: bracket every kernel launch with HIP events; N > 1: in the device pipeline bracket the kernels of every
 * N-th submitted pair only (the event records themselves cost ~0.2 ms of device timeline per pair). */
int ebvo_profile_enable(ebvo_ctx *ctx, int on);
int ebvo_profile_reset(ebvo_ctx *ctx);
int ebvo_profile_get(ebvo_ctx *ctx, ebvo_kernel_time *out /* EBVO_MAX_KERNELS */, int *n);

/* Test hooks, not part of the drop-in surface.  key 0: attempts of the regrow loop of ebvo_stereo_wait (0 = default 4);
 * key 1: treat the next `value` pair results as "candidate buffers overflowed" (exercises the regrow / give-up path);
 * key 2: lanes -- from four slots on, ebvo_stereo_submit deals the kernels of the pairs round-robin to
 *        min(lanes, slots - 1) streams of the context instead of one stream per slot (default 4, the measured optimum
 *        on MI355X; 0 = one stream per slot whatever their number).
 * key 3: the profiler instruments ONE stage (value = its index in ebvo_profile_get's order + 1; 0 = every stage): no
 *        event markers between the other kernels, so the stage is timed as it runs in the unprofiled pipeline.
 * key 4: 1 = the photometric refinements never use their eight-lanes-per-pair launch layout (0 = default: chosen per
 *        iteration from the number of active pairs); key 5: that threshold (0 = built-in).  Same bits either way.
 * key 7: 1 = the stereo refinement's eight-lanes layout as a launch per iteration instead of one persistent launch;
 * key 8: waves per SIMD the persistent launch is built for (2 or 3); key 9: most workgroups of that launch (0 = the default,
 *        1024; at most 1 << 20).  Same bits either way.
 * key 6: set the candidate-quad capacity of every slot's temporal stage to `value` (>= 1): the next ebvo_temporal_match
 *        finds more quads than its buffers hold and takes the regrow path.
 * key 10: 0 = ebvo_stereo_submit enqueues the pair as direct launches, 1 = as a captured hipGraph (default).
 * keys 11, 12: grid of toed_exact_centre / toed_exact_mags in blocks (0 = what the device keeps resident; at most 65536);
 * key 13: 1 = ebvo_stereo_upload_async copies on the upload stream instead of the pull kernel; key 14: 1 = lines, boxes,
 *        sin / cos and row pairs as four launches instead of one; key 17: grid of ncc_tile_kernel in blocks (0 = resident);
 *        key 18: grids of decide / cand_scatter / candidates<fill> (512 / 512 / 4096 blocks) divided by `value` (0 = the
 *        default, 4; at most 512); key 19: most blocks of candidates<count> (0 = the default, 1024; at most 4096).  Same bits
 *        either way (A/B switches).
 * key 15: bit mask -- an idempotent kernel of the resident pair's chain is launched TWICE (1 centre, 2 mags, 4 right bank,
 *        8 NCC tile): what one more launch costs the pair rate (tools/gpu_marginal_cost.py).
 * key 16: the resident pair's chain ENDS after stage `value` (0 = whole chain; the pair's record keeps the counts of the last
 *        whole run, the buffers behind the stage are stale): the pair rate of every prefix of the chain
 *        (tools/gpu_prefix_chain.py).  Measurement only.
 * key 20: index pairs per batch of the pose search (ebvo_temporal_estimate_pose / ebvo_pose_from_quads; 0 = the default,
 *        4096; at most 1 << 20).  Same bits for any value.
 * key 22: most blocks of every grid-stride launch of ebvo_temporal_match(_submit / _wait) -- grid, candidates, NCC, SIFT,
 *        glue, refinement, clustering (0 = each launch's own cap; at most 65536).  Same bits for any value; the stereo
 *        pair's launches are not touched.
 * key 23: most blocks of every grid-stride launch ebvo_stereo_finalize(_submit) enqueues -- SIFT filter, row glue, both
 *        Best-Nearly-Best tests, shift, the refinement (its persistent launch included), clustering, patches, the final
 *        lists and output rows, the ground-truth rows of an armed slot (0 = each launch's own cap; at most 65536).  The
 *        tiled scans and the second NCC pass launch one block per tile / one thread per item and keep their grids.  Same
 *        bits for any value; the pair chain, the temporal chain and the host-buffer calls are not touched, and keys 22
 *        and 23 do not see each other.
 * A negative value, an unknown key or a value outside the key's range returns EBVO_ERR_ARG and changes nothing. */
int ebvo_debug_set(ebvo_ctx *ctx, int key, int value);

/* Raw FP64 vector-ALU microbenchmark (mul + add, no FMA) used to anchor the compute roofline:
 * returns achieved TFLOP/s over `iters` launches. */
int ebvo_fp64_peak(ebvo_ctx *ctx, int iters, double *tflops_muladd, double *tflops_fma);

#ifdef __cplusplus
}
#endif
#endif /* EBVO_HIP_H */
