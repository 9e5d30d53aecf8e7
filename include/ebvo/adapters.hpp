// adapters.hpp -- C++17 host-side mirror of the reference's interface for the hot path, over the
// C ABI of ebvo_hip.h.  Header-only; depends on the STL and ebvo_hip.h only, so it compiles with or
// without OpenCV / Eigen.  integration/*.cpp shows the reference-side translation units built on it.
//
//   ebvo::ThirdOrderEdgeDetectionHIP<EdgeT>  -- same public surface as ThirdOrderEdgeDetectionCPU
//                                               (include/toed/cpu_toed.hpp:70-115 of the reference)
//   ebvo::StereoMatcherHIP<EdgeT>            -- the bodies of apply_Epipolar_Line_Distance_Filtering,
//                                               apply_Disparity_Filtering, apply_orientation_filter and
//                                               apply_NCC_Filtering (include/Stereo_Matches.h:61-68) on
//                                               plain vectors; the reference-side glue copies to/from
//                                               Stereo_Edge_Pairs (include/Dataset.h:180-289)
//   ebvo::undistort / sift_descriptors / sift_min_distances -- cv::undistort (src/Pipeline.cpp:78-79) and the cv::SIFT
//                                               calls of augment_Edge_Data / apply_SIFT_filtering (src/Stereo_Matches.cpp:655-787)
//   ebvo::patch_similarity / ncc_quads       -- Utility::get_patch_similarity (src/utility.cpp:163-180),
//                                               Temporal_Matches::apply_NCC_filtering_quads scoring and the
//                                               MatlabNCCComputer::computeNCC-shaped entry
//
// EdgeT is the reference's `struct Edge` (or anything with .location.x, .location.y, .orientation,
// .index): TOED fills exactly those fields and leaves the rest as the default constructor set them
// (b_isEmpty = true, frame_source = -1), like src/toed/cpu_toed.cpp:557-563.
//
// Errors: the reference prints and continues; these adapters print the library's message to stderr and
// leave outputs empty, and additionally expose last_status for callers that want to check.
#ifndef EBVO_ADAPTERS_HPP
#define EBVO_ADAPTERS_HPP

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <cstring>
#include <iomanip>
#include <limits>
#include <memory>
#include <ostream>
#include <string>
#include <utility>
#include <vector>

#include "../ebvo_hip.h"

namespace ebvo
{

// One shared device context per (device, size): the reference creates one TOED object per Pipeline and
// the matchers have no state of their own, so they borrow the TOED object's context.
class Context
{
  public:
    Context(int max_h, int max_w, int device = 0) : h_(max_h), w_(max_w)
    {
        status_ = ebvo_ctx_create(device, max_h, max_w, &ctx_);
        if (status_ != EBVO_OK)
            std::fprintf(stderr, "\033[1;31m[ERROR] ebvo_ctx_create: %s\033[0m\n", ebvo_strerror(status_));
    }
    ~Context() { ebvo_ctx_destroy(ctx_); }
    Context(const Context &) = delete;
    Context &operator=(const Context &) = delete;
    ebvo_ctx *get() const { return ctx_; }
    int status() const { return status_; }
    int max_h() const { return h_; }
    int max_w() const { return w_; }
    typedef std::shared_ptr<Context> Ptr;

    // Resident stage-wise path: what the last two get_Third_Order_Edges calls produced is still on the device (one result
    // per image workspace of the library, used alternately: main_VO detects left, then right, src/Pipeline.cpp:93-97) and
    // in page-locked memory (`edges`).  A later stage that is handed a vector with exactly these edges names the device copy
    // by its tag instead of uploading the vector.
    struct ResidentEdges
    {
        uint64_t tag = 0; // 0: nothing
        const ebvo_edge *edges = nullptr;
        int n = 0;
    };
    ResidentEdges resident[2];
    int next_workspace = 0;

  private:
    ebvo_ctx *ctx_ = nullptr;
    int status_ = EBVO_OK, h_, w_;
};

inline bool report(const Context &c, int rc, const char *where)
{
    if (rc == EBVO_OK)
        return true;
    std::fprintf(stderr, "\033[1;31m[ERROR] %s: %s (%s)\033[0m\n", where, ebvo_strerror(rc),
                 c.get() ? ebvo_last_error(c.get()) : "");
    return false;
}

template <class EdgeT>
inline ebvo_edge to_abi(const EdgeT &e)
{
    ebvo_edge o;
    o.x = e.location.x;
    o.y = e.location.y;
    o.theta = e.orientation;
    o.index = e.index;
    o.pad = 0;
    return o;
}

// read-only view of an array the library or a result object owns
template <class T>
struct Span
{
    const T *p = nullptr;
    size_t n = 0;
    Span() = default;
    Span(const T *p_, size_t n_) : p(p_), n(n_) {}
    Span(const std::vector<T> &v) : p(v.data()), n(v.size()) {}
    const T *data() const { return p; }
    size_t size() const { return n; }
    bool empty() const { return n == 0; }
    const T &operator[](size_t k) const { return p[k]; }
    const T *begin() const { return p; }
    const T *end() const { return p + n; }
};

inline bool same_bits(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// the workspace whose resident edge list is EXACTLY `edges` (every x, y, orientation bit for bit, every index), or -1
template <class EdgeT>
inline int resident_workspace(const Context &c, const std::vector<EdgeT> &edges)
{
    for (int ws = 0; ws < 2; ++ws)
    {
        const Context::ResidentEdges &r = c.resident[ws];
        if (!r.tag || (size_t)r.n != edges.size())
            continue;
        size_t k = 0;
        for (; k < edges.size(); ++k)
        {
            const ebvo_edge &a = r.edges[k];
            const EdgeT &e = edges[k];
            if (!(same_bits(a.x, e.location.x) && same_bits(a.y, e.location.y) && same_bits(a.theta, e.orientation) &&
                  a.index == (int32_t)e.index))
                break;
        }
        if (k == edges.size())
            return ws;
    }
    return -1;
}

// ---------------------------------------------------------------------------------------------
template <class EdgeT>
class ThirdOrderEdgeDetectionHIP
{
  public:
    // public data members of ThirdOrderEdgeDetectionCPU (include/toed/cpu_toed.hpp:90-114)
    double *subpix_edge_pts_final = nullptr; // N x 4: x, y, orientation, sub-pixel gradient magnitude
    int edge_pt_list_idx = 0;
    int num_of_edge_data = 4;
    int omp_threads = 1;
    double time_conv = 0, time_nms = 0;
    std::vector<EdgeT> toed_edges;
    int Total_Num_Of_TOED = 0;
    int last_status = EBVO_OK;
    typedef std::shared_ptr<ThirdOrderEdgeDetectionHIP> Ptr;

    ThirdOrderEdgeDetectionHIP(int H, int W, int device = 0)
        : img_height(H), img_width(W), ctx_(std::make_shared<Context>(H, W, device))
    {
        all4_.resize(4); // subpix_edge_pts_final of an image without a single maximum
        subpix_edge_pts_final = all4_.data();
        last_status = ctx_->status();
    }

    // get_Third_Order_Edges(cv::Mat): any Mat-like with .data (uchar*), .rows, .cols, .step
    template <class MatT>
    void get_Third_Order_Edges(const MatT &img)
    {
        get_Third_Order_Edges(reinterpret_cast<const uint8_t *>(img.data), img.rows, img.cols, (ptrdiff_t)img.step);
    }

    void get_Third_Order_Edges(const uint8_t *data, int rows, int cols, ptrdiff_t step)
    {
        toed_edges.clear(); // preprocessing(), src/toed/cpu_toed.cpp:86
        Total_Num_Of_TOED = 0;
        edge_pt_list_idx = 0;
        if (rows != img_height || cols != img_width)
        { // the reference object is sized once from the left image (include/Pipeline.h:89-101)
            std::fprintf(stderr, "\033[1;31m[ERROR] TOED: image %dx%d does not match %dx%d\033[0m\n", cols, rows,
                         img_width, img_height);
            last_status = EBVO_ERR_ARG;
            return;
        }
        // the result stays on the device (workspace `ws`) and arrives in page-locked memory: toed_edges is built straight
        // from it, subpix_edge_pts_final points at it (valid until the next call but one, like the reference's member buffer
        // is valid until the next call)
        const int ws = ctx_->next_workspace;
        ctx_->next_workspace ^= 1;
        ctx_->resident[ws] = Context::ResidentEdges();
        ebvo_toed_view v;
        last_status = ebvo_toed_resident(ctx_->get(), ws, data, rows, cols, step, 1, &v);
        if (!report(*ctx_, last_status, "ebvo_toed_resident"))
            return;
        time_conv = v.t_conv;
        time_nms = v.t_nms;
        const int n_kept = v.n_kept, n_total = v.n_total;
        toed_edges.reserve((size_t)n_kept);
        EdgeT e{}; // default-constructed: b_isEmpty = true, frame_source = -1
        for (int k = 0; k < n_kept; ++k)
        {
            e.location.x = v.edges[k].x;
            e.location.y = v.edges[k].y;
            e.orientation = v.edges[k].theta;
            e.index = v.edges[k].index;
            toed_edges.push_back(e);
        }
        subpix_edge_pts_final = n_total ? const_cast<double *>(v.all4) : all4_.data();
        ctx_->resident[ws].tag = v.tag;
        ctx_->resident[ws].edges = v.edges;
        ctx_->resident[ws].n = n_kept;
        Total_Num_Of_TOED = n_total;
        edge_pt_list_idx = n_total;
    }

    const Context::Ptr &context() const { return ctx_; }

  private:
    int img_height, img_width;
    Context::Ptr ctx_;
    std::vector<double> all4_;
};

// ---------------------------------------------------------------------------------------------
// Candidate lists as the reference keeps them per focused edge: indices into the candidate edge
// vector, ascending (EdgeCluster::contributing_edges_toed_indices[0], src/Stereo_Matches.cpp:413).
struct CandidateLists
{
    std::vector<int32_t> row_ptr; // nL + 1
    std::vector<int32_t> col_idx; // right TOED index per pair
    size_t rows() const { return row_ptr.empty() ? 0 : row_ptr.size() - 1; }
};

struct NccScores
{
    std::vector<double> pp_nn_pn_np; // 4 per pair (src/Stereo_Matches.cpp:592-595)
    std::vector<double> best;        // final_SIM_score (:596)
    std::vector<uint8_t> keep;       // best > NCC_THRESH (:597)
    std::vector<float> left_patches; // nL x 2 x 49 (left_edge_patches, :578)
};

template <class EdgeT>
class StereoMatcherHIP
{
  public:
    explicit StereoMatcherHIP(Context::Ptr ctx) : ctx_(std::move(ctx)) {}
    int last_status = EBVO_OK;

    // Stereo_Matches::CalculateEpipolarLine with a row-major 3x3 F (src/Stereo_Matches.cpp:10-20).
    static std::vector<std::array<double, 3>> CalculateEpipolarLine(const double F[9], const std::vector<EdgeT> &edges)
    {
        std::vector<std::array<double, 3>> lines(edges.size());
        static thread_local std::vector<ebvo_edge> abi; // reused: a fresh 4 MB vector per frame costs more than the lines
        abi.resize(edges.size());
        for (size_t k = 0; k < edges.size(); ++k)
            abi[k] = to_abi(edges[k]);
        ebvo_epipolar_lines(F, abi.data(), (int)abi.size(), lines.empty() ? nullptr : lines[0].data());
        return lines;
    }

    // stage_mask = EBVO_STAGE_EPIPOLAR            -> apply_Epipolar_Line_Distance_Filtering (:381-419)
    //              ... | EBVO_STAGE_DISPARITY     -> + apply_Disparity_Filtering (:534-553)
    //              ... | EBVO_STAGE_ORIENTATION   -> + apply_orientation_filter (:863-915)
    // The three filters are independent predicates on (left, right) and each keeps the list order, so
    // applying them fused equals applying them one after the other.
    CandidateLists candidates(const std::vector<EdgeT> &left, const std::vector<EdgeT> &right,
                              const std::vector<std::array<double, 3>> &lines, int stage_mask = EBVO_STAGE_ALL,
                              double epi_thr = EBVO_EPIPOLAR_LINE_DIST_THRESH, double max_disp = EBVO_MAX_DISPARITY,
                              double orient_thr_deg = EBVO_ORIENT_THRESH_DEG)
    {
        CandidateLists out;
        std::vector<ebvo_edge> L(left.size()), R(right.size());
        for (size_t k = 0; k < left.size(); ++k)
            L[k] = to_abi(left[k]);
        for (size_t k = 0; k < right.size(); ++k)
            R[k] = to_abi(right[k]);
        out.row_ptr.assign(left.size() + 1, 0);
        int64_t n = 0;
        const double *ln = lines.empty() ? nullptr : lines[0].data();
        // one search when the list fits a first guess of 24 candidates per edge (the reported size is exact otherwise)
        int64_t cap = stage_mask == EBVO_STAGE_EPIPOLAR ? 0 : (int64_t)(24 * left.size() + 1024);
        for (int attempt = 0; attempt < 2; ++attempt)
        {
            out.col_idx.resize((size_t)cap);
            last_status = ebvo_epi_candidates(ctx_->get(), L.data(), (int)L.size(), R.data(), (int)R.size(), ln, epi_thr, max_disp,
                                              orient_thr_deg, stage_mask, out.row_ptr.data(), cap ? out.col_idx.data() : nullptr,
                                              cap, &n);
            if (last_status != EBVO_ERR_CAPACITY && !(cap == 0 && last_status == EBVO_OK && n > 0))
                break;
            cap = n;
        }
        out.col_idx.resize(last_status == EBVO_OK ? (size_t)n : 0);
        report(*ctx_, last_status, "ebvo_epi_candidates");
        return out;
    }

    // The three geometric stages of get_Stereo_Edge_Pairs (:1374, :1387, :1399) from ONE device search: the list under the
    // epipolar and disparity predicates + orient_ok[k] = pair k also passes apply_orientation_filter.  A stage-wise caller
    // fills matching_edge_clusters from the list at the first stage (the epipolar-only list, hundreds of candidates per
    // edge, is never formed), has nothing to do at the second and keeps the flagged pairs at the third.
    struct StagedCandidates
    {
        CandidateLists lists;
        std::vector<uint8_t> orient_ok;
    };
    StagedCandidates candidates_staged(const std::vector<EdgeT> &left, const std::vector<EdgeT> &right,
                                       const std::vector<std::array<double, 3>> &lines,
                                       double epi_thr = EBVO_EPIPOLAR_LINE_DIST_THRESH, double max_disp = EBVO_MAX_DISPARITY,
                                       double orient_thr_deg = EBVO_ORIENT_THRESH_DEG)
    {
        StagedCandidates out;
        std::vector<ebvo_edge> L(left.size()), R(right.size());
        for (size_t k = 0; k < left.size(); ++k)
            L[k] = to_abi(left[k]);
        for (size_t k = 0; k < right.size(); ++k)
            R[k] = to_abi(right[k]);
        out.lists.row_ptr.assign(left.size() + 1, 0);
        int64_t n = 0, cap = (int64_t)(24 * left.size() + 1024);
        const double *ln = lines.empty() ? nullptr : lines[0].data();
        for (int attempt = 0; attempt < 2; ++attempt)
        {
            out.lists.col_idx.resize((size_t)cap);
            out.orient_ok.resize((size_t)cap);
            last_status = ebvo_epi_candidates_staged(ctx_->get(), L.data(), (int)L.size(), R.data(), (int)R.size(), ln, epi_thr,
                                                     max_disp, orient_thr_deg, out.lists.row_ptr.data(), out.lists.col_idx.data(),
                                                     out.orient_ok.data(), cap, &n);
            if (last_status != EBVO_ERR_CAPACITY)
                break;
            cap = n;
        }
        out.lists.col_idx.resize(last_status == EBVO_OK ? (size_t)n : 0);
        out.orient_ok.resize(out.lists.col_idx.size());
        report(*ctx_, last_status, "ebvo_epi_candidates_staged");
        return out;
    }

    // apply_NCC_Filtering (:555-616): candidates are explicit edges (TOED edges in the first pass,
    // cluster centres in the second); images are the RAW left / right images (:562-563).
    NccScores ncc(const uint8_t *imgL, const uint8_t *imgR, int rows, int cols, ptrdiff_t stepL, ptrdiff_t stepR,
                  const std::vector<EdgeT> &left, const std::vector<int32_t> &row_ptr,
                  const std::vector<EdgeT> &candidate_per_pair, double thr = EBVO_NCC_THRESH)
    {
        NccScores s;
        std::vector<ebvo_edge> L(left.size()), Rc(candidate_per_pair.size());
        for (size_t k = 0; k < left.size(); ++k)
            L[k] = to_abi(left[k]);
        for (size_t k = 0; k < Rc.size(); ++k)
            Rc[k] = to_abi(candidate_per_pair[k]);
        s.pp_nn_pn_np.resize(Rc.size() * 4);
        s.best.resize(Rc.size());
        s.keep.resize(Rc.size());
        s.left_patches.resize(left.size() * 98);
        last_status = ebvo_ncc_pairs(ctx_->get(), imgL, imgR, rows, cols, stepL, stepR, L.data(), (int)L.size(),
                                     Rc.data(), row_ptr.data(), thr, s.left_patches.data(), s.pp_nn_pn_np.data(),
                                     s.best.data(), s.keep.data());
        report(*ctx_, last_status, "ebvo_ncc_pairs");
        return s;
    }

    // ---- the same stages for a caller that hands back the vectors get_Third_Order_Edges gave it (main_VO as it is) ----
    // If `left` and `right` are exactly the edge lists still resident on the device (Context::resident), the stage runs on
    // the device copies and its results are views of page-locked memory of the context -- no edge list is uploaded, no result
    // vector is allocated; they stay valid until the next call of the same stage.  Otherwise (edges edited, other edges, a
    // call in between that used the library's slot 0) the host-buffer path above runs and the views point into `own`.
    // Same bits either way (tests/test_cpp_adapter.py).
    struct StagedView
    {
        Span<int32_t> row_ptr, col_idx;             // the lists after the epipolar and disparity stages
        Span<uint8_t> orient_ok;                    // per listed pair: passes the orientation stage
        Span<int32_t> row_ptr_final, col_idx_final; // the lists after the orientation stage (the flagged pairs, in order)
        bool resident = false;
        StagedCandidates own;
        CandidateLists own_final;
        StagedView() = default;
        StagedView(StagedView &&) = default;
        StagedView &operator=(StagedView &&) = default;
        StagedView(const StagedView &) = delete;
        size_t rows() const { return row_ptr.empty() ? 0 : row_ptr.size() - 1; }
    };
    StagedView candidates_staged_view(const std::vector<EdgeT> &left, const std::vector<EdgeT> &right,
                                      const std::vector<std::array<double, 3>> &lines,
                                      double epi_thr = EBVO_EPIPOLAR_LINE_DIST_THRESH, double max_disp = EBVO_MAX_DISPARITY,
                                      double orient_thr_deg = EBVO_ORIENT_THRESH_DEG)
    {
        StagedView out;
        const int wl = resident_workspace(*ctx_, left), wr = resident_workspace(*ctx_, right);
        if (wl >= 0 && wr >= 0 && wl != wr && lines.size() == left.size())
        {
            ebvo_candidates_view v;
            last_status = ebvo_epi_candidates_resident(ctx_->get(), ctx_->resident[wl].tag, ctx_->resident[wr].tag,
                                                       lines.empty() ? nullptr : lines[0].data(), epi_thr, max_disp, orient_thr_deg,
                                                       EBVO_STAGE_EPIPOLAR | EBVO_STAGE_DISPARITY, 1, &v);
            if (last_status == EBVO_OK)
            {
                out.resident = true;
                out.row_ptr = Span<int32_t>(v.row_ptr, left.size() + 1);
                out.col_idx = Span<int32_t>(v.col_idx, (size_t)v.n_pairs);
                out.orient_ok = Span<uint8_t>(v.orient_ok, (size_t)v.n_pairs);
                out.row_ptr_final = Span<int32_t>(v.row_ptr_final, left.size() + 1);
                out.col_idx_final = Span<int32_t>(v.col_idx_final, (size_t)v.n_final);
                return out;
            }
            if (last_status != EBVO_ERR_STATE) // a stale tag is not an error: the host-buffer path takes over
            {
                report(*ctx_, last_status, "ebvo_epi_candidates_resident");
                return out;
            }
            ctx_->resident[0] = ctx_->resident[1] = Context::ResidentEdges();
        }
        out.own = candidates_staged(left, right, lines, epi_thr, max_disp, orient_thr_deg);
        out.row_ptr = out.own.lists.row_ptr;
        out.col_idx = out.own.lists.col_idx;
        out.orient_ok = out.own.orient_ok;
        // the flagged pairs of every row, in order (branch-free: a slot is overwritten unless its pair is flagged)
        out.own_final.row_ptr.assign(out.row_ptr.size(), 0);
        out.own_final.col_idx.resize(out.col_idx.size());
        size_t n = 0;
        for (size_t i = 0; i + 1 < out.row_ptr.size(); ++i)
        {
            for (int32_t k = out.row_ptr[i]; k < out.row_ptr[i + 1]; ++k)
            {
                out.own_final.col_idx[n] = out.col_idx[(size_t)k];
                n += out.orient_ok[(size_t)k];
            }
            out.own_final.row_ptr[i + 1] = (int32_t)n;
        }
        out.own_final.col_idx.resize(n);
        out.row_ptr_final = out.own_final.row_ptr;
        out.col_idx_final = out.own_final.col_idx;
        return out;
    }

    // apply_NCC_Filtering in its first pass (:1427): candidate k of the lists is right[col_idx[k]] (a TOED edge,
    // contributing_edges_toed_indices[0], :413).  The four scores per pair only if asked for.
    struct NccView
    {
        Span<float> left_patches;     // nL x 2 x 49 (left_edge_patches, :578)
        Span<double> pp_nn_pn_np;     // 4 per pair, empty unless want_sims
        Span<double> best;            // final_SIM_score (:596)
        Span<uint8_t> keep;           // best > NCC_THRESH (:597)
        bool resident = false;
        NccScores own;
        NccView() = default;
        NccView(NccView &&) = default;
        NccView &operator=(NccView &&) = default;
        NccView(const NccView &) = delete;
    };
    NccView ncc_indexed(const uint8_t *imgL, const uint8_t *imgR, int rows, int cols, ptrdiff_t stepL, ptrdiff_t stepR,
                        const std::vector<EdgeT> &left, const std::vector<EdgeT> &right, Span<int32_t> row_ptr,
                        Span<int32_t> col_idx, double thr = EBVO_NCC_THRESH, bool want_sims = false)
    {
        NccView out;
        if (row_ptr.size() != left.size() + 1 || (left.size() && (size_t)row_ptr[left.size()] != col_idx.size()))
        {
            last_status = EBVO_ERR_ARG;
            report(*ctx_, last_status, "ncc_indexed: row_ptr / col_idx do not describe one list per left edge");
            return out;
        }
        const int wl = resident_workspace(*ctx_, left), wr = resident_workspace(*ctx_, right);
        if (wl >= 0 && wr >= 0 && wl != wr)
        {
            ebvo_ncc_view v;
            last_status = ebvo_ncc_pairs_resident(ctx_->get(), ctx_->resident[wl].tag, ctx_->resident[wr].tag, imgL, imgR, rows, cols,
                                                  stepL, stepR, row_ptr.data(), col_idx.data(), thr,
                                                  EBVO_NCC_WANT_LEFT_PATCHES | (want_sims ? EBVO_NCC_WANT_SIMS : 0), &v);
            if (last_status == EBVO_OK)
            {
                out.resident = true;
                out.left_patches = Span<float>(v.left_patches, (size_t)v.n_left * 98);
                out.pp_nn_pn_np = Span<double>(v.sims, v.sims ? (size_t)v.n_pairs * 4 : 0);
                out.best = Span<double>(v.best, (size_t)v.n_pairs);
                out.keep = Span<uint8_t>(v.keep, (size_t)v.n_pairs);
                return out;
            }
            if (last_status != EBVO_ERR_STATE)
            {
                report(*ctx_, last_status, "ebvo_ncc_pairs_resident");
                return out;
            }
            ctx_->resident[0] = ctx_->resident[1] = Context::ResidentEdges();
        }
        std::vector<EdgeT> cand(col_idx.size());
        for (size_t k = 0; k < cand.size(); ++k)
        {
            if ((size_t)col_idx[k] >= right.size())
            {
                last_status = EBVO_ERR_ARG;
                report(*ctx_, last_status, "ncc_indexed: candidate index outside the right edge list");
                return out;
            }
            cand[k] = right[(size_t)col_idx[k]];
        }
        std::vector<int32_t> rp(row_ptr.begin(), row_ptr.end());
        out.own = ncc(imgL, imgR, rows, cols, stepL, stepR, left, rp, cand, thr);
        out.left_patches = out.own.left_patches;
        if (want_sims)
            out.pp_nn_pn_np = out.own.pp_nn_pn_np;
        out.best = out.own.best;
        out.keep = out.own.keep;
        return out;
    }

    // refine_edge_disparity (:1290-1358): photometric Gauss-Newton of every (left edge, candidate centre) pair along
    // the epipolar line.  Images are the undistorted left / right images; pass them swapped for is_left = false.
    struct Refined
    {
        std::vector<double> alpha, score, confidence, xy; // xy: n_pairs x 2 updated centre locations (:1349-1351)
        std::vector<uint8_t> validity;                    // refine_validities; 2 = left undefined by the reference
        std::vector<int32_t> iters;
    };
    Refined refine(const uint8_t *imgL, const uint8_t *imgR, int rows, int cols, ptrdiff_t stepL, ptrdiff_t stepR,
                   const std::vector<EdgeT> &left, const std::vector<std::array<double, 3>> &lines,
                   const std::vector<int32_t> &row_ptr, const std::vector<double> &candidate_xy)
    {
        Refined r;
        const size_t n = candidate_xy.size() / 2;
        std::vector<ebvo_edge> L(left.size());
        for (size_t k = 0; k < left.size(); ++k)
            L[k] = to_abi(left[k]);
        r.alpha.resize(n);
        r.score.resize(n);
        r.confidence.resize(n);
        r.xy.resize(2 * n);
        r.validity.resize(n);
        r.iters.resize(n);
        ebvo_gn_params p;
        ebvo_gn_default_params(&p);
        last_status = ebvo_gn_refine_stereo(ctx_->get(), imgL, imgR, rows, cols, stepL, stepR, L.data(), (int)L.size(),
                                            lines.empty() ? nullptr : lines[0].data(), row_ptr.data(), candidate_xy.data(),
                                            &p, r.alpha.data(), r.score.data(), r.confidence.data(), r.validity.data(),
                                            r.iters.data(), r.xy.data());
        report(*ctx_, last_status, "ebvo_gn_refine_stereo");
        return r;
    }

    // ---- stage glue on flattened candidate lists (row_ptr + one entry per candidate) ------------------------------
    struct Selection
    {
        std::vector<int32_t> new_count; // survivors per row
        std::vector<int32_t> order;     // order[row_ptr[i] + k] = index of the k-th survivor of row i
    };
    // apply_Best_Nearly_Best_Test (:789-862): is_NCC -> scores = refine_final_scores, else refine_confidences
    Selection bnb_test(const std::vector<int32_t> &row_ptr, const std::vector<double> &scores, double ratio, bool is_NCC)
    {
        Selection sel;
        sel.new_count.assign(row_ptr.size() - 1, 0);
        sel.order.assign(scores.size(), -1);
        last_status = ebvo_bnb_test(ctx_->get(), row_ptr.data(), (int)row_ptr.size() - 1, scores.data(), ratio, is_NCC ? 1 : 0,
                                    sel.new_count.data(), sel.order.data());
        report(*ctx_, last_status, "ebvo_bnb_test");
        return sel;
    }
    // apply_Lowe_Ratio_Test as written (:916-964): the best candidate of every row
    Selection keep_best(const std::vector<int32_t> &row_ptr, const std::vector<double> &scores)
    {
        Selection sel;
        sel.new_count.assign(row_ptr.size() - 1, 0);
        sel.order.assign(scores.size(), -1);
        last_status = ebvo_keep_best(ctx_->get(), row_ptr.data(), (int)row_ptr.size() - 1, scores.data(), sel.new_count.data(),
                                     sel.order.data());
        report(*ctx_, last_status, "ebvo_keep_best");
        return sel;
    }
    // consolidate_redundant_edge_hypothesis, shift pass (:976-996): shift_Edge_to_Epipolar_Line of every candidate
    std::vector<ebvo_edge> epipolar_shift(const std::vector<EdgeT> &candidates, const std::vector<std::array<double, 3>> &lines,
                                          const std::vector<int32_t> &row_ptr)
    {
        std::vector<ebvo_edge> in(candidates.size()), out(candidates.size());
        for (size_t k = 0; k < in.size(); ++k)
            in[k] = to_abi(candidates[k]);
        last_status = ebvo_epipolar_shift(ctx_->get(), in.data(), lines.empty() ? nullptr : lines[0].data(), row_ptr.data(),
                                          (int)row_ptr.size() - 1, out.data());
        report(*ctx_, last_status, "ebvo_epipolar_shift");
        return out;
    }
    // consolidate_redundant_edge_hypothesis, clustering pass (:1006-1034): EdgeClusterer per row
    struct Clusters
    {
        std::vector<int32_t> new_count, cluster_of; // clusters per row; cluster index of every input candidate
        std::vector<ebvo_edge> centres;             // centres[row_ptr[i] + c], c < new_count[i]
    };
    Clusters cluster_rows(const std::vector<ebvo_edge> &candidates, const std::vector<int32_t> &row_ptr, bool by_orientation,
                          bool skip_single)
    {
        Clusters c;
        c.new_count.assign(row_ptr.size() - 1, 0);
        c.cluster_of.assign(candidates.size(), -1);
        c.centres.resize(candidates.size());
        last_status = ebvo_cluster_rows(ctx_->get(), candidates.data(), row_ptr.data(), (int)row_ptr.size() - 1,
                                        by_orientation ? 1 : 0, skip_single ? 1 : 0, c.new_count.data(), c.centres.data(),
                                        c.cluster_of.data());
        report(*ctx_, last_status, "ebvo_cluster_rows");
        return c;
    }

    // Temporal_Matches::min_Edge_Photometric_Residual_by_Gauss_Newton (src/Temporal_Matches.cpp:735-851) over n
    // (keyframe edge, current-frame edge, initial disparity) items of ONE camera, as apply_photometric_refinement_quads
    // issues them for the left and for the right image of every candidate quad (:605-610).
    struct RefinedTemporal
    {
        std::vector<double> disp, score; // disp: n x 2 refined_disparity; the new location is kf.location - disp
        std::vector<uint8_t> validity;
        std::vector<int32_t> iters;
    };
    RefinedTemporal refine_temporal(const uint8_t *imgKF, const uint8_t *imgCF, int rows, int cols, ptrdiff_t stepKF,
                                    ptrdiff_t stepCF, const std::vector<EdgeT> &kf, const std::vector<EdgeT> &cf,
                                    const std::vector<double> &init_disp)
    {
        RefinedTemporal r;
        const size_t n = kf.size();
        std::vector<ebvo_edge> K(n), C(n);
        for (size_t k = 0; k < n; ++k)
        {
            K[k] = to_abi(kf[k]);
            C[k] = to_abi(cf[k]);
        }
        r.disp.resize(2 * n);
        r.score.resize(n);
        r.validity.resize(n);
        r.iters.resize(n);
        ebvo_gn_params p;
        ebvo_gn_default_params(&p);
        last_status = ebvo_gn_refine_temporal(ctx_->get(), imgKF, imgCF, rows, cols, stepKF, stepCF, K.data(), C.data(),
                                              init_disp.data(), (int)n, &p, r.disp.data(), r.score.data(),
                                              r.validity.data(), r.iters.data());
        report(*ctx_, last_status, "ebvo_gn_refine_temporal");
        return r;
    }

    // Stereo_Matches::get_Stereo_Edge_Pairs (src/Stereo_Matches.cpp:1360-1540) for one frame in ONE pass over the device:
    // both TOED runs, the three geometric filters, [SIFT filter,] NCC, both Best-Nearly-Best tests, epipolar shift,
    // photometric refinement, shift + clustering, second NCC pass, best candidate per row -- images up, final pairs down,
    // every intermediate list stays in HBM (ebvo_stereo_upload_slot / submit / wait / finalize / fetch_final).  This is the
    // path a frame loop takes when it does not inspect the intermediate `matching_edge_clusters` between the stages; the
    // stage-wise calls above remain for a caller that does.
    struct FinalPairs
    {
        ebvo_stereo_counts stage1{};   // TOED edges, candidate pairs after the geometric filters, NCC matches
        ebvo_finalize_counts stages{}; // survivors of the later stages
        std::vector<ebvo_edge> left_edges;  // all kept TOED edges of the left image (stereo_frame->left_edges)
        std::vector<int32_t> left_index;    // per final pair: index into left_edges
        std::vector<ebvo_edge> right;       // per final pair: the matched right edge (a refined cluster centre)
        std::vector<double> ncc_score;      // per final pair
        std::vector<double> out16;          // per final pair: the 16 numbers of the output row (if calib was given)
    };
    FinalPairs stereo_edge_pairs(const uint8_t *imgL, const uint8_t *imgR, int rows, int cols, ptrdiff_t stepL, ptrdiff_t stepR,
                                 const double F21[9], const ebvo_stereo_calib *calib, bool use_sift = true, int slot = 0,
                                 const ebvo_stereo_params *stereo = nullptr, const ebvo_finalize_params *fin = nullptr)
    {
        FinalPairs r;
        ebvo_stereo_params sp;
        if (stereo)
            sp = *stereo;
        else
        {
            ebvo_stereo_default_params(&sp);
            std::memcpy(sp.F21, F21, sizeof sp.F21);
        }
        ebvo_finalize_params fp;
        if (fin)
            fp = *fin;
        else
        {
            ebvo_finalize_default_params(&fp);
            fp.use_sift = use_sift ? 1 : 0;
        }
        ebvo_ctx *c = ctx_->get();
        if (!report(*ctx_, last_status = ebvo_stereo_upload_slot(c, slot, imgL, imgR, rows, cols, stepL, stepR),
                    "ebvo_stereo_upload_slot") ||
            !report(*ctx_, last_status = ebvo_stereo_submit(c, slot, &sp), "ebvo_stereo_submit") ||
            !report(*ctx_, last_status = ebvo_stereo_wait(c, slot, &r.stage1), "ebvo_stereo_wait") ||
            !report(*ctx_, last_status = ebvo_stereo_finalize(c, slot, &fp, calib, &r.stages), "ebvo_stereo_finalize"))
            return r;
        const size_t n = (size_t)r.stages.n_final;
        r.left_edges.resize((size_t)r.stage1.n_left);
        r.left_index.resize(n);
        r.right.resize(n);
        r.ncc_score.resize(n);
        if (calib)
            r.out16.resize(16 * n);
        if (report(*ctx_, last_status = ebvo_stereo_fetch_slot(c, slot, r.left_edges.data(), nullptr, nullptr, nullptr, nullptr,
                                                               nullptr, nullptr, nullptr),
                   "ebvo_stereo_fetch_slot"))
            report(*ctx_, last_status = ebvo_stereo_fetch_final(c, slot, r.left_index.data(), r.right.data(),
                                                                r.ncc_score.data(), calib ? r.out16.data() : nullptr),
                   "ebvo_stereo_fetch_final");
        return r;
    }

    // The same in three enqueue-only steps for a frame loop that keeps several frames in flight (one slot each,
    // ebvo_stereo_set_slots): _begin uploads the pair and submits TOED + candidates + NCC; _chain reads their counts and
    // enqueues every later stage (no host synchronisation between the stages: their totals stay on the device); _end waits
    // for the chain and copies the final pairs back.  While the chain of frame k runs, the caller begins frame k + 1 and
    // ends frame k - 1: the chains of different slots overlap on the device (bench.py: dropin_final_pairs_per_s).
    bool stereo_edge_pairs_begin(const uint8_t *imgL, const uint8_t *imgR, int rows, int cols, ptrdiff_t stepL, ptrdiff_t stepR,
                                 const double F21[9], int slot, const ebvo_stereo_params *stereo = nullptr)
    {
        ebvo_stereo_params sp;
        if (stereo)
            sp = *stereo;
        else
        {
            ebvo_stereo_default_params(&sp);
            std::memcpy(sp.F21, F21, sizeof sp.F21);
        }
        ebvo_ctx *c = ctx_->get();
        return report(*ctx_, last_status = ebvo_stereo_upload_slot(c, slot, imgL, imgR, rows, cols, stepL, stepR),
                      "ebvo_stereo_upload_slot") &&
               report(*ctx_, last_status = ebvo_stereo_submit(c, slot, &sp), "ebvo_stereo_submit");
    }
    bool stereo_edge_pairs_chain(int slot, const ebvo_stereo_calib *calib, bool use_sift = true, ebvo_stereo_counts *stage1 = nullptr,
                                 const ebvo_finalize_params *fin = nullptr)
    {
        ebvo_finalize_params fp;
        if (fin)
            fp = *fin;
        else
        {
            ebvo_finalize_default_params(&fp);
            fp.use_sift = use_sift ? 1 : 0;
        }
        ebvo_stereo_counts tmp{};
        ebvo_ctx *c = ctx_->get();
        return report(*ctx_, last_status = ebvo_stereo_wait(c, slot, stage1 ? stage1 : &tmp), "ebvo_stereo_wait") &&
               report(*ctx_, last_status = ebvo_stereo_finalize_submit(c, slot, &fp, calib), "ebvo_stereo_finalize_submit");
    }
    FinalPairs stereo_edge_pairs_end(int slot, bool with_rows, int n_left_edges = -1)
    {
        FinalPairs r;
        ebvo_ctx *c = ctx_->get();
        if (!report(*ctx_, last_status = ebvo_stereo_finalize_wait(c, slot, &r.stages), "ebvo_stereo_finalize_wait"))
            return r;
        const size_t n = (size_t)r.stages.n_final;
        r.left_index.resize(n);
        r.right.resize(n);
        r.ncc_score.resize(n);
        if (with_rows)
            r.out16.resize(16 * n);
        if (n_left_edges >= 0)
        {
            r.left_edges.resize((size_t)n_left_edges);
            if (!report(*ctx_, last_status = ebvo_stereo_fetch_slot(c, slot, r.left_edges.data(), nullptr, nullptr, nullptr, nullptr,
                                                                    nullptr, nullptr, nullptr),
                        "ebvo_stereo_fetch_slot"))
                return r;
        }
        report(*ctx_, last_status = ebvo_stereo_fetch_final(c, slot, r.left_index.data(), r.right.data(), r.ncc_score.data(),
                                                            with_rows ? r.out16.data() : nullptr),
               "ebvo_stereo_fetch_final");
        return r;
    }

  private:
    Context::Ptr ctx_;
};

// Temporal_Matches::get_Temporal_Edge_Pairs_from_Quads (src/Temporal_Matches.cpp:168-218) on the FINAL stereo mates of
// resident pairs: the keyframe's mates stay on the device (set_keyframe after StereoMatcherHIP::stereo_edge_pairs on that
// slot), every later frame's mates are matched against them.  stages = 0 stops after the NCC filter (:192), 1 runs the
// SIFT filter, both Best-Nearly-Best tests, the photometric refinement and the edge clustering as well.
class TemporalMatcherHIP
{
  public:
    explicit TemporalMatcherHIP(Context::Ptr ctx) : ctx_(std::move(ctx)) {}
    int last_status = EBVO_OK;

    bool set_keyframe(int slot = 0) // keyframe = frame 0 in the reference (src/Pipeline.cpp:133-138)
    {
        return report(*ctx_, last_status = ebvo_temporal_set_keyframe(ctx_->get(), slot), "ebvo_temporal_set_keyframe");
    }

    struct Quads
    {
        ebvo_temporal_counts counts{};
        // per keyframe mate i: the quads row_ptr[i] .. row_ptr[i + 1] that left the chain
        std::vector<int32_t> row_ptr, cf_index;
        std::vector<ebvo_edge> left, right; // cluster centres (CF_left / CF_right center_edge)
        std::vector<double> ncc_left, sift_left, refine_score_left, refine_score_right;
        std::vector<uint8_t> refine_validity;
    };
    // The pose the NEXT match of `slot` searches under (ebvo_temporal_set_prior): row-major R and t of the relative pose
    // keyframe -> current frame, in the convention of MotionTrackerHIP's result (ebvo::predict_pose forms one from the last
    // two).  One-shot: the next successful match consumes it, set_keyframe drops it.  This project's own: the reference
    // always searches around the keyframe position.
    bool set_prior(const double *R, const double *t, const ebvo_stereo_calib &calib, const ebvo_tprior_params *params = nullptr,
                   int slot = 0)
    {
        return report(*ctx_, last_status = ebvo_temporal_set_prior(ctx_->get(), slot, R, t, &calib, params), "ebvo_temporal_set_prior");
    }
    bool clear_prior(int slot = 0)
    {
        return report(*ctx_, last_status = ebvo_temporal_clear_prior(ctx_->get(), slot), "ebvo_temporal_clear_prior");
    }

    Quads match(int slot = 0, int stages = 1, const ebvo_temporal_params *params = nullptr)
    {
        Quads q;
        ebvo_temporal_params p;
        if (params)
            p = *params;
        else
        {
            ebvo_temporal_default_params(&p);
            p.stages = stages;
        }
        if (!report(*ctx_, last_status = ebvo_temporal_match(ctx_->get(), slot, &p, &q.counts), "ebvo_temporal_match") || !p.stages)
            return q;
        const size_t n = (size_t)q.counts.n_final;
        q.row_ptr.resize((size_t)q.counts.n_kf + 1);
        q.cf_index.resize(n);
        q.left.resize(n);
        q.right.resize(n);
        q.ncc_left.resize(n);
        q.sift_left.resize(n);
        q.refine_score_left.resize(n);
        q.refine_score_right.resize(n);
        q.refine_validity.resize(n);
        report(*ctx_,
               last_status = ebvo_temporal_fetch_final(ctx_->get(), slot, q.row_ptr.data(), q.cf_index.data(), q.left.data(),
                                                       q.right.data(), q.ncc_left.data(), q.sift_left.data(),
                                                       q.refine_score_left.data(), q.refine_score_right.data(),
                                                       q.refine_validity.data()),
               "ebvo_temporal_fetch_final");
        return q;
    }

  private:
    Context::Ptr ctx_;
};

// MotionTracker (src/MotionTracker.cpp): estimate_Relative_Pose_From_Quad_Pairs on the final quads a TemporalMatcherHIP left
// in `slot` (match with stages = 1) against the keyframe -- the quads never leave the device.  The options and the state
// mirror Ransac_Options / Ransac_State (include/MotionTracker.h); `opt` defaults to the reference's values (plus TAU_C1..4).
// Returns false, with the identity pose, where the reference returns false (fewer than two quads to sample) and on an error
// (last_status); a search that hit the draw cap (pose.status = 2) returns true with the best hypothesis so far.
// On a slot armed with ground truth (ebvo_temporal_set_gt after the match), gt_rows = true runs the search the reference runs
// under has_gt() -- over the quads of the listed, true-positive keyframe mates -- and Solution_Constraints_Application /
// Print_Quad_Pairs_Metrics_Statistics (:255-434) report the recall and precision of the four quad-pair constraints.
class MotionTrackerHIP
{
  public:
    explicit MotionTrackerHIP(Context::Ptr ctx, const ebvo_stereo_calib &calib) : ctx_(std::move(ctx)), calib_(calib) {}
    int last_status = EBVO_OK;

    struct Ransac_Options
    {
        ebvo_pose_params p;
        Ransac_Options() { ebvo_pose_default_params(&p); }
    };
    struct Ransac_State
    {
        std::array<double, 9> R{{1, 0, 0, 0, 1, 0, 0, 0, 1}}; // best_pose_hypothesis, row-major
        std::array<double, 3> t{{0, 0, 0}};
        size_t iterations = 0;
        double inlier_ratio = 0;
        size_t best_minimal_inlier_count = 0;
        size_t dynamic_max_iter = 0;
        std::vector<uint8_t> inliers; // per final quad (CSR order of TemporalMatcherHIP::Quads) when asked for
        ebvo_pose_result pose{};      // every field of the search
        ebvo_pose_refined refined{};  // what refine_Relative_Pose left: the refitted pose and every field of the refit
    };
    struct Refine_Options
    {
        ebvo_pose_refine_params p;
        Refine_Options() { ebvo_pose_refine_default_params(&p); }
    };

    struct Quad_Pair_Evaluation_Metrics // include/MotionTracker.h
    {
        std::string stage_name;
        double recall;
        double precision;
        size_t num_of_surviving_veridical_quad_pairs;
    };

    bool estimate_Relative_Pose_From_Quad_Pairs(int slot, const Ransac_Options &opt, Ransac_State &state, bool want_inliers = false,
                                                bool gt_rows = false)
    {
        state = Ransac_State();
        int32_t n_kf = 0;
        int64_t n_final = 0;
        last_status = ebvo_temporal_final_size(ctx_->get(), slot, &n_kf, &n_final); // the slot's own count sizes the mask
        if (!report(*ctx_, last_status, "ebvo_temporal_final_size"))
            return false;
        if (want_inliers)
            state.inliers.assign((size_t)n_final, 0);
        uint8_t *mask = want_inliers ? state.inliers.data() : nullptr;
        last_status = gt_rows ? ebvo_temporal_estimate_pose_gt(ctx_->get(), slot, &calib_, &opt.p, &state.pose, mask)
                              : ebvo_temporal_estimate_pose(ctx_->get(), slot, &calib_, &opt.p, &state.pose, mask);
        if (!report(*ctx_, last_status, gt_rows ? "ebvo_temporal_estimate_pose_gt" : "ebvo_temporal_estimate_pose"))
            return false;
        const ebvo_pose_result &r = state.pose;
        std::copy(r.R, r.R + 9, state.R.begin());
        std::copy(r.t, r.t + 3, state.t.begin());
        state.iterations = (size_t)r.iterations;
        state.inlier_ratio = r.inlier_ratio;
        state.best_minimal_inlier_count = (size_t)r.best_inliers;
        state.dynamic_max_iter = (size_t)r.dynamic_max_iter;
        return r.status != 1;
    }

    // The inlier refit (this project's own; the reference never fits its best hypothesis): Gauss-Newton over both cameras
    // from the start pose in state.R / state.t (what the search left there) on the quads the search ran on.  The refitted
    // pose and the refit's fields are left in state.refined, state.R / state.t stay the start pose; state.inliers holds the
    // inliers of the refitted pose when asked for.  Returns true when the pose was refined (refined.status == 0).
    bool refine_Relative_Pose(int slot, const Ransac_Options &opt, const Refine_Options &refine_opt, Ransac_State &state,
                              bool gt_rows = false, bool want_inliers = false)
    {
        state.refined = ebvo_pose_refined{};
        int32_t n_kf = 0;
        int64_t n_final = 0;
        last_status = ebvo_temporal_final_size(ctx_->get(), slot, &n_kf, &n_final);
        if (!report(*ctx_, last_status, "ebvo_temporal_final_size"))
            return false;
        if (want_inliers)
            state.inliers.assign((size_t)n_final, 0);
        last_status = ebvo_temporal_refine_pose(ctx_->get(), slot, &calib_, &opt.p, &refine_opt.p, state.R.data(), state.t.data(),
                                                gt_rows ? 1 : 0, &state.refined, want_inliers ? state.inliers.data() : nullptr);
        if (!report(*ctx_, last_status, "ebvo_temporal_refine_pose"))
            return false;
        return state.refined.status == 0;
    }

    // The alignment of a pose to the current frame's TOED edges by normal distance (this project's own; the contract is in
    // ebvo_hip.h): the keyframe mates' 3-D points are projected under the pose, associated with the nearest edge of compatible
    // orientation in each image and the distances along the edges' normals minimised, re-associating every round.  It needs
    // neither quads nor finalisation of the current frame.  NOTE: camera 1 uses the TRUE K_right of the calibration, unlike
    // the search and the refit above (K_right := K_left).
    struct Align_Options
    {
        ebvo_align_params p;
        Align_Options() { ebvo_align_default_params(&p); }
    };
    struct Align_State
    {
        std::array<double, 9> R{{1, 0, 0, 0, 1, 0, 0, 0, 1}}; // in: the start pose; stays as given
        std::array<double, 3> t{{0, 0, 0}};
        ebvo_aligned_pose aligned{};                           // out: the aligned pose and every field of the stage
        std::vector<int32_t> assoc_left, assoc_right;          // per keyframe mate: edge index or -1, when asked for
    };

    // the context's keyframe against the TOED edge lists the slot's waited pair left resident; true when aligned.status == 0
    bool align_Relative_Pose(int slot, const Align_Options &opt, Align_State &state, bool want_assoc = false)
    {
        state.aligned = ebvo_aligned_pose{};
        int32_t n_kf = 0, n0 = 0, n1 = 0;
        last_status = ebvo_temporal_align_size(ctx_->get(), slot, &n_kf, &n0, &n1);
        if (!report(*ctx_, last_status, "ebvo_temporal_align_size"))
            return false;
        size_assoc(state, want_assoc ? (size_t)n_kf : 0);
        last_status = ebvo_temporal_align_pose(ctx_->get(), slot, &calib_, &opt.p, state.R.data(), state.t.data(), &state.aligned,
                                               want_assoc ? state.assoc_left.data() : nullptr,
                                               want_assoc ? state.assoc_right.data() : nullptr);
        if (!report(*ctx_, last_status, "ebvo_temporal_align_pose"))
            return false;
        return state.aligned.status == 0;
    }

    // the same on host arrays: keyframe mates and the two edge lists of a frame of img_w x img_h (edges_right may be empty
    // with opt.p.cameras = 1)
    bool align_Relative_Pose(const std::vector<ebvo_edge> &kf_left, const std::vector<ebvo_edge> &kf_right,
                             const std::vector<ebvo_edge> &edges_left, const std::vector<ebvo_edge> &edges_right, int img_w, int img_h,
                             const Align_Options &opt, Align_State &state, bool want_assoc = false)
    {
        state.aligned = ebvo_aligned_pose{};
        if (kf_left.size() != kf_right.size())
        {
            last_status = EBVO_ERR_ARG;
            return false;
        }
        size_assoc(state, want_assoc ? kf_left.size() : 0);
        last_status = ebvo_pose_align_edges(ctx_->get(), kf_left.data(), kf_right.data(), (int)kf_left.size(), edges_left.data(),
                                            (int)edges_left.size(), edges_right.empty() ? nullptr : edges_right.data(),
                                            (int)edges_right.size(), img_w, img_h, &calib_, &opt.p, state.R.data(), state.t.data(),
                                            &state.aligned, want_assoc ? state.assoc_left.data() : nullptr,
                                            want_assoc ? state.assoc_right.data() : nullptr);
        if (!report(*ctx_, last_status, "ebvo_pose_align_edges"))
            return false;
        return state.aligned.status == 0;
    }

    // The inverse-depth filter of the keyframe mates (this project's own; the contract is in ebvo_hip.h): every aligned frame
    // refines lambda_i, the ratio of mate i's triangulated depth to the refined one, from the normal distances of its
    // projections to the edges they were associated with.
    struct Depth_Options
    {
        ebvo_depth_params p;
        Depth_Options() { ebvo_depth_default_params(&p); }
    };
    struct Mate_Depths
    {
        std::vector<double> lambda, info;   // per keyframe mate; empty lambda on the way in: the prior
        std::vector<int32_t> n_obs;
        std::vector<uint8_t> flags;         // EBVO_DEPTH_* of the last update
        ebvo_depth_refined refined{};       // the last update's record
    };

    // one update of the context's keyframe from the slot's waited pair under the pose (state.R, state.t); the association
    // takes its radius, cell size and orientation threshold from align_opt
    bool refine_Mate_Depths(int slot, const Align_Options &align_opt, const Depth_Options &opt, const Align_State &state,
                            ebvo_depth_refined &refined)
    {
        refined = ebvo_depth_refined{};
        last_status = ebvo_temporal_refine_depth(ctx_->get(), slot, &calib_, &align_opt.p, &opt.p, state.R.data(), state.t.data(), &refined);
        return report(*ctx_, last_status, "ebvo_temporal_refine_depth");
    }

    // the same on host arrays, with the associations an alignment returned (state.assoc_left / assoc_right); depths is the
    // incoming state (empty lambda: the prior) and the outgoing one
    bool refine_Mate_Depths(const std::vector<ebvo_edge> &kf_left, const std::vector<ebvo_edge> &kf_right,
                            const std::vector<ebvo_edge> &edges_left, const std::vector<ebvo_edge> &edges_right, int img_w, int img_h,
                            const Depth_Options &opt, const Align_State &state, Mate_Depths &depths)
    {
        const size_t n = kf_left.size();
        depths.refined = ebvo_depth_refined{};
        const bool prior = depths.lambda.empty() && n > 0;
        if (kf_right.size() != n || (!state.assoc_left.empty() && state.assoc_left.size() != n) ||
            (!state.assoc_right.empty() && state.assoc_right.size() != n) ||
            (!prior && (depths.lambda.size() != n || depths.info.size() != n || depths.n_obs.size() != n)))
        {
            last_status = EBVO_ERR_ARG;
            return false;
        }
        depths.lambda.resize(n);
        depths.info.resize(n);
        depths.n_obs.resize(n);
        depths.flags.assign(n, 0);
        last_status = ebvo_depth_refine_edges(
            ctx_->get(), kf_left.data(), kf_right.data(), (int)n, edges_left.data(), (int)edges_left.size(),
            edges_right.empty() ? nullptr : edges_right.data(), (int)edges_right.size(), state.assoc_left.empty() ? nullptr : state.assoc_left.data(),
            state.assoc_right.empty() ? nullptr : state.assoc_right.data(), img_w, img_h, &calib_, &opt.p, state.R.data(), state.t.data(),
            prior ? nullptr : depths.lambda.data(), prior ? nullptr : depths.info.data(), prior ? nullptr : depths.n_obs.data(),
            depths.lambda.data(), depths.info.data(), depths.n_obs.data(), depths.flags.data(), &depths.refined);
        return report(*ctx_, last_status, "ebvo_depth_refine_edges");
    }

    // the keyframe's resident state (n_kf of the slot's ebvo_temporal_align_size)
    bool mate_depths(int slot, Mate_Depths &depths)
    {
        int32_t n_kf = 0, n0 = 0, n1 = 0;
        last_status = ebvo_temporal_align_size(ctx_->get(), slot, &n_kf, &n0, &n1);
        if (!report(*ctx_, last_status, "ebvo_temporal_align_size"))
            return false;
        depths.lambda.assign((size_t)n_kf, 1.0);
        depths.info.assign((size_t)n_kf, 0.0);
        depths.n_obs.assign((size_t)n_kf, 0);
        depths.flags.assign((size_t)n_kf, 0);
        last_status = ebvo_temporal_depth_fetch(ctx_->get(), depths.lambda.data(), depths.info.data(), depths.n_obs.data(), depths.flags.data());
        return report(*ctx_, last_status, "ebvo_temporal_depth_fetch");
    }

    bool reset_Mate_Depths()
    {
        last_status = ebvo_temporal_depth_reset(ctx_->get());
        return report(*ctx_, last_status, "ebvo_temporal_depth_reset");
    }

    // while on, align_Relative_Pose(slot, ...) works on the refined points Gamma / lambda; default off
    bool use_Mate_Depths(bool on)
    {
        last_status = ebvo_temporal_use_depth(ctx_->get(), on ? 1 : 0);
        return report(*ctx_, last_status, "ebvo_temporal_use_depth");
    }

    // The handover of the refined depths when the current frame becomes the keyframe (this project's own; the contract is in
    // ebvo_hip.h): each new mate takes the depth the nearest old projection of compatible orientation predicts for it and
    // fuses it with its own triangulation prior.  When to switch stays the caller's decision.
    struct Carry_Options
    {
        ebvo_depth_carry_params p;
        Carry_Options() { ebvo_depth_carry_default_params(&p); }
    };
    struct Carried_Depths
    {
        Mate_Depths depths;             // the NEW keyframe's mates (depths.refined is not used)
        std::vector<int32_t> src_index; // per new mate: the old mate it took its depth from, or -1
        ebvo_depth_carried carried{};
    };

    // the slot's finalised pair becomes the keyframe and inherits the old keyframe's depths through the pose (state.R, state.t),
    // old keyframe -> this frame
    bool promote_Keyframe(int slot, const Carry_Options &opt, const Align_State &state, ebvo_depth_carried &carried)
    {
        carried = ebvo_depth_carried{};
        last_status = ebvo_temporal_promote_keyframe(ctx_->get(), slot, &calib_, &opt.p, state.R.data(), state.t.data(), &carried);
        return report(*ctx_, last_status, "ebvo_temporal_promote_keyframe");
    }

    // the same on host arrays: `old_depths` is the old mates' state (empty lambda: nothing to carry, the priors alone)
    bool carry_Mate_Depths(const std::vector<ebvo_edge> &kf_left, const std::vector<ebvo_edge> &kf_right, const Mate_Depths &old_depths,
                           const std::vector<ebvo_edge> &new_left, const std::vector<ebvo_edge> &new_right, int img_w, int img_h,
                           const Carry_Options &opt, const Align_State &state, Carried_Depths &out)
    {
        const size_t no = kf_left.size(), nn = new_left.size();
        out.carried = ebvo_depth_carried{};
        const bool none = old_depths.lambda.empty();
        if (kf_right.size() != no || new_right.size() != nn ||
            (!none && (old_depths.lambda.size() != no || old_depths.info.size() != no || old_depths.n_obs.size() != no)))
        {
            last_status = EBVO_ERR_ARG;
            return false;
        }
        out.depths.lambda.assign(nn, 1.0);
        out.depths.info.assign(nn, 0.0);
        out.depths.n_obs.assign(nn, 0);
        out.depths.flags.assign(nn, 0);
        out.src_index.assign(nn, -1);
        last_status = ebvo_depth_carry(ctx_->get(), kf_left.data(), kf_right.data(), (int)no, none ? nullptr : old_depths.lambda.data(),
                                       none ? nullptr : old_depths.info.data(), none ? nullptr : old_depths.n_obs.data(), new_left.data(),
                                       new_right.data(), (int)nn, img_w, img_h, &calib_, &opt.p, state.R.data(), state.t.data(),
                                       out.depths.lambda.data(), out.depths.info.data(), out.depths.n_obs.data(), out.depths.flags.data(),
                                       out.src_index.data(), &out.carried);
        return report(*ctx_, last_status, "ebvo_depth_carry");
    }

    // src_index of the last promote_Keyframe (n_kf of the slot's ebvo_temporal_align_size)
    bool mate_depth_sources(int slot, std::vector<int32_t> &src_index)
    {
        int32_t n_kf = 0, n0 = 0, n1 = 0;
        last_status = ebvo_temporal_align_size(ctx_->get(), slot, &n_kf, &n0, &n1);
        if (!report(*ctx_, last_status, "ebvo_temporal_align_size"))
            return false;
        src_index.assign((size_t)n_kf, -1);
        last_status = ebvo_temporal_depth_source(ctx_->get(), src_index.data());
        return report(*ctx_, last_status, "ebvo_temporal_depth_source");
    }

    // How much of the keyframe still explains the current frame and how much of the current frame it does not explain, the
    // policy that reads the measurement and one call per frame that ties the stages together (this project's own; the
    // contract is in ebvo_hip.h).
    struct Cover_Options
    {
        ebvo_cover_params p;
        Cover_Options() { ebvo_cover_default_params(&p); }
    };
    struct Switch_Policy
    {
        ebvo_keyframe_policy p;
        Switch_Policy() { ebvo_keyframe_policy_default(&p); }
    };
    struct Keyframe_Coverage
    {
        ebvo_keyframe_cover cover{};
        std::vector<uint8_t> flags;      // per keyframe mate: EBVO_COVER_*                    (the arrays when asked for)
        std::vector<int32_t> assoc;      // per keyframe mate: edge index or -1
        std::vector<double> disp;        // per keyframe mate: displacement from its keyframe position, NaN when not in frame
        std::vector<uint8_t> explained;  // per current left edge
        std::vector<int32_t> cell_edges, cell_explained; // cover.cw * cover.ch
    };

    // the context's keyframe against the slot's waited pair under the pose (state.R, state.t)
    bool keyframe_Coverage(int slot, const Cover_Options &opt, const Align_State &state, Keyframe_Coverage &out, bool want_arrays = false)
    {
        out = Keyframe_Coverage{};
        if (want_arrays)
        {
            int32_t n_kf = 0, n0 = 0, cw = 0, ch = 0;
            last_status = ebvo_temporal_cover_size(ctx_->get(), slot, &opt.p, &n_kf, &n0, &cw, &ch);
            if (!report(*ctx_, last_status, "ebvo_temporal_cover_size"))
                return false;
            size_cover(out, (size_t)n_kf, (size_t)n0, (size_t)cw * (size_t)ch);
        }
        last_status = ebvo_temporal_keyframe_cover(ctx_->get(), slot, &calib_, &opt.p, state.R.data(), state.t.data(), &out.cover,
                                                   want_arrays ? out.flags.data() : nullptr, want_arrays ? out.assoc.data() : nullptr,
                                                   want_arrays ? out.disp.data() : nullptr, want_arrays ? out.explained.data() : nullptr,
                                                   want_arrays ? out.cell_edges.data() : nullptr,
                                                   want_arrays ? out.cell_explained.data() : nullptr);
        return report(*ctx_, last_status, "ebvo_temporal_keyframe_cover");
    }

    // the same on host arrays: keyframe mates, their lambda (empty: the triangulated depths) and the left edge list of a frame
    // of img_w x img_h
    bool keyframe_Coverage(const std::vector<ebvo_edge> &kf_left, const std::vector<ebvo_edge> &kf_right, const std::vector<double> &lambda,
                           const std::vector<ebvo_edge> &edges_left, int img_w, int img_h, const Cover_Options &opt, const Align_State &state,
                           Keyframe_Coverage &out, bool want_arrays = true)
    {
        out = Keyframe_Coverage{};
        const size_t n = kf_left.size();
        if (kf_right.size() != n || (!lambda.empty() && lambda.size() != n) || img_w < 1 || img_h < 1 || opt.p.cover_cell < 1)
        {
            last_status = EBVO_ERR_ARG;
            return false;
        }
        if (want_arrays)
            size_cover(out, n, edges_left.size(),
                       (size_t)((img_w + (int64_t)opt.p.cover_cell - 1) / opt.p.cover_cell) *
                           (size_t)((img_h + (int64_t)opt.p.cover_cell - 1) / opt.p.cover_cell));
        last_status = ebvo_keyframe_cover_edges(ctx_->get(), kf_left.data(), kf_right.data(), lambda.empty() ? nullptr : lambda.data(), (int)n,
                                                edges_left.data(), (int)edges_left.size(), img_w, img_h, &calib_, &opt.p, state.R.data(),
                                                state.t.data(), &out.cover, want_arrays ? out.flags.data() : nullptr,
                                                want_arrays ? out.assoc.data() : nullptr, want_arrays ? out.disp.data() : nullptr,
                                                want_arrays ? out.explained.data() : nullptr, want_arrays ? out.cell_edges.data() : nullptr,
                                                want_arrays ? out.cell_explained.data() : nullptr);
        return report(*ctx_, last_status, "ebvo_keyframe_cover_edges");
    }

    // 0 keep, 1 switch, 2 lost; reasons: EBVO_KF_* bits.  A pure host function of the record.
    int should_Switch_Keyframe(const ebvo_keyframe_cover &cover, const Switch_Policy &policy, uint32_t *reasons = nullptr) const
    {
        return ebvo_keyframe_decide(&cover, &policy.p, reasons);
    }

    struct Track_Options
    {
        ebvo_track_params p;
        Track_Options() { ebvo_track_default_params(&p); }
    };

    // One frame on a slot whose pair has been waited for: align from (state.R, state.t), refine the keyframe's depths, measure
    // the coverage, decide and -- on decision 1 -- finalise the slot and promote it.  true when the frame was tracked
    // (frame.tracked == 1); a refusal leaves last_status and frame.failed_stage.
    bool track_Frame(int slot, const Track_Options &opt, const Align_State &state, ebvo_tracked_frame &frame)
    {
        frame = ebvo_tracked_frame{};
        last_status = ebvo_temporal_track_frame(ctx_->get(), slot, &calib_, &opt.p, state.R.data(), state.t.data(), &frame);
        if (!report(*ctx_, last_status, "ebvo_temporal_track_frame"))
            return false;
        return frame.tracked == 1;
    }

    // the keyframe's pose in the sequence frame: X_kf = R X_seq + t (the identity after set_Keyframe, composed by every promotion)
    bool keyframe_Pose(std::array<double, 9> &R, std::array<double, 3> &t)
    {
        last_status = ebvo_temporal_keyframe_pose(ctx_->get(), R.data(), t.data());
        return report(*ctx_, last_status, "ebvo_temporal_keyframe_pose");
    }

    // n_runs calls of the reference's Solution_Constraints_Application (src/Pipeline.cpp:198-203 makes 20) in one device
    // call: one vector of five stages per run.  Empty on an error (last_status) and when the slot has too few quads.
    std::vector<std::vector<Quad_Pair_Evaluation_Metrics>> Solution_Constraints_Application(int slot, const Ransac_Options &opt,
                                                                                             int n_runs = 1)
    {
        static const char *const names[EBVO_PC_NUM_STAGES] = {"Baseline", "Normalized Length Constraint",
                                                              "T1 Angle Similarity Constraint", "T2 Angle Similarity Constraint",
                                                              "Tangent Angle Similarity Constraint"};
        std::vector<std::vector<Quad_Pair_Evaluation_Metrics>> out;
        std::vector<ebvo_pose_cascade_run> runs((size_t)(n_runs > 0 ? n_runs : 0));
        last_status = ebvo_temporal_pose_constraint_metrics(ctx_->get(), slot, &calib_, &opt.p, n_runs, runs.data(), nullptr, nullptr);
        if (!report(*ctx_, last_status, "ebvo_temporal_pose_constraint_metrics"))
            return out;
        for (const ebvo_pose_cascade_run &r : runs)
        {
            if (r.status != 0)
                continue;
            std::vector<Quad_Pair_Evaluation_Metrics> m;
            for (const ebvo_pose_cascade_stage &g : r.stages)
                m.push_back({names[g.stage], g.recall, g.precision, (size_t)g.veridical});
            out.push_back(std::move(m));
        }
        return out;
    }

    // the per-stage means over the runs, formed and laid out as the reference does (:383-434)
    static void Print_Quad_Pairs_Metrics_Statistics(const std::vector<std::vector<Quad_Pair_Evaluation_Metrics>> &all, std::ostream &os)
    {
        if (all.empty() || all.front().empty())
            return;
        os << "\n===== Quad Pair Constraints Metrics (Solution Constraints Application) =====" << std::endl;
        os << "               Stage               |         Recall         |        Precision       |       Number of Surviving "
              "Veridical Quad Pairs"
           << std::endl;
        for (const auto &ref_metric : all.front())
        {
            double sum_recall = 0.0, sum_precision = 0.0;
            std::size_t sum_num_veridical = 0, count = 0;
            for (const auto &per_run : all)
            {
                auto it = std::find_if(per_run.begin(), per_run.end(), [&ref_metric](const Quad_Pair_Evaluation_Metrics &m) {
                    return m.stage_name == ref_metric.stage_name;
                });
                if (it != per_run.end())
                {
                    sum_recall += it->recall;
                    sum_precision += it->precision;
                    sum_num_veridical += it->num_of_surviving_veridical_quad_pairs;
                    ++count;
                }
            }
            if (count > 0)
                os << std::setw(35) << ref_metric.stage_name << " | " << std::setw(20) << sum_recall / static_cast<double>(count) << " | "
                   << std::setw(20) << sum_precision / static_cast<double>(count) << " | " << std::setw(20)
                   << sum_num_veridical / static_cast<double>(count) << std::endl;
        }
        os << std::endl;
    }

  private:
    static void size_assoc(Align_State &state, size_t n)
    {
        state.assoc_left.assign(n, -1);
        state.assoc_right.assign(n, -1);
    }
    static void size_cover(Keyframe_Coverage &out, size_t n_kf, size_t n0, size_t n_cells)
    {
        out.flags.assign(n_kf, 0);
        out.assoc.assign(n_kf, -1);
        out.disp.assign(n_kf, std::numeric_limits<double>::quiet_NaN());
        out.explained.assign(n0, 0);
        out.cell_edges.assign(n_cells, 0);
        out.cell_explained.assign(n_cells, 0);
    }
    Context::Ptr ctx_;
    ebvo_stereo_calib calib_;
};

// The error of a relative pose (row-major R, t) against the true one, on the host: the angle of E = R_gt^T R as
// atan2(|vee(E - E^T)| / 2, (tr E - 1) / 2) in degrees, |t - t_gt|, and the angle between t and t_gt in degrees (NaN when
// either is zero).  The metric of the reference's commented-out evaluate_Pose_Accuracy.
struct PoseError
{
    double rot_deg, trans_abs, trans_dir_deg;
};
inline PoseError pose_error(const double *R, const double *t, const double *R_gt, const double *t_gt)
{
    double E[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            E[i * 3 + j] = R_gt[i] * R[j] + R_gt[3 + i] * R[3 + j] + R_gt[6 + i] * R[6 + j];
    const double deg = 180.0 / 3.14159265358979323846;
    const double v[3] = {E[7] - E[5], E[2] - E[6], E[3] - E[1]};
    const double d[3] = {t[0] - t_gt[0], t[1] - t_gt[1], t[2] - t_gt[2]};
    const double x[3] = {t[1] * t_gt[2] - t[2] * t_gt[1], t[2] * t_gt[0] - t[0] * t_gt[2], t[0] * t_gt[1] - t[1] * t_gt[0]};
    auto norm = [](const double *a) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); };
    PoseError e;
    e.rot_deg = std::atan2(norm(v) / 2.0, (E[0] + E[4] + E[8] - 1.0) / 2.0) * deg;
    e.trans_abs = norm(d);
    e.trans_dir_deg = norm(t) == 0.0 || norm(t_gt) == 0.0 ? std::nan("")
                                                          : std::atan2(norm(x), t[0] * t_gt[0] + t[1] * t_gt[1] + t[2] * t_gt[2]) * deg;
    return e;
}

// Constant-velocity prediction of the next relative pose keyframe -> frame, for TemporalMatcherHIP::set_prior, on the host
// (the twin of api.predict_pose): the step of the last two poses, T_k T_{k-1}^-1, applied once more to T_k.  Row-major R.
// prev2_R == nullptr (one earlier pose only): the last pose itself.
struct PredictedPose
{
    std::array<double, 9> R;
    std::array<double, 3> t;
};
inline PredictedPose predict_pose(const double *prev_R, const double *prev_t, const double *prev2_R = nullptr,
                                  const double *prev2_t = nullptr)
{
    PredictedPose out;
    if (!prev2_R || !prev2_t)
    {
        std::copy(prev_R, prev_R + 9, out.R.begin());
        std::copy(prev_t, prev_t + 3, out.t.begin());
        return out;
    }
    double D[9], d[3]; // T_k T_{k-1}^-1 = (R_k R_{k-1}^T, t_k - D t_{k-1})
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            D[i * 3 + j] = prev_R[i * 3] * prev2_R[j * 3] + prev_R[i * 3 + 1] * prev2_R[j * 3 + 1] + prev_R[i * 3 + 2] * prev2_R[j * 3 + 2];
    for (int i = 0; i < 3; ++i)
        d[i] = prev_t[i] - (D[i * 3] * prev2_t[0] + D[i * 3 + 1] * prev2_t[1] + D[i * 3 + 2] * prev2_t[2]);
    for (int i = 0; i < 3; ++i)
    {
        for (int j = 0; j < 3; ++j)
            out.R[i * 3 + j] = D[i * 3] * prev_R[j] + D[i * 3 + 1] * prev_R[3 + j] + D[i * 3 + 2] * prev_R[6 + j];
        out.t[i] = D[i * 3] * prev_t[0] + D[i * 3 + 1] * prev_t[1] + D[i * 3 + 2] * prev_t[2] + d[i];
    }
    return out;
}

// Frame_Evaluation_Metrics (include/Stereo_Matches.h): what get_Stereo_Edge_Pairs returns on a dataset with ground truth --
// one (name, recall / precision / pair precision / ambiguity) entry per stage the chain ran, in pipeline order.
struct StageMetrics
{
    double recall = 0.0, precision = 0.0, precision_pair = 0.0, ambiguity = 0.0;
};
struct FrameEvaluationMetrics
{
    std::vector<std::pair<std::string, StageMetrics>> stages; // preserves pipeline order
    std::vector<ebvo_gt_stage> totals;                        // the same stages with their integer totals
    int status = EBVO_OK;
};

// Find_Stereo_GT_Locations + get_Stereo_Edge_GT_Pairs (src/Stereo_Matches.cpp:133-268) on the pair that ran in `slot`:
// arms the slot with the CV_32F left disparity map (disp0GT.pfm; step in floats).  Call it before
// ebvo_stereo_finalize / get_Stereo_Edge_Pairs_resident so that every stage is evaluated, then evaluate() below.
inline bool set_ground_truth(const Context &c, int slot, const float *disparity, int rows, int cols, ptrdiff_t step_elems,
                             const ebvo_stereo_calib &calib, const ebvo_gt_params *params = nullptr)
{
    return report(c, ebvo_stereo_set_gt(c.get(), slot, disparity, rows, cols, step_elems, &calib, params), "ebvo_stereo_set_gt");
}

// Evaluate_Stereo_Edge_Correspondences after every stage (:1377-1536) of the armed slot, under the reference's stage names
// ("NCC" twice, as there); stages the chain did not run are left out.
inline FrameEvaluationMetrics evaluate(const Context &c, int slot)
{
    static const char *const names[EBVO_GT_NUM_STAGES] = {"Epipolar Proximity", "Location Proximity", "Orientation", "SIFT", "NCC",
                                                          "BNB-NCC", "BNB-SIFT", "Photometric Refinement", "Edge Clustering", "NCC",
                                                          "Best", "Final"};
    FrameEvaluationMetrics out;
    ebvo_gt_stage st[EBVO_GT_NUM_STAGES];
    const int n = ebvo_stereo_gt_metrics(c.get(), slot, st);
    if (n < 0)
    {
        out.status = n;
        report(c, n, "ebvo_stereo_gt_metrics");
        return out;
    }
    for (int k = 0; k < n; ++k)
        if (st[k].present)
        {
            StageMetrics m;
            m.recall = st[k].recall;
            m.precision = st[k].precision;
            m.precision_pair = st[k].precision_pair;
            m.ambiguity = st[k].ambiguity;
            out.stages.emplace_back(names[st[k].stage], m);
            out.totals.push_back(st[k]);
        }
    return out;
}

// A camera pose as the reference's Camera_Pose holds it (row-major R, t: X_camera = R X_world + t)
struct CameraPose
{
    double R[9], t[3];
};

// Utility::get_Relative_Pose (src/utility.cpp:121-128): rel_R = target.R * source.R^T, rel_T = -rel_R * source.t + target.t
inline CameraPose relative_pose(const CameraPose &source, const CameraPose &target)
{
    CameraPose rel;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            rel.R[i * 3 + j] = (target.R[i * 3] * source.R[j * 3] + target.R[i * 3 + 1] * source.R[j * 3 + 1]) + target.R[i * 3 + 2] * source.R[j * 3 + 2];
    for (int i = 0; i < 3; ++i)
        rel.t[i] = (((-rel.R[i * 3]) * source.t[0] + (-rel.R[i * 3 + 1]) * source.t[1]) + (-rel.R[i * 3 + 2]) * source.t[2]) + target.t[i];
    return rel;
}

// The slot's NEXT temporal match keeps (on) or drops (off) its stage trail (ebvo_temporal_keep_stages): with it, evaluate()
// below returns every stage of get_Temporal_Edge_Pairs_from_Quads.  The match's own results are the same either way.
inline int temporal_keep_stages(const Context &c, int slot, bool on)
{
    const int rc = ebvo_temporal_keep_stages(c.get(), slot, on ? 1 : 0);
    if (rc != EBVO_OK)
        report(c, rc, "ebvo_temporal_keep_stages");
    return rc;
}

// build_Veridical_Quads + Evaluate_Temporal_Edge_Pairs_on_Quads (src/Temporal_Matches.cpp:57-166, :220-292) on the temporal
// match of `slot`: arms it with the relative pose of the two GT camera poses (keyframe, current frame) and returns the
// stages the match formed under the reference's names, in its order: "Orientation", "NCC", and "Edge Clustering" after
// stages = 1; a match made after temporal_keep_stages(c, slot, true) also gives "Location Proximity" and, after stages = 1,
// "SIFT", "BNB-NCC", "BNB-SIFT" and "Photometric Refinement" -- the reference's eight.
// kf_gamma (n_kf x 3) / kf_is_tp (n_kf): the keyframe mates' GT 3-D points and b_is_TP, or nullptr (ebvo_hip.h).
inline FrameEvaluationMetrics evaluate(const Context &c, int slot, const CameraPose &keyframe_gt_pose, const CameraPose &current_gt_pose,
                                       const ebvo_stereo_calib &calib, const ebvo_tgt_params *params = nullptr,
                                       const double *kf_gamma = nullptr, const uint8_t *kf_is_tp = nullptr)
{
    static const char *const names[EBVO_TGT_NUM_STAGES] = {"Location Proximity", "Orientation", "NCC", "SIFT", "BNB-NCC", "BNB-SIFT",
                                                           "Photometric Refinement", "Edge Clustering"};
    FrameEvaluationMetrics out;
    const CameraPose rel = relative_pose(keyframe_gt_pose, current_gt_pose);
    out.status = ebvo_temporal_set_gt(c.get(), slot, rel.R, rel.t, &calib, params, kf_gamma, kf_is_tp);
    if (out.status != EBVO_OK)
    {
        report(c, out.status, "ebvo_temporal_set_gt");
        return out;
    }
    ebvo_gt_stage st[EBVO_TGT_NUM_STAGES];
    const int n = ebvo_temporal_gt_metrics(c.get(), slot, st);
    if (n < 0)
    {
        out.status = n;
        report(c, n, "ebvo_temporal_gt_metrics");
        return out;
    }
    for (int k = 0; k < n; ++k)
        if (st[k].present)
        {
            StageMetrics m;
            m.recall = st[k].recall;
            m.precision = st[k].precision;
            m.precision_pair = st[k].precision_pair;
            m.ambiguity = st[k].ambiguity;
            out.stages.emplace_back(names[st[k].stage], m);
            out.totals.push_back(st[k]);
        }
    return out;
}

// cv::undistort(src, dst, K, dist) of src/Pipeline.cpp:78-79 on a CV_8UC1 image (K = fx fy cx cy, dist = k1 k2 p1 p2 [k3])
inline std::vector<uint8_t> undistort(const Context &c, const uint8_t *img, int rows, int cols, ptrdiff_t step, const double K[4],
                                      const std::vector<double> &dist)
{
    std::vector<uint8_t> out((size_t)rows * cols);
    const int rc = ebvo_undistort(c.get(), img, rows, cols, step, K, dist.data(), (int)dist.size(), out.data(), cols);
    if (!report(c, rc, "ebvo_undistort"))
        out.clear();
    return out;
}

// The two SIFT descriptors of every edge (cv::SIFT::create()->compute at the +-8 px points; src/Stereo_Matches.cpp:669-677,
// :720-727, :1628-1634): n x 2 x 128 floats, descriptor of shifted_points.first then of .second.
template <class EdgeT>
inline std::vector<float> sift_descriptors(const Context &c, const uint8_t *img, int rows, int cols, ptrdiff_t step,
                                           const std::vector<EdgeT> &edges)
{
    std::vector<ebvo_edge> e(edges.size());
    for (size_t k = 0; k < edges.size(); ++k)
        e[k] = to_abi(edges[k]);
    std::vector<float> out(256 * edges.size());
    const int rc = ebvo_sift_descriptors(c.get(), img, rows, cols, step, e.data(), (int)e.size(), out.data());
    if (!report(c, rc, "ebvo_sift_descriptors"))
        out.clear();
    return out;
}

// apply_SIFT_filtering's score per candidate pair (:736-740): cand_desc holds one descriptor pair per pair of the CSR lists
inline std::vector<double> sift_min_distances(const Context &c, const std::vector<float> &left_desc,
                                              const std::vector<float> &cand_desc, const std::vector<int32_t> &row_ptr)
{
    std::vector<double> d(cand_desc.size() / 256);
    const int rc = ebvo_sift_min_distances(c.get(), left_desc.data(), (int)(left_desc.size() / 256), cand_desc.data(),
                                           row_ptr.data(), d.data());
    if (!report(c, rc, "ebvo_sift_min_distances"))
        d.clear();
    return d;
}


// Utility::get_patch_similarity on two 7x7 CV_32F patches (src/utility.cpp:163-180); also the shape
// of MatlabNCCComputer::computeNCC(patch1, patch2) -> double (include/MatlabNCCComputer.h:41): NaN
// on failure, like the MATLAB wrapper (src/MatlabNCCComputer.cpp:58-90).
inline double patch_similarity(const Context &c, const float *patch_one, const float *patch_two)
{
    double s = 0;
    const int rc = ebvo_ncc_patches(c.get(), patch_one, patch_two, 1, &s);
    if (!report(c, rc, "ebvo_ncc_patches"))
        return __builtin_nan("");
    return s;
}

// The numeric body of Stereo_Matches::write_finalized_stereo_edge_pairs_to_file (src/Stereo_Matches.cpp:1656-1699):
// 16 numbers per final (left edge, right edge) pair, computed on the device.
template <class EdgeT>
inline std::vector<double> finalize_pairs(const Context &c, const ebvo_stereo_calib &calib, const std::vector<EdgeT> &left,
                                          const std::vector<EdgeT> &right)
{
    std::vector<ebvo_edge> L(left.size()), R(right.size());
    for (size_t k = 0; k < left.size(); ++k)
        L[k] = to_abi(left[k]);
    for (size_t k = 0; k < right.size(); ++k)
        R[k] = to_abi(right[k]);
    std::vector<double> out(16 * left.size());
    const int rc = ebvo_finalize_pairs(c.get(), &calib, L.data(), R.data(), (int)L.size(), out.data());
    if (!report(c, rc, "ebvo_finalize_pairs"))
        out.clear();
    return out;
}

// ... and its text: the header line and one row of 16 space-separated numbers per pair, through the same iostream
// insertions as the reference (:1660, :1690-1695), hence the same default formatting (6 significant digits).
inline bool write_finalized_stereo_edge_pairs(const std::string &filename, const std::vector<double> &out16)
{
    std::ofstream outfile(filename);
    if (!outfile)
        return false;
    outfile << "left_edge_location, left_edge_orientation, right_edge_location, right_edge_orientation, "
               "left_edge_3D_point, left_edge_tangent"
            << std::endl;
    for (size_t k = 0; k + 16 <= out16.size(); k += 16)
    {
        const double *o = &out16[k];
        outfile << o[0] << " " << o[1] << " " << o[2] << " " << o[3] << " " << o[4] << " " << o[5] << " " << o[6] << " "
                << o[7] << " " << o[8] << " " << o[9] << " " << o[10] << " " << o[11] << " " << o[12] << " " << o[13] << " "
                << o[14] << " " << o[15] << std::endl;
    }
    return (bool)outfile;
}

} // namespace ebvo
#endif
