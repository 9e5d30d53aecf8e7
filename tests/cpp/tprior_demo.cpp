// tprior_demo.cpp -- TemporalMatcherHIP::set_prior + match (include/ebvo/adapters.hpp): the temporal chain of a current frame
// against a keyframe under a pose prior; compiled with plain g++ against the C ABI alone.
// usage: tprior_demo <in.bin> <out.bin>     (no arguments: prints ebvo::predict_pose of a hand-composed pair of poses)
// in.bin:  int32 h, w; double F21[9]; ebvo_stereo_calib; double R[9], t[3], grid_radius; int32 use_orientation, pad;
//          keyframe left, right, current left, right images (h * w bytes each)
// out.bin: ebvo_temporal_counts; row_ptr [n_kf + 1], cf_index [n] (int32); left, right [n] (ebvo_edge); ncc_left, sift_left,
//          score_left, score_right [n] (double); valid [n] (bytes); then int32 status of a second match, which is unprimed
//          (the prior is one-shot), and its int64 candidate count
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "ebvo/adapters.hpp"

struct Point2d
{
    double x, y;
};
struct Edge
{
    Point2d location{-1.0, -1.0};
    double orientation = -100;
    bool b_isEmpty = true;
    int frame_source = -1;
    int index = 0;
};

struct Header
{
    int32_t h, w;
    double F[9];
    ebvo_stereo_calib calib;
    double R[9], t[3], grid_radius;
    int32_t use_orientation, pad;
};

template <class T>
static void put(FILE *o, const std::vector<T> &v)
{
    if (!v.empty())
        std::fwrite(v.data(), sizeof(T), v.size(), o);
}

int main(int argc, char **argv)
{
    if (argc != 3)
    {
        // T1 = (Rz(90 deg), (1, 0, 0)), the step D = (Rz(90 deg), (0, 0, 2)): T2 = D T1, and the prediction is D T2
        const double R1[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, t1[3] = {1, 0, 0};
        const double R2[9] = {-1, 0, 0, 0, -1, 0, 0, 0, 1}, t2[3] = {0, 1, 2};
        const ebvo::PredictedPose p = ebvo::predict_pose(R2, t2, R1, t1), same = ebvo::predict_pose(R2, t2);
        std::printf("predict");
        for (double v : p.R)
            std::printf(" %.17g", v);
        for (double v : p.t)
            std::printf(" %.17g", v);
        std::printf("\nlast");
        for (double v : same.R)
            std::printf(" %.17g", v);
        for (double v : same.t)
            std::printf(" %.17g", v);
        std::printf("\n");
        return 0;
    }
    FILE *f = std::fopen(argv[1], "rb");
    Header hd;
    if (!f || std::fread(&hd, sizeof hd, 1, f) != 1)
        return 2;
    const size_t px = (size_t)hd.h * hd.w;
    std::vector<unsigned char> img[4];
    for (auto &b : img)
    {
        b.resize(px);
        if (std::fread(b.data(), 1, px, f) != px)
            return 2;
    }
    std::fclose(f);
    auto ctx = std::make_shared<ebvo::Context>(hd.h, hd.w);
    if (ctx->status() != EBVO_OK)
        return 3;
    ebvo::StereoMatcherHIP<Edge> matcher(ctx);
    ebvo::TemporalMatcherHIP temporal(ctx);
    matcher.stereo_edge_pairs(img[0].data(), img[1].data(), hd.h, hd.w, hd.w, hd.w, hd.F, &hd.calib, false);
    if (matcher.last_status != EBVO_OK || !temporal.set_keyframe(0))
        return 4;
    matcher.stereo_edge_pairs(img[2].data(), img[3].data(), hd.h, hd.w, hd.w, hd.w, hd.F, &hd.calib, false);
    if (matcher.last_status != EBVO_OK)
        return 5;
    ebvo_tprior_params pp;
    ebvo_tprior_default_params(&pp);
    pp.use_orientation = hd.use_orientation;
    ebvo_temporal_params tp;
    ebvo_temporal_default_params(&tp);
    tp.stages = 1;
    tp.grid_radius = hd.grid_radius;
    // set + clear + set: the cleared prior leaves nothing behind
    if (!temporal.set_prior(hd.R, hd.t, hd.calib) || !temporal.clear_prior() || !temporal.set_prior(hd.R, hd.t, hd.calib, &pp))
        return 6;
    const ebvo::TemporalMatcherHIP::Quads q = temporal.match(0, 1, &tp);
    if (temporal.last_status != EBVO_OK)
        return 7;
    tp.stages = 0;
    const ebvo::TemporalMatcherHIP::Quads again = temporal.match(0, 0, &tp);
    const int32_t again_status = temporal.last_status;
    FILE *o = std::fopen(argv[2], "wb");
    if (!o)
        return 8;
    std::fwrite(&q.counts, sizeof q.counts, 1, o);
    put(o, q.row_ptr);
    put(o, q.cf_index);
    put(o, q.left);
    put(o, q.right);
    put(o, q.ncc_left);
    put(o, q.sift_left);
    put(o, q.refine_score_left);
    put(o, q.refine_score_right);
    put(o, q.refine_validity);
    std::fwrite(&again_status, sizeof again_status, 1, o);
    std::fwrite(&again.counts.n_candidates, sizeof again.counts.n_candidates, 1, o);
    std::fclose(o);
    std::printf("tprior_demo ok: %lld candidates, %lld final quads\n", (long long)q.counts.n_candidates, (long long)q.counts.n_final);
    return 0;
}
