// depth_demo.cpp -- MotionTrackerHIP::refine_Mate_Depths (include/ebvo/adapters.hpp) on host arrays: the keyframe mates, the
// two TOED edge lists and the associations of a tiny scene read from files, fused twice (from the prior, then from the state
// the first update left); compiled with plain g++ against the C ABI alone.
// usage: depth_demo <kf_left.bin> <kf_right.bin> <edges_left.bin> <edges_right.bin> <assoc.bin> <pose.bin> <w> <h> <iterations> <out.bin>
//   *.bin of edges: packed ebvo_edge records; assoc.bin: assoc_left then assoc_right, n_kf int32 each; pose.bin: 42 doubles --
//   K_left, K_right, R21 (9 each), T21 (3), R (9), t (3)
//   (no arguments: prints the default options)
// out.bin, per update: ebvo_depth_refined; lambda, info (n_kf doubles each), n_obs (n_kf int32), flags (n_kf bytes).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "ebvo/adapters.hpp"

template <class T> static std::vector<T> slurp(const char *path)
{
    std::vector<T> v;
    FILE *f = std::fopen(path, "rb");
    if (!f)
    {
        std::fprintf(stderr, "cannot read %s\n", path);
        std::exit(2);
    }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes / sizeof(T));
    if (bytes % (long)sizeof(T) || (bytes && std::fread(v.data(), sizeof(T), v.size(), f) != v.size()))
    {
        std::fprintf(stderr, "bad size or short read: %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

int main(int argc, char **argv)
{
    ebvo::MotionTrackerHIP::Depth_Options opt;
    if (argc != 11)
    {
        std::printf("sigma_disp_px %g sigma_normal_px %g huber_px %g gate_px %g iterations %d cameras %d lambda_min %g lambda_max %g "
                    "info_max %g img_margin %g block_threads %d reserved %d\n",
                    opt.p.sigma_disp_px, opt.p.sigma_normal_px, opt.p.huber_px, opt.p.gate_px, opt.p.iterations, opt.p.cameras,
                    opt.p.lambda_min, opt.p.lambda_max, opt.p.info_max, opt.p.img_margin, opt.p.block_threads, opt.p.reserved);
        return 0;
    }
    const auto kfL = slurp<ebvo_edge>(argv[1]), kfR = slurp<ebvo_edge>(argv[2]), E0 = slurp<ebvo_edge>(argv[3]), E1 = slurp<ebvo_edge>(argv[4]);
    const auto assoc = slurp<int32_t>(argv[5]);
    const auto pose = slurp<double>(argv[6]);
    const size_t n = kfL.size();
    if (pose.size() != 42 || assoc.size() != 2 * n)
        return 2;
    const int w = std::atoi(argv[7]), h = std::atoi(argv[8]);
    opt.p.iterations = std::atoi(argv[9]);
    auto ctx = std::make_shared<ebvo::Context>(h, w);
    if (ctx->status() != EBVO_OK)
        return 3;
    ebvo_stereo_calib calib;
    std::memcpy(calib.K_left, pose.data(), sizeof(double) * 9);
    std::memcpy(calib.K_right, pose.data() + 9, sizeof(double) * 9);
    std::memcpy(calib.R21, pose.data() + 18, sizeof(double) * 9);
    std::memcpy(calib.T21, pose.data() + 27, sizeof(double) * 3);
    ebvo::MotionTrackerHIP tracker(ctx, calib);
    ebvo::MotionTrackerHIP::Align_State state;
    std::memcpy(state.R.data(), pose.data() + 30, sizeof(double) * 9);
    std::memcpy(state.t.data(), pose.data() + 39, sizeof(double) * 3);
    state.assoc_left.assign(assoc.begin(), assoc.begin() + (long)n);
    state.assoc_right.assign(assoc.begin() + (long)n, assoc.end());
    FILE *f = std::fopen(argv[10], "wb");
    if (!f)
        return 5;
    ebvo::MotionTrackerHIP::Mate_Depths depths; // empty: the prior
    for (int pass = 0; pass < 2; ++pass)
    {
        if (!tracker.refine_Mate_Depths(kfL, kfR, E0, E1, w, h, opt, state, depths))
            return 4;
        const ebvo_depth_refined &r = depths.refined;
        std::printf("update %d n_kf %d dead %d updated %d restored %d terms %d %d gated %d %d rms %.17g -> %.17g\n", pass, r.n_kf, r.n_dead,
                    r.n_updated, r.n_restored, r.n_terms[0], r.n_terms[1], r.n_gated[0], r.n_gated[1], r.rms_before, r.rms_after);
        std::fwrite(&r, sizeof r, 1, f);
        std::fwrite(depths.lambda.data(), sizeof(double), n, f);
        std::fwrite(depths.info.data(), sizeof(double), n, f);
        std::fwrite(depths.n_obs.data(), sizeof(int32_t), n, f);
        std::fwrite(depths.flags.data(), 1, n, f);
    }
    std::fclose(f);
    return 0;
}
