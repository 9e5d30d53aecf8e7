// carry_demo.cpp -- MotionTrackerHIP::carry_Mate_Depths (include/ebvo/adapters.hpp) on host arrays: the old keyframe's mates
// and their state and the new keyframe's mates of a tiny scene read from files, carried once with the state and once without
// (the priors alone); compiled with plain g++ against the C ABI alone.
// usage: carry_demo <kf_left.bin> <kf_right.bin> <state.bin> <new_left.bin> <new_right.bin> <pose.bin> <w> <h> <carry> <out.bin>
//   *.bin of edges: packed ebvo_edge records; state.bin: lambda, info (n_old doubles each), n_obs (n_old int32); pose.bin: 42
//   doubles -- K_left, K_right, R21 (9 each), T21 (3), R (9), t (3)
//   (no arguments: prints the default options)
// out.bin, per pass: ebvo_depth_carried; lambda, info (n_new doubles each), n_obs, src_index (n_new int32 each), flags (n_new bytes).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "ebvo/adapters.hpp"

static std::vector<char> slurp(const char *path)
{
    std::vector<char> v;
    FILE *f = std::fopen(path, "rb");
    if (!f)
    {
        std::fprintf(stderr, "cannot read %s\n", path);
        std::exit(2);
    }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)bytes);
    if (bytes && std::fread(v.data(), 1, v.size(), f) != v.size())
    {
        std::fprintf(stderr, "short read: %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
    return v;
}

static std::vector<ebvo_edge> edges(const char *path)
{
    const std::vector<char> b = slurp(path);
    if (b.size() % sizeof(ebvo_edge))
        std::exit(2);
    std::vector<ebvo_edge> e(b.size() / sizeof(ebvo_edge));
    if (!e.empty())
        std::memcpy(e.data(), b.data(), b.size());
    return e;
}

int main(int argc, char **argv)
{
    ebvo::MotionTrackerHIP::Carry_Options opt;
    if (argc != 11)
    {
        std::printf("sigma_disp_px %g radius %g cell_size %d min_obs %d orient_thr_deg %g carry %g gate_sigmas %g lambda_min %g lambda_max %g "
                    "info_max %g img_margin %g reserved %d pad %d\n",
                    opt.p.sigma_disp_px, opt.p.radius, opt.p.cell_size, opt.p.min_obs, opt.p.orient_thr_deg, opt.p.carry, opt.p.gate_sigmas,
                    opt.p.lambda_min, opt.p.lambda_max, opt.p.info_max, opt.p.img_margin, opt.p.reserved, opt.p.pad);
        return 0;
    }
    const auto kfL = edges(argv[1]), kfR = edges(argv[2]), nL = edges(argv[4]), nR = edges(argv[5]);
    const std::vector<char> st = slurp(argv[3]), pb = slurp(argv[6]);
    const size_t no = kfL.size(), nn = nL.size();
    if (pb.size() != 42 * sizeof(double) || st.size() != 20 * no)
        return 2;
    double pose[42];
    std::memcpy(pose, pb.data(), sizeof pose);
    const int w = std::atoi(argv[7]), h = std::atoi(argv[8]);
    opt.p.carry = std::atof(argv[9]);
    auto ctx = std::make_shared<ebvo::Context>(h, w);
    if (ctx->status() != EBVO_OK)
        return 3;
    ebvo_stereo_calib calib;
    std::memcpy(calib.K_left, pose, sizeof(double) * 9);
    std::memcpy(calib.K_right, pose + 9, sizeof(double) * 9);
    std::memcpy(calib.R21, pose + 18, sizeof(double) * 9);
    std::memcpy(calib.T21, pose + 27, sizeof(double) * 3);
    ebvo::MotionTrackerHIP tracker(ctx, calib);
    ebvo::MotionTrackerHIP::Align_State state;
    std::memcpy(state.R.data(), pose + 30, sizeof(double) * 9);
    std::memcpy(state.t.data(), pose + 39, sizeof(double) * 3);
    ebvo::MotionTrackerHIP::Mate_Depths old_depths;
    old_depths.lambda.resize(no);
    old_depths.info.resize(no);
    old_depths.n_obs.resize(no);
    if (no)
    {
        std::memcpy(old_depths.lambda.data(), st.data(), 8 * no);
        std::memcpy(old_depths.info.data(), st.data() + 8 * no, 8 * no);
        std::memcpy(old_depths.n_obs.data(), st.data() + 16 * no, 4 * no);
    }
    FILE *f = std::fopen(argv[10], "wb");
    if (!f)
        return 5;
    for (int pass = 0; pass < 2; ++pass)
    {
        ebvo::MotionTrackerHIP::Carried_Depths out;
        if (!tracker.carry_Mate_Depths(kfL, kfR, pass == 0 ? old_depths : ebvo::MotionTrackerHIP::Mate_Depths(), nL, nR, w, h, opt, state, out))
            return 4;
        const ebvo_depth_carried &r = out.carried;
        std::printf("pass %d n_old %d sources %d live %d n_new %d dead %d assoc %d carried %d gated %d\n", pass, r.n_old, r.n_sources, r.n_live,
                    r.n_new, r.n_dead, r.n_assoc, r.n_carried, r.n_gated);
        std::fwrite(&r, sizeof r, 1, f);
        std::fwrite(out.depths.lambda.data(), sizeof(double), nn, f);
        std::fwrite(out.depths.info.data(), sizeof(double), nn, f);
        std::fwrite(out.depths.n_obs.data(), sizeof(int32_t), nn, f);
        std::fwrite(out.src_index.data(), sizeof(int32_t), nn, f);
        std::fwrite(out.depths.flags.data(), 1, nn, f);
    }
    std::fclose(f);
    return 0;
}
