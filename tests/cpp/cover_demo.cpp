// cover_demo.cpp -- MotionTrackerHIP::keyframe_Coverage and should_Switch_Keyframe (include/ebvo/adapters.hpp) on host arrays:
// the keyframe's mates, their lambda and the current frame's left edges of a tiny scene read from files, measured once on
// Gamma / lambda and once on the triangulated Gamma; compiled with plain g++ against the C ABI alone.
// usage: cover_demo <kf_left.bin> <kf_right.bin> <lambda.bin> <edges_left.bin> <pose.bin> <w> <h> <cover_cell> <out.bin>
//   *.bin of edges: packed ebvo_edge records; lambda.bin: n_kf doubles; pose.bin: 42 doubles -- K_left, K_right, R21 (9 each),
//   T21 (3), R (9), t (3)
//   (no arguments: prints the default options, one line per struct)
// out.bin, per pass: ebvo_keyframe_cover; decision, reasons (int32 each); disp (n_kf doubles); assoc (n_kf int32); cell_edges,
// cell_explained (cw * ch int32 each); flags (n_kf bytes); explained (n0 bytes).
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
    ebvo::MotionTrackerHIP::Cover_Options opt;
    ebvo::MotionTrackerHIP::Switch_Policy policy;
    if (argc != 10)
    {
        std::printf("radius %g orient_thr_deg %g img_margin %g inlier_px %g bin_px %g cell_size %d cover_cell %d min_cell_edges %d "
                    "min_cell_explained %d reserved %d pad %d\n",
                    opt.p.radius, opt.p.orient_thr_deg, opt.p.img_margin, opt.p.inlier_px, opt.p.bin_px, opt.p.cell_size, opt.p.cover_cell,
                    opt.p.min_cell_edges, opt.p.min_cell_explained, opt.p.reserved, opt.p.pad);
        std::printf("min_assoc %d max_disp_bins %d min_in_frame_share %g min_assoc_share %g min_cell_cover %g\n", policy.p.min_assoc,
                    policy.p.max_disp_bins, policy.p.min_in_frame_share, policy.p.min_assoc_share, policy.p.min_cell_cover);
        return 0;
    }
    const auto kfL = edges(argv[1]), kfR = edges(argv[2]), E0 = edges(argv[4]);
    const std::vector<char> lb = slurp(argv[3]), pb = slurp(argv[5]);
    const size_t n = kfL.size(), n0 = E0.size();
    if (pb.size() != 42 * sizeof(double) || lb.size() != 8 * n)
        return 2;
    double pose[42];
    std::memcpy(pose, pb.data(), sizeof pose);
    std::vector<double> lambda(n);
    if (n)
        std::memcpy(lambda.data(), lb.data(), 8 * n);
    const int w = std::atoi(argv[6]), h = std::atoi(argv[7]);
    opt.p.cover_cell = std::atoi(argv[8]);
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
    FILE *f = std::fopen(argv[9], "wb");
    if (!f)
        return 5;
    for (int pass = 0; pass < 2; ++pass)
    {
        ebvo::MotionTrackerHIP::Keyframe_Coverage out;
        if (!tracker.keyframe_Coverage(kfL, kfR, pass == 0 ? lambda : std::vector<double>(), E0, w, h, opt, state, out))
            return 4;
        const ebvo_keyframe_cover &r = out.cover;
        uint32_t reasons = 0;
        const int32_t decision = tracker.should_Switch_Keyframe(r, policy, &reasons);
        std::printf("pass %d n_kf %d dead %d in_frame %d assoc %d inliers %d edges %d explained %d cells %d of %d median_bin %d decision %d "
                    "reasons %u\n",
                    pass, r.n_kf, r.n_dead, r.n_in_frame, r.n_assoc, r.n_inliers, r.n_edges, r.n_explained, r.n_cells_covered, r.n_cells_cur,
                    r.disp_median_bin, decision, reasons);
        const int32_t dr[2] = {decision, (int32_t)reasons};
        std::fwrite(&r, sizeof r, 1, f);
        std::fwrite(dr, sizeof dr, 1, f);
        std::fwrite(out.disp.data(), sizeof(double), n, f);
        std::fwrite(out.assoc.data(), sizeof(int32_t), n, f);
        std::fwrite(out.cell_edges.data(), sizeof(int32_t), out.cell_edges.size(), f);
        std::fwrite(out.cell_explained.data(), sizeof(int32_t), out.cell_explained.size(), f);
        std::fwrite(out.flags.data(), 1, n, f);
        std::fwrite(out.explained.data(), 1, n0, f);
    }
    std::fclose(f);
    return 0;
}
