// align_demo.cpp -- MotionTrackerHIP::align_Relative_Pose (include/ebvo/adapters.hpp) on host arrays: the keyframe mates and
// the two TOED edge lists of a tiny scene read from files; compiled with plain g++ against the C ABI alone.
// usage: align_demo <kf_left.bin> <kf_right.bin> <edges_left.bin> <edges_right.bin> <pose.bin> <w> <h> <rounds> <iterations> <out.bin>
//   *.bin of edges: packed ebvo_edge records; pose.bin: 42 doubles -- K_left, K_right, R21 (9 each), T21 (3), R0 (9), t0 (3)
//   (no arguments: prints the default options)
// out.bin: ebvo_aligned_pose; assoc_left and assoc_right, n_kf int32 each.  The pose bits are printed as hex words too.
#include <cinttypes>
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
    ebvo::MotionTrackerHIP::Align_Options opt;
    if (argc != 11)
    {
        std::printf("rounds %d iterations %d radius %g cell_size %d orient_thr_deg %g huber_px %g inlier_px %g step_eps %g min_terms %d "
                    "img_margin %g cameras %d block_threads %d\n",
                    opt.p.rounds, opt.p.iterations, opt.p.radius, opt.p.cell_size, opt.p.orient_thr_deg, opt.p.huber_px, opt.p.inlier_px,
                    opt.p.step_eps, opt.p.min_terms, opt.p.img_margin, opt.p.cameras, opt.p.block_threads);
        return 0;
    }
    const auto kfL = slurp<ebvo_edge>(argv[1]), kfR = slurp<ebvo_edge>(argv[2]), E0 = slurp<ebvo_edge>(argv[3]), E1 = slurp<ebvo_edge>(argv[4]);
    const auto pose = slurp<double>(argv[5]);
    if (pose.size() != 42)
        return 2;
    const int w = std::atoi(argv[6]), h = std::atoi(argv[7]);
    opt.p.rounds = std::atoi(argv[8]);
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
    const bool ok = tracker.align_Relative_Pose(kfL, kfR, E0, E1, w, h, opt, state, true);
    if (tracker.last_status != EBVO_OK)
        return 4;
    const ebvo_aligned_pose &a = state.aligned;
    std::printf("aligned %d status %d stop %d rounds %d steps %d assoc %d %d inliers %lld\n", ok ? 1 : 0, a.status, a.stop_reason,
                a.rounds_run, a.steps_kept, a.n_assoc[0], a.n_assoc[1], (long long)a.inliers);
    for (int i = 0; i < 12; ++i)
    {
        uint64_t bits;
        std::memcpy(&bits, i < 9 ? &a.R[i] : &a.t[i - 9], sizeof bits);
        std::printf("%016" PRIx64 "%c", bits, i == 11 ? '\n' : ' ');
    }
    FILE *f = std::fopen(argv[10], "wb");
    if (!f)
        return 5;
    std::fwrite(&a, sizeof a, 1, f);
    std::fwrite(state.assoc_left.data(), sizeof(int32_t), state.assoc_left.size(), f);
    std::fwrite(state.assoc_right.data(), sizeof(int32_t), state.assoc_right.size(), f);
    std::fclose(f);
    return 0;
}
