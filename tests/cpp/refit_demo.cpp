// refit_demo.cpp -- MotionTrackerHIP::refine_Relative_Pose (include/ebvo/adapters.hpp) after the search, on the temporal quads of
// a frame against itself moved by two pixels, as adapter_demo.cpp forms them; compiled with plain g++ against the C ABI alone.
// usage: refit_demo <left.raw> <right.raw> <h> <w> <out.bin>     (no arguments: prints the default options and ebvo::pose_error)
// out.bin: int64 n_final; ebvo_pose_result of the search; ebvo_pose_refined; n_final mask bytes of the refitted pose
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

static std::vector<unsigned char> slurp(const char *path, size_t n)
{
    std::vector<unsigned char> b(n);
    FILE *f = std::fopen(path, "rb");
    if (!f || std::fread(b.data(), 1, n, f) != n)
    {
        std::fprintf(stderr, "cannot read %s\n", path);
        std::exit(2);
    }
    std::fclose(f);
    return b;
}

int main(int argc, char **argv)
{
    ebvo::MotionTrackerHIP::Refine_Options ropt;
    if (argc != 6)
    {
        const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, Rz[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, a[3] = {0, 2, 0}, b[3] = {3, 0, 0};
        const ebvo::PoseError e = ebvo::pose_error(Rz, a, I, b);
        std::printf("rounds %d iterations %d huber_px %g step_eps %g block_threads %d\n", ropt.p.rounds, ropt.p.iterations,
                    ropt.p.huber_px, ropt.p.step_eps, ropt.p.block_threads);
        std::printf("pose_error %.17g %.17g %.17g\n", e.rot_deg, e.trans_abs, e.trans_dir_deg);
        return 0;
    }
    const int h = std::atoi(argv[3]), w = std::atoi(argv[4]);
    auto bl = slurp(argv[1], (size_t)h * w), br = slurp(argv[2], (size_t)h * w);
    auto ctx = std::make_shared<ebvo::Context>(h, w);
    if (ctx->status() != EBVO_OK)
        return 3;
    const double f = 718.856, t = 0.54;
    const double F[9] = {0, 0, 0, 0, 0, -t / f, 0, t / f, 0};
    ebvo_stereo_calib calib = {{f, 0, 607.1928, 0, f, 185.2157, 0, 0, 1}, {f, 0, 607.1928, 0, f, 185.2157, 0, 0, 1},
                               {1, 0, 0, 0, 1, 0, 0, 0, 1}, {t, 0, 0}};
    ebvo::StereoMatcherHIP<Edge> matcher(ctx);
    matcher.stereo_edge_pairs(bl.data(), br.data(), h, w, w, w, F, &calib, true);
    ebvo::TemporalMatcherHIP temporal(ctx);
    if (matcher.last_status != EBVO_OK || !temporal.set_keyframe(0))
        return 4;
    std::vector<unsigned char> l2(bl.size()), r2(br.size());
    for (int y = 0; y < h; ++y)
        for (int x = 0; x < w; ++x)
        {
            l2[(size_t)y * w + x] = bl[(size_t)y * w + (x + w - 2) % w];
            r2[(size_t)y * w + x] = br[(size_t)y * w + (x + w - 2) % w];
        }
    matcher.stereo_edge_pairs(l2.data(), r2.data(), h, w, w, w, F, &calib, true);
    auto tq = temporal.match(0, 1);
    if (matcher.last_status != EBVO_OK || temporal.last_status != EBVO_OK)
        return 5;
    ebvo::MotionTrackerHIP tracker(ctx, calib);
    ebvo::MotionTrackerHIP::Ransac_Options opt;
    ebvo::MotionTrackerHIP::Ransac_State state;
    if (!tracker.estimate_Relative_Pose_From_Quad_Pairs(0, opt, state))
        return 6;
    const bool refined = tracker.refine_Relative_Pose(0, opt, ropt, state, false, true);
    if (tracker.last_status != EBVO_OK || refined != (state.refined.status == 0))
        return 7;
    const int64_t n = (int64_t)state.inliers.size();
    FILE *o = std::fopen(argv[5], "wb");
    if (!o)
        return 8;
    std::fwrite(&n, sizeof n, 1, o);
    std::fwrite(&state.pose, sizeof state.pose, 1, o);
    std::fwrite(&state.refined, sizeof state.refined, 1, o);
    std::fwrite(state.inliers.data(), 1, state.inliers.size(), o);
    std::fclose(o);
    std::printf("refit_demo ok: %lld quads, status %d stop %d\n", (long long)n, state.refined.status, state.refined.stop_reason);
    return 0;
}
