// MotionTrackerHIP (include/ebvo/adapters.hpp) driven as Pipeline::get_Pose_From_Quad_Pairs drives MotionTracker
// (src/Pipeline.cpp:192-223): compiled with plain g++ against the C ABI alone.  Without a device it reports the context
// error and exits 0 after printing the default options.
#include <cstdio>
#include <memory>

#include "ebvo/adapters.hpp"

int main()
{
    ebvo::MotionTrackerHIP::Ransac_Options opt;
    std::printf("max_iterations %d min_iterations %d success_prob %g top_rank_fraction %g\n", opt.p.max_iterations,
                opt.p.min_iterations, opt.p.success_prob, opt.p.top_rank_fraction);
    auto ctx = std::make_shared<ebvo::Context>(64, 64);
    if (ctx->status() != EBVO_OK)
        return 0;
    ebvo_stereo_calib calib{};
    calib.K_left[0] = calib.K_left[4] = 500.0;
    calib.K_left[2] = 32.0;
    calib.K_left[5] = 32.0;
    calib.K_left[8] = 1.0;
    calib.R21[0] = calib.R21[4] = calib.R21[8] = 1.0;
    calib.T21[0] = -0.1;
    ebvo::MotionTrackerHIP tracker(ctx, calib);
    ebvo::MotionTrackerHIP::Ransac_State state;
    // no temporal quads in slot 0 yet: the call is refused (EBVO_ERR_STATE) and reports false
    const bool ok = tracker.estimate_Relative_Pose_From_Quad_Pairs(0, opt, state, true);
    std::printf("estimate: %d status %d\n", (int)ok, tracker.last_status);
    return ok ? 1 : 0;
}
