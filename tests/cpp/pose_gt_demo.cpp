// MotionTrackerHIP under ground truth (include/ebvo/adapters.hpp): the GT-row search, Solution_Constraints_Application and
// Print_Quad_Pairs_Metrics_Statistics as src/Pipeline.cpp:198-203 drives them, compiled with plain g++ against the C ABI
// alone.  Without a device it prints the statistics of two hand-made runs and exits 0.
#include <iostream>
#include <memory>

#include "ebvo/adapters.hpp"

int main()
{
    using Tracker = ebvo::MotionTrackerHIP;
    std::vector<std::vector<Tracker::Quad_Pair_Evaluation_Metrics>> runs = {
        {{"Baseline", 1.0, 0.5, 10}, {"Normalized Length Constraint", 0.9, 0.75, 9}},
        {{"Baseline", 1.0, 0.25, 6}, {"Normalized Length Constraint", 0.5, 0.5, 3}},
    };
    Tracker::Print_Quad_Pairs_Metrics_Statistics(runs, std::cout);
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
    Tracker tracker(ctx, calib);
    Tracker::Ransac_Options opt;
    Tracker::Ransac_State state;
    // slot 0 is not armed: both calls are refused (EBVO_ERR_STATE)
    const bool ok = tracker.estimate_Relative_Pose_From_Quad_Pairs(0, opt, state, true, true);
    const auto all = tracker.Solution_Constraints_Application(0, opt, 20);
    Tracker::Print_Quad_Pairs_Metrics_Statistics(all, std::cout);
    std::cout << "estimate: " << ok << " runs " << all.size() << " status " << tracker.last_status << std::endl;
    return ok || !all.empty() ? 1 : 0;
}
