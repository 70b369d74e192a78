// Compile-only check that the BundleAdjustment / GlobalBAUpdateMap wrappers build against the C-ABI header.
#include "orbslam2_amd.hpp"

bool use_bundle_adjustment(const orbba_problem& pr, orbba_gba_result& res, const volatile int32_t* stop) {
    return ORB_SLAM2_AMD::BundleAdjustment(pr, res) && ORB_SLAM2_AMD::BundleAdjustment(pr, res, 10, stop, false);
}

void use_update_map(const orbba_gba_map& m, void* stream) {
    ORB_SLAM2_AMD::GlobalBAUpdateMap(m);
    ORB_SLAM2_AMD::GlobalBAUpdateMapDevice(m, stream);
}
