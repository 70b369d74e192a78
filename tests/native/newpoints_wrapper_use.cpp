// include/orbslam2_amd.hpp's CreateNewMapPoints compiles under -Wall -Werror and links; an empty plan returns and a
// round that names a keyframe twice, or as keyframe 1 and as keyframe 2 of one slot set, is refused before any
// device call (tests/test_newpoints_validation.py).
#include "orbslam2_amd.hpp"

int use_new_points() {
    using namespace ORB_SLAM2_AMD;
    int refused = 0;
    const int32_t f1[4] = {0, 1, 0, 0}, f2[4] = {2, 3, 4, 4}, g2[4] = {2, 0, 4, 5};
    try {
        CreateNewMapPoints::CheckPlan(1, 2, f1, f2, true);   // round 0 alone is fine
        CreateNewMapPoints::CheckPlan(0, 0, nullptr, nullptr, true);
    } catch (const std::exception&) {
        return 1;
    }
    try {
        CreateNewMapPoints::CheckPlan(2, 2, f1, f2, true);
    } catch (const std::exception&) {
        refused++;
    }
    try {
        CreateNewMapPoints::CheckPlan(1, 2, f1, g2, true);
    } catch (const std::exception&) {
        refused++;
    }
    orblm_batch b{};
    orbm_tri_batch s{};
    orblm_pairs pairs{};
    orblm_points out{};
    CreateNewMapPoints lm(b, s);
    try {
        lm.Run(1, 2, f1, f2, nullptr, nullptr, pairs, out, nullptr, nullptr);   // null arrays: ORB_EINVAL, thrown
    } catch (const std::exception&) {
        refused++;
    }
    return refused == 3 ? 0 : 2;
}
