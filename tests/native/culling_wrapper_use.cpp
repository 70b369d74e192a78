// include/orbslam2_amd.hpp's Culling compiles under -Wall -Werror and links; empty tables are refused before any device
// call (tests/test_culling_validation.py), and so are the C entries on null arguments.
#include "orbslam2_amd.hpp"

int use_culling() {
    using namespace ORB_SLAM2_AMD;
    int refused = 0;
    orbmm_cull t{};
    Culling cull(t);
    int32_t n = 0;
    try {
        cull.MapPointCulling(nullptr, 0, 3, false, &n);   // kf_cap = 0
    } catch (const std::exception&) {
        refused++;
    }
    try {
        cull.KeyFrameCulling(0, false, 3.5f, &n, &n, &n);   // kf_cap = 0
    } catch (const std::exception&) {
        refused++;
    }
    try {
        cull.CompactObservations(nullptr, nullptr, nullptr);   // no arrays
    } catch (const std::exception&) {
        refused++;
    }
    try {
        cull.UpdateLiveChildren(nullptr, nullptr);
    } catch (const std::exception&) {
        refused++;
    }
    if (orbmm_cull_map_points(nullptr, 0, nullptr, 0, 0, nullptr, 0) == ORB_EINVAL) refused++;
    if (orbmm_cull_keyframes(nullptr, 0, 0, 0.f, nullptr, nullptr, nullptr, 0) == ORB_EINVAL) refused++;
    if (orbmm_compact_observations(-1, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0) == ORB_EINVAL) refused++;
    if (orbmm_children_live(-1, nullptr, nullptr, nullptr, nullptr, 0) == ORB_EINVAL) refused++;
    return refused == 8 ? 0 : 2;
}
