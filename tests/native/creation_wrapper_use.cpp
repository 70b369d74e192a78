// include/orbslam2_amd.hpp's MapBuilder compiles under -Wall -Werror and links; empty tables are refused before any device
// call (tests/test_creation_validation.py), as the C entries refuse null arguments.
#include "orbslam2_amd.hpp"

template <class Fn>
static int refuses(Fn call) {
    try {
        call();
    } catch (const std::exception&) {
        return 1;
    }
    return 0;
}

int use_map_builder() {
    using namespace ORB_SLAM2_AMD;
    orbmk_keyframes kf{};   // kf_cap = 0
    orbmk_map map{};
    orbmk_frames fr{};
    orbtf_frames tf{};
    orbtf_created tc{};
    orblm_points lp{};
    orbmk_created out{};
    const MapBuilder mb(kf, map);
    int refused = 0;
    refused += refuses([&] { mb.InsertKeyFrames(fr, 1, nullptr, nullptr, nullptr, nullptr); });
    refused += refuses([&] { mb.CreatePoints(orbmk_lists{}, out); });
    refused += refuses([&] { mb.CreatePoints(tf, tc, nullptr, nullptr, out); });
    refused += refuses([&] { mb.CreatePoints(lp, 2, 100, nullptr, nullptr, out); });
    if (orbmk_insert_keyframes_device(nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, nullptr) == ORB_EINVAL) refused++;
    if (orbmk_create_points(nullptr, nullptr, nullptr, 0) == ORB_EINVAL) refused++;
    return refused == 6 && mb.map().kf_cap == 0 && mb.keyframes().conn_cap == 0 && ORBMK_OVERFLOW == 1 ? 0 : 2;
}
