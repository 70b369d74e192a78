// include/orbslam2_amd.hpp's LocalBA compiles under -Wall -Werror and links; empty tables are refused before any device
// call (tests/test_local_ba_map_validation.py), and so are the C entries on null arguments.
#include "orbslam2_amd.hpp"

int use_local_ba() {
    using namespace ORB_SLAM2_AMD;
    int refused = 0;
    orbba_window_map m{};
    orbba_window w{};
    orbba_map_result r{};
    LocalBA ba(m);
    auto expect = [&](auto&& call) {
        try {
            call();
        } catch (const std::exception&) {
            refused++;
        }
    };
    expect([&] { ba.Window(0, w); });   // kf_cap = 0
    expect([&] { ba.Apply(w, nullptr, nullptr, nullptr, nullptr); });
    expect([&] { ba.Run(0, w, r); });
    expect([&] { ba.WindowHost(0, w); });
    expect([&] { ba.ApplyHost(w, nullptr, nullptr, nullptr, nullptr); });
    expect([&] { ba.RunHost(0, r); });
    if (orbba_local_window(nullptr, 0, nullptr, 0) == ORB_EINVAL) refused++;
    if (orbba_local_ba_apply_device(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == ORB_EINVAL) refused++;
    if (orbba_local_ba_map(nullptr, 0, nullptr, nullptr, 0) == ORB_EINVAL) refused++;
    return refused == 9 ? 0 : 2;
}
