// include/orbslam2_amd.hpp's FrameBuilder compiles under -Wall -Werror and links; Build refuses a batch with kp_cap = 0
// before any device call (tests/test_frame_validation.py), so do the C entries on null arguments, and the CPU bounds of an
// undistorted camera are the image.
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

int use_frame_builder() {
    using namespace ORB_SLAM2_AMD;
    orbtf_frames fr{};   // kp_cap = 0
    orbtf_map m{};
    const float dist[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, camera[5] = {500.f, 500.f, 320.f, 240.f, 40.f};
    const FrameBuilder fb(fr, dist, 480, 640);
    int refused = 0;
    refused += refuses([&] { fb.Build(ORBFR_MONO, nullptr, nullptr); });
    refused += refuses([&] { fb.Build(ORBFR_RGBD, nullptr, nullptr, nullptr, ORBFR_DEPTH_U16, 0, 1280, 0.0002f); });
    if (orbfr_build_frames_device(nullptr, nullptr, nullptr) == ORB_EINVAL) refused++;
    if (orbfr_build_frames(nullptr, nullptr, 0) == ORB_EINVAL) refused++;
    refused += refuses([&] { FrameBuilder::ImageBounds(0, 640, camera, dist, nullptr); });
    float b[4] = {-1.f, -1.f, -1.f, -1.f};
    FrameBuilder::ImageBounds(480, 640, camera, dist, b);
    const TrackingFrames tf(fb.frames(), m);   // the builder's tables are the next step's
    return refused == 5 && b[0] == 0.f && b[1] == 640.f && b[2] == 0.f && b[3] == 480.f && tf.frames().kp_cap == 0 ? 0 : 2;
}
