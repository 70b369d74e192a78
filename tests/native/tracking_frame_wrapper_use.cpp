// include/orbslam2_amd.hpp's TrackingFrames compiles under -Wall -Werror and links; every method refuses a batch with
// kp_cap = 0 before any device call (tests/test_tracking_frame_validation.py), and so do the C entries on null arguments.
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

int use_tracking_frames() {
    using namespace ORB_SLAM2_AMD;
    orbtf_frames fr{};   // kp_cap = 0
    orbtf_map m{};
    orbtf_edges edges{};
    orbtf_motion motion{};
    orbtf_created created{};
    orbba_pose_result result{};
    const TrackingFrames tf(fr, m);
    int refused = 0;
    refused += refuses([&] { tf.ApplyMatches(ORBTF_MERGE, nullptr, nullptr, 0, 1); });
    refused += refuses([&] { tf.PoseOptimization(nullptr, 8, edges, result, ORBTF_DISCARD, false, false, nullptr); });
    refused += refuses([&] { tf.MotionProject(fr, nullptr, nullptr, false, motion); });
    refused += refuses([&] { tf.EndFrame(8.f, nullptr, nullptr, nullptr, nullptr); });
    refused += refuses([&] { tf.DropOutliers(); });
    refused += refuses([&] { tf.StereoPoints(ORBTF_KEYFRAME, 8.f, created); });
    if (orbtf_drop_outliers_device(nullptr, nullptr) == ORB_EINVAL) refused++;
    if (orbtf_stereo_points(&fr, nullptr, ORBTF_INIT, 8.f, &created, 0) == ORB_EINVAL) refused++;
    return refused == 8 && tf.frames().kp_cap == 0 ? 0 : 2;
}
