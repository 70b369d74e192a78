// include/orbslam2_amd.hpp's KeyFrameDatabase compiles under -Wall -Werror and links; a null vocabulary is refused
// before any device call (tests/test_keyframe_db_validation.py), and so are the C entries on a null database.
#include "orbslam2_amd.hpp"

int use_keyframe_db() {
    using namespace ORB_SLAM2_AMD;
    int refused = 0;
    try {
        KeyFrameDatabase db(nullptr, 70, 200);
    } catch (const std::exception&) {
        refused++;
    }
    orbdb_query_batch b{};
    orbdb_result out{};
    if (orbdb_detect_reloc_device(nullptr, &b, &out, nullptr) == ORB_EINVAL) refused++;
    if (orbdb_detect_loop_device(nullptr, &b, &out, nullptr) == ORB_EINVAL) refused++;
    if (orbdb_min_score_device(nullptr, &b, nullptr, nullptr, nullptr, nullptr) == ORB_EINVAL) refused++;
    return refused == 4 ? 0 : 2;
}
