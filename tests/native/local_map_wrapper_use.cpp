// include/orbslam2_amd.hpp's LocalMap compiles under -Wall -Werror and links; an empty map or batch is refused before any
// device call (tests/test_local_map_validation.py), and so are the C entries on null arguments.
#include "orbslam2_amd.hpp"

int use_local_map() {
    using namespace ORB_SLAM2_AMD;
    int refused = 0;
    orbtl_map m{};
    orbtl_frames fr{};
    orbtl_result out{};
    LocalMap lm(m);
    try {
        lm.Update(fr, out);   // kf_cap = 0
    } catch (const std::exception&) {
        refused++;
    }
    try {
        orbm_proj_batch kp{};
        lm.TrackLocalMap(fr, out, kp, nullptr, nullptr);
    } catch (const std::exception&) {
        refused++;
    }
    if (orbtl_track_local_map_device(nullptr, &fr, &out, nullptr) == ORB_EINVAL) refused++;
    if (orbtl_track_local_map(&m, nullptr, &out, 0) == ORB_EINVAL) refused++;
    return refused == 4 ? 0 : 2;
}
