// include/orbslam2_amd.hpp's Initializer compiles under -Wall -Werror and links; an empty batch returns and
// max_iterations = 0 / sigma = 0 are refused before any device call (tests/test_initializer_validation.py).
#include "orbslam2_amd.hpp"

int use_initializer_empty() {
    using namespace ORB_SLAM2_AMD;
    const int32_t begin[1] = {0};
    Initializer ini(0, 0, begin, nullptr, nullptr, 1.0f, 200);
    orb_initializer_result r{};
    try {
        ini.InitializeBatch(0, begin, nullptr, nullptr, nullptr, r);   // n_pairs = 0: returns
    } catch (const std::exception&) {
        return 1;
    }
    int refused = 0;
    try {
        Initializer bad(0, 0, begin, nullptr, nullptr, 1.0f, 0);
        bad.InitializeBatch(0, begin, nullptr, nullptr, nullptr, r);
    } catch (const std::exception&) {
        refused++;
    }
    try {
        Initializer bad(0, 0, begin, nullptr, nullptr, 0.0f, 200);
        bad.InitializeBatch(0, begin, nullptr, nullptr, nullptr, r);
    } catch (const std::exception&) {
        refused++;
    }
    return refused == 2 ? 0 : 2;
}
