// include/orbslam2_amd.hpp's LoopCorrection compiles under -Wall -Werror and links; empty tables are refused before any
// device call (tests/test_loop_correct_validation.py).
#include "orbslam2_amd.hpp"

int use_loop_correction() {
    using namespace ORB_SLAM2_AMD;
    int refused = 0;
    orblc_map m{};
    LoopCorrection lc(m);
    int32_t n = 0;
    float f = 0;
    uint8_t b = 0;
    try {
        lc.Connected(0, &n, &n);   // conn_cap = 0
    } catch (const std::exception&) {
        refused++;
    }
    try {
        lc.Propagate(0, &f, &n, 0, &f, &f, &n, &n);
    } catch (const std::exception&) {
        refused++;
    }
    try {
        lc.LoopConnections(&n, 0, &n, &n, &n, &n);
    } catch (const std::exception&) {
        refused++;
    }
    try {
        orbba_eg_tables t{};
        LoopCorrection::EssentialGraphEdges(t, 0, 0, 0, 100, 0, &n, &n, &b, &n);   // n_keyframes = 0
    } catch (const std::exception&) {
        refused++;
    }
    return refused;
}
