// Compiles against include/orbslam2_amd.hpp alone (tests/test_pnpsolver_validation.py): the PnPsolver wrapper in the
// reference's shape, an empty batch and two refused parameter sets, none of which reaches a device.
#include <cstdio>
#include <exception>

#include "orbslam2_amd.hpp"

int use_pnpsolver_empty() {
    const float sigma2[1] = {1.f};
    ORB_SLAM2_AMD::PnPsolver solver(0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, sigma2, nullptr, 1);
    solver.SetRansacParameters(0.99, 10, 300, 4, 0.5f, 5.991f);
    orb_pnpsolver_result r{};
    solver.IterateBatch(5, r);   // an empty batch returns before any pointer is read
    int refused = 0;
    for (int which = 0; which < 2; which++) {
        ORB_SLAM2_AMD::PnPsolver bad(0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 1, sigma2, nullptr, 1);
        if (which == 0) bad.SetRansacParameters(0.99, 10, 300, 5, 0.5f, 5.991f);   // min_set != 4
        else bad.SetRansacParameters(0.99, 5, 300, 4, 0.5f, 5.991f);              // min_inliers < 6
        try {
            bad.IterateBatch(5, r);
        } catch (const std::exception& e) {
            std::printf("refused: %s\n", e.what());
            refused++;
        }
    }
    return refused == 2 ? 0 : 1;
}
