// Compile-only check that the Sim3Solver wrappers build against the C-ABI header.
#include "orbslam2_amd.hpp"

bool use_sim3solver(const orb_sim3solver_batch& b, float* s12) {
    int32_t iterations = 0, max_inliers = 0;
    std::vector<uint8_t> inlier;
    std::vector<int32_t> match12;
    bool terminate = false;
    return ORB_SLAM2_AMD::Sim3Solver::Iterate(b, iterations, max_inliers, s12, inlier, match12, terminate);
}

void use_sim3solver_batch(const orb_sim3solver_batch& b, orb_sim3solver_result& r, void* stream) {
    ORB_SLAM2_AMD::Sim3Solver::IterateBatch(b, r, stream);
}

// the host entry returns before touching the device on an empty batch, and refuses min_inliers < 3
int use_sim3solver_empty() {
    orb_sim3solver_batch b = {};
    const float sigma2[1] = {1.f};
    b.n_levels = 1;
    b.level_sigma2 = sigma2;
    b.rand_max = 2147483647;
    b.probability = 0.99;
    b.min_inliers = 20;
    b.max_iterations = 300;
    b.maxk = 5;
    orb_sim3solver_result r = {};
    const int ok = orb_sim3solver_iterate(&b, &r, 0);
    b.min_inliers = 2;
    const int refused = orb_sim3solver_iterate(&b, &r, 0) == ORB_EINVAL ? 0 : 1;
    return ok + refused;
}
