// Compile-only check that the Fuse / Sim3 SearchByProjection wrappers build against the C-ABI header.
#include "orbslam2_amd.hpp"

int use_fuse(const orbm_fuse_batch& b) {
    std::vector<int32_t> bestIdx, bestDist;
    return ORB_SLAM2_AMD::Fuse(b, bestIdx, bestDist);
}

void use_fuse_batch(const orbm_fuse_batch& b, int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_n_fused,
                    const uint8_t* d_claimed, int32_t* d_kp_match, int32_t* d_n_matches, void* stream) {
    ORB_SLAM2_AMD::FuseBatch(b, d_best_idx, d_best_dist, d_n_fused, stream);
    ORB_SLAM2_AMD::SearchByProjectionSim3Batch(b, d_claimed, d_kp_match, d_n_matches, stream);
}

// the host entry refuses a batch before touching the device: an empty batch is a no-op
int use_fuse_empty() {
    orbm_fuse_batch b = {};
    const float sf[1] = {1.f};
    b.n_levels = 1;
    b.scale_factors = sf;
    int32_t nf = 0;
    return orbm_fuse(&b, nullptr, nullptr, &nf, 0) + orbm_search_by_projection_sim3(&b, nullptr, nullptr, &nf, 0);
}
