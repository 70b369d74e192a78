// Compile-only check that the SearchBySim3 / ComputeDistinctiveDescriptors wrappers build against the C-ABI header.
#include "orbslam2_amd.hpp"

int use_sim3(const orbm_sim3_batch& b) {
    std::vector<int32_t> match12;
    return ORB_SLAM2_AMD::SearchBySim3(b, match12);
}

int use_distinct(const std::vector<uint8_t>& rows, uint8_t* descriptor) {
    return ORB_SLAM2_AMD::ComputeDistinctiveDescriptors(rows, descriptor);
}

void use_sim3_batch(const orbm_sim3_batch& b, int32_t* d_match12, int32_t* d_match1, int32_t* d_match2, int32_t* d_n_found,
                    const uint8_t* d_desc, const int32_t* d_begin, int32_t n_points, int32_t* d_best, int32_t* d_median,
                    uint8_t* d_out_desc, void* stream) {
    ORB_SLAM2_AMD::SearchBySim3Batch(b, d_match12, d_match1, d_match2, d_n_found, stream);
    ORB_SLAM2_AMD::ComputeDistinctiveDescriptorsBatch(d_desc, d_begin, n_points, d_best, d_median, d_out_desc, stream);
}

// the host entries return before touching the device on an empty batch, and refuse a point over the limit
int use_sim3_empty() {
    orbm_sim3_batch b = {};
    const float sf[1] = {1.f};
    b.n_levels = 1;
    b.scale_factors = sf;
    int32_t nf = 0;
    const int32_t begin[2] = {0, ORBM_DISTINCT_MAX_OBS + 1};
    int32_t best = 0;
    const int refused = orbm_distinctive_descriptors(nullptr, begin, 1, &best, nullptr, nullptr, 0) == ORB_EINVAL ? 0 : 1;
    return orbm_search_by_sim3(&b, nullptr, nullptr, nullptr, &nf, 0) +
           orbm_distinctive_descriptors(nullptr, nullptr, 0, nullptr, nullptr, nullptr, 0) + refused;
}
