// Compile-only check that the OptimizeEssentialGraph wrappers build against the C-ABI header.
#include "orbslam2_amd.hpp"

int use_essential_graph(const orbba_essential_graph& g, std::vector<float>& pose, std::vector<float>& points) {
    return ORB_SLAM2_AMD::Optimizer::OptimizeEssentialGraph(g, pose, points);
}

void use_essential_graph_device(const orbba_essential_graph& g, orbba_essential_graph_result& r, void* stream) {
    ORB_SLAM2_AMD::Optimizer::OptimizeEssentialGraphDevice(g, r, stream);
}

void use_edges(const orbba_eg_tables& t, std::vector<int32_t>& ei, std::vector<int32_t>& ej, std::vector<uint8_t>& et) {
    ORB_SLAM2_AMD::Optimizer::EssentialGraphEdges(t, ei, ej, et);
}

// the entries refuse before touching the device
int use_essential_graph_refusals() {
    orbba_essential_graph g = {};
    orbba_essential_graph_result r = {};
    g.n_keyframes = ORBBA_EG_MAX_KEYFRAMES + 1;
    return (orbba_optimize_essential_graph(&g, &r, 0) == ORB_EINVAL ? 0 : 1) +
           (orbba_optimize_essential_graph_device(&g, &r, nullptr) == ORB_EINVAL ? 0 : 1);
}
