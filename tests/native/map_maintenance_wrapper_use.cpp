// include/orbslam2_amd.hpp's MapMaintenance compiles under -Wall -Werror and links; empty tables are refused before any
// device call (tests/test_map_maintenance_validation.py), and so are the C entries on null arguments.
#include "orbslam2_amd.hpp"

int use_map_maintenance() {
    using namespace ORB_SLAM2_AMD;
    int refused = 0;
    orbmm_points p{};
    orbmm_graph g{};
    orbmm_csr c{};
    MapMaintenance mm(g);
    try {
        mm.UpdateNormalAndDepth(p);   // kf_cap = 0
    } catch (const std::exception&) {
        refused++;
    }
    try {
        mm.UpdateConnections(nullptr, 1);   // conn_cap = 0
    } catch (const std::exception&) {
        refused++;
    }
    try {
        mm.PackCovisibility(c);
    } catch (const std::exception&) {
        refused++;
    }
    try {
        mm.UpdateChildren(nullptr, nullptr);   // no graph arrays
    } catch (const std::exception&) {
        refused++;
    }
    if (orbmm_update_normal_depth(nullptr, 0) == ORB_EINVAL) refused++;
    if (orbmm_update_connections_device(nullptr, 0, nullptr, nullptr) == ORB_EINVAL) refused++;
    if (orbmm_children(-1, nullptr, nullptr, nullptr, 0) == ORB_EINVAL) refused++;
    if (orbmm_covis_csr(&g, nullptr, 0) == ORB_EINVAL) refused++;
    return refused == 8 ? 0 : 2;
}
