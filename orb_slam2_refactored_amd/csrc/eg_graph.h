// The edge list of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:798-903) from slot tables: host code, no
// device call.  orbba_essential_graph_edges (orbeg.hip) checks the tables and calls it.
#pragma once

#include <cstdint>
#include <set>
#include <utility>
#include <vector>

#include "orbslam2_amd.h"

namespace orbamd {

struct EgEdge { int32_t i, j; uint8_t table; };

// covisibility weight of (a, b): KeyFrame::GetWeight, 0 when b is not connected to a
inline int eg_weight(const orbba_eg_tables& g, int a, int b) {
    for (int p = g.covis_begin[a]; p < g.covis_begin[a + 1]; p++)
        if (g.covis_slot[p] == b) return g.covis_weight[p];
    return 0;
}

inline std::vector<EgEdge> eg_build_edges(const orbba_eg_tables& g, int min_weight) {
    std::vector<EgEdge> out;
    std::set<std::pair<int32_t, int32_t>> inserted;   // MakeMinMaxPair of the ids; slots stand for them
    auto mm = [](int a, int b) { return std::make_pair(a < b ? a : b, a < b ? b : a); };
    for (int c = 0; c < g.n_connections; c++) {   // :804-828
        const int k1 = g.conn_kf[c];
        for (int p = g.conn_begin[c]; p < g.conn_begin[c + 1]; p++) {
            const int k2 = g.conn_slot[p];
            if ((k1 != g.curr_slot || k2 != g.loop_kf_slot) && eg_weight(g, k1, k2) < min_weight) continue;
            out.push_back({k1, k2, 0});
            inserted.insert(mm(k1, k2));
        }
    }
    for (int k = 0; k < g.n_keyframes; k++) {   // :831-903
        const int par = g.parent[k];
        if (par >= 0) out.push_back({k, par, 1});
        const int lb = g.loop_begin[k], le = g.loop_begin[k + 1];
        for (int p = lb; p < le; p++) {
            const int l = g.loop_slot[p];
            if (l < 0 || g.kf_id[l] >= g.kf_id[k]) continue;
            out.push_back({k, l, 1});
        }
        for (int p = g.covis_begin[k]; p < g.covis_begin[k + 1]; p++) {
            const int n = g.covis_slot[p];
            if (g.covis_weight[p] < min_weight) continue;   // GetCovisiblesByWeight(minWeight)
            if (n < 0) continue;                            // isBad()
            bool is_loop = false;
            for (int q = lb; q < le; q++) is_loop = is_loop || g.loop_slot[q] == n;
            if (n == par || g.parent[n] == k || is_loop) continue;   // :882
            if (g.kf_id[n] >= g.kf_id[k]) continue;                  // :885
            if (inserted.count(mm(k, n))) continue;                  // :888
            out.push_back({k, n, 1});
        }
    }
    return out;
}

}  // namespace orbamd
