// orblc.hip — LoopCorrector::Correct on gfx950 (include/orbslam2_amd.h, "LoopCorrector::Correct"): the connected list, the
// propagation of Scw with the correction of the neighbours' map points and poses, the LoopConnections sets, and the edge
// list of OptimizeEssentialGraph, in place on the tables of orbmm_points / orbmm_graph.
//
// Reference: src/LoopClosing.cc:546-676, src/Optimizer.cc:798-903.  The arithmetic and the rules are csrc/lc_propagate.h's.
// Passes, stream-ordered, nothing read back:
//   lc_connected_kernel   one wavefront: the stable compaction of cur's ordered row, then cur, then -1
//   lc_keyframe_kernel    one lane per keyframe: both Sim3 rows, the entry centre, for a connected keyframe (a scan of
//                         the list) the corrected pose and its centre; the claim array reset; the list sorted (rank sort)
//   lc_claim_kernel       one lane per entry of a connected keyframe's row: atomicMin of the slot on the point's claim
//   lc_point_kernel       one lane per point: the correction, UpdateNormalAndDepth with the centre selected per
//                         observer, point_ref; one lane per keyframe: SetPose
//   lc_snapshot_kernel, orbmm_update_connections_device with one item, lc_difference_kernel per connected keyframe;
//   lc_pack_kernel        one workgroup: rank sort by slot, scan, fill
//   eg_loop_edges_kernel  one workgroup: the loop connections in order, a scan per row; the kept pairs stay in the workspace
//   eg_count_kernel / eg_scan_kernel / eg_fill_kernel   per keyframe: count, scan, fill and the (-1, -1, 0) padding
// The workspace of this unit is its own (g_lc): orbmm_update_connections_device runs between its kernels on g_mm's.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"
#include "lc_propagate.h"
#include "mm_groups.h"
#include "mm_host.h"

namespace orbamd {

inline thread_local Scratch g_lc;

__global__ __launch_bounds__(64) void lc_connected_kernel(int K, int cap, const int32_t* ord_slot, const int32_t* n_ord, int cur,
                                                          int32_t* connected, int32_t* n_connected) {
    const MmWave g{(int)threadIdx.x};
    const int n = lc_clamp(n_ord[cur], 0, cap);
    const int32_t* row = ord_slot + (size_t)cur * cap;
    int at = 0;
    for (int base = 0; base < n; base += 64) {   // uniform trip count
        const int i = base + g.lane;
        const int s = i < n ? row[i] : -1;
        const bool keep = s >= 0 && s < K;
        int total;
        const int off = g.prefix(keep, total);
        if (keep) connected[at + off] = s;   // at + off <= i <= cap - 1
        at += total;
    }
    for (int i = at + g.lane; i <= cap; i += 64) connected[i] = i == at ? cur : -1;
    if (g.lane == 0) *n_connected = at + 1;
}

// The key of list entry j in the ascending order: its slot, or past every slot when it is skipped
__device__ int lc_key(const int32_t* connected, int j, int K) {
    const int k = connected[j];
    return (k >= 0 && k < K) ? k : INT_MAX;
}

__device__ int lc_rank(const int32_t* connected, int n, int j, int K) {
    const int key = lc_key(connected, j, K);
    int r = 0;
    for (int i = 0; i < n; i++) {
        const int ki = lc_key(connected, i, K);
        r += (ki < key || (ki == key && i < j)) ? 1 : 0;
    }
    return r;
}

__global__ __launch_bounds__(256) void lc_keyframe_kernel(LcMap t, LcWork w, int cur, const float* scw, const int32_t* connected,
                                                          int max_connected, float* vertex_sim3, float* edge_sim3, int32_t* items) {
    const int g = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    for (int k = g; k < t.pts.K; k += stride) lc_keyframe(t, w, k, cur, scw, connected, max_connected, vertex_sim3, edge_sim3);
    for (int p = g; p < t.pts.M; p += stride) w.claim[p] = LC_UNCLAIMED;
    if (items)
        for (int j = g; j < max_connected; j += stride) {
            const int key = lc_key(connected, j, t.pts.K);
            items[lc_rank(connected, max_connected, j, t.pts.K)] = key == INT_MAX ? -1 : key;
        }
}

__global__ __launch_bounds__(256) void lc_claim_kernel(LcMap t, LcWork w, int cur, const int32_t* connected) {
    const int k = connected[blockIdx.x];
    if (k < 0 || k >= t.pts.K) return;
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (i >= t.pts.kf_cap) return;
    const int p = lc_claimed_point(t, k, i, t.kf_id[cur]);
    if (p >= 0) atomicMin(&w.claim[p], k);
}

__global__ __launch_bounds__(256) void lc_point_kernel(LcMap t, LcWork w, int cur, const float* vertex_sim3, const float* edge_sim3,
                                                       int32_t* point_ref) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g < t.pts.M) lc_point(t, w, g, t.kf_id[cur], vertex_sim3, edge_sim3, point_ref);
    if (g < t.pts.K && w.is_conn[g])   // SetPose: no lane of this launch reads kf_pose
        for (int i = 0; i < 12; i++) t.kf_pose[12 * (size_t)g + i] = w.new_pose[12 * (size_t)g + i];
}

// ---------------------------------------------------------------------------------------------- LoopConnections
struct LcSets {
    int32_t* set;      // [max_connected][cap]
    int32_t* count;    // [max_connected]
    int32_t* sorted;   // [max_connected + 1] the counts in output order
    int32_t* prev;     // [cap]
    int32_t* n_prev;   // [1]
    int32_t* status;   // [K] of one update
};

__global__ __launch_bounds__(256) void lc_snapshot_kernel(int K, int cap, const int32_t* ord_slot, const int32_t* n_ord,
                                                          const int32_t* connected, int j, LcSets s) {
    const int k = connected[j];
    const bool live = k >= 0 && k < K;
    const int n = live ? lc_clamp(n_ord[k], 0, cap) : 0;
    for (int i = threadIdx.x; i < n; i += 256) s.prev[i] = ord_slot[(size_t)k * cap + i];
    if (threadIdx.x == 0) *s.n_prev = n;
}

__global__ __launch_bounds__(64) void lc_difference_kernel(int K, int cap, const int32_t* conn_slot, const int32_t* n_conn,
                                                           const int32_t* connected, int max_connected, int j, LcSets s,
                                                           int32_t* status) {
    const MmWave g{(int)threadIdx.x};
    const int k = connected[j];
    int at = 0;
    if (k >= 0 && k < K) {
        const int n = lc_clamp(n_conn[k], 0, cap), n_prev = *s.n_prev;
        for (int base = 0; base < n; base += 64) {   // uniform trip count
            const int i = base + g.lane;
            const int slot = i < n ? conn_slot[(size_t)k * cap + i] : -1;
            const bool keep = i < n && lc_new_link(slot, K, s.prev, n_prev, connected, max_connected);
            int total;
            const int off = g.prefix(keep, total);
            if (keep) s.set[(size_t)j * cap + at + off] = slot;
            at += total;
        }
    }
    if (g.lane == 0) s.count[j] = at;
    for (int i = g.lane; i < K; i += 64)
        if (s.status[i] != ORBMM_OK) status[i] = s.status[i];
}

__global__ __launch_bounds__(256) void lc_pack_kernel(int K, int cap, const int32_t* connected, int max_connected, LcSets s,
                                                      int32_t* conn_kf, int32_t* conn_begin, int32_t* conn_slot,
                                                      int32_t* n_connections) {
    for (int j = threadIdx.x; j < max_connected; j += 256) {
        const int key = lc_key(connected, j, K);
        const int r = lc_rank(connected, max_connected, j, K);
        conn_kf[r] = key == INT_MAX ? -1 : key;
        s.sorted[r] = s.count[j];
    }
    __syncthreads();
    mm_block_scan<int32_t>(s.sorted, max_connected, conn_begin, 0, cap, 0);
    __syncthreads();
    for (int j = threadIdx.x; j < max_connected; j += 256) {
        const int r = lc_rank(connected, max_connected, j, K), b = conn_begin[r], n = lc_clamp(s.count[j], 0, cap);
        for (int i = 0; i < n; i++) conn_slot[b + i] = s.set[(size_t)j * cap + i];
    }
    if (threadIdx.x == 0) {
        int live = 0;
        for (int j = 0; j < max_connected; j++) live += lc_key(connected, j, K) != INT_MAX ? 1 : 0;
        *n_connections = live;
    }
}

// ---------------------------------------------------------------------------------------------- the edge list
struct EgDev {
    orbba_eg_tables g;
    int n_loop, n_covis, n_conn;   // entries of loop_slot, covis_slot / covis_weight, conn_slot
};

__device__ void eg_row(const int32_t* begin, int r, int limit, int& b0, int& b1) {
    b0 = lc_clamp(begin[r], 0, limit);
    b1 = lc_clamp(begin[r + 1], b0, limit);
}

// KeyFrame::GetWeight
__device__ int eg_weight_dev(const EgDev& d, int a, int b) {
    int b0, b1;
    eg_row(d.g.covis_begin, a, d.n_covis, b0, b1);
    for (int p = b0; p < b1; p++)
        if (d.g.covis_slot[p] == b) return d.g.covis_weight[p];
    return 0;
}

// Optimizer.cc:804-828.  pair: the kept (min, max) pairs, 2 * n_conn entries
__global__ __launch_bounds__(64 * MM_CULL_WAVES) void eg_loop_edges_kernel(EgDev d, int min_weight, int capacity, int32_t* edge_i,
                                                                            int32_t* edge_j, uint8_t* edge_table, int32_t* pair,
                                                                            int32_t* n_kept) {
    __shared__ int32_t s_red[MM_CULL_WAVES];
    const MmBlock b{(int)threadIdx.x, s_red};
    const int V = d.g.n_keyframes;
    int at = 0;
    for (int c = 0; c < d.g.n_connections; c++) {   // uniform
        const int k1 = d.g.conn_kf[c];
        if (k1 < 0 || k1 >= V) continue;
        int b0, b1;
        eg_row(d.g.conn_begin, c, d.n_conn, b0, b1);
        for (int base = b0; base < b1; base += b.width) {
            const int p = base + b.lane;
            const int k2 = p < b1 ? d.g.conn_slot[p] : -1;
            const bool keep = k2 >= 0 && k2 < V &&
                              ((k1 == d.g.curr_slot && k2 == d.g.loop_kf_slot) || eg_weight_dev(d, k1, k2) >= min_weight);
            int total;
            const int e = at + b.prefix(keep, total);
            if (keep) {
                if (e < d.n_conn) {   // rows that overlap could list more pairs than conn_slot has entries
                    pair[2 * (size_t)e] = ::min(k1, k2);
                    pair[2 * (size_t)e + 1] = ::max(k1, k2);
                }
                if (e < capacity) {
                    edge_i[e] = k1;
                    edge_j[e] = k2;
                    edge_table[e] = 0;
                }
            }
            at += total;
        }
    }
    if (b.lane == 0) *n_kept = at;
}

// Optimizer.cc:831-903 for keyframe k: emit(j) for every edge (k, j) in insertion order
template <class Emit>
__device__ void eg_keyframe_edges(const EgDev& d, int k, int min_weight, const int32_t* pair, int n_kept, Emit emit) {
    const int V = d.g.n_keyframes, par = d.g.parent[k], id = d.g.kf_id[k];
    n_kept = ::min(n_kept, d.n_conn);
    if (par >= 0 && par < V) emit(par);
    int lb, le, cb, ce;
    eg_row(d.g.loop_begin, k, d.n_loop, lb, le);
    eg_row(d.g.covis_begin, k, d.n_covis, cb, ce);
    for (int p = lb; p < le; p++) {
        const int l = d.g.loop_slot[p];
        if (l < 0 || l >= V || d.g.kf_id[l] >= id) continue;
        emit(l);
    }
    for (int p = cb; p < ce; p++) {
        const int n = d.g.covis_slot[p];
        if (d.g.covis_weight[p] < min_weight || n < 0 || n >= V) continue;
        bool is_loop = false;
        for (int q = lb; q < le; q++) is_loop = is_loop || d.g.loop_slot[q] == n;
        if (n == par || d.g.parent[n] == k || is_loop) continue;
        if (d.g.kf_id[n] >= id) continue;
        const int lo = ::min(k, n), hi = ::max(k, n);
        bool inserted = false;
        for (int q = 0; q < n_kept; q++) inserted = inserted || (pair[2 * (size_t)q] == lo && pair[2 * (size_t)q + 1] == hi);
        if (inserted) continue;
        emit(n);
    }
}

__global__ __launch_bounds__(256) void eg_count_kernel(EgDev d, int min_weight, const int32_t* pair, const int32_t* n_kept,
                                                       int32_t* count) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= d.g.n_keyframes) return;
    int c = 0;
    eg_keyframe_edges(d, k, min_weight, pair, *n_kept, [&](int) { c++; });
    count[k] = c;
}

__global__ __launch_bounds__(256) void eg_scan_kernel(int V, int32_t* count, const int32_t* n_kept, int32_t* n_edges) {
    const int32_t total = mm_block_scan<int32_t>(count, V, count, 0, INT_MAX, 0);
    if (threadIdx.x == 0) *n_edges = *n_kept + total;
}

__global__ __launch_bounds__(256) void eg_fill_kernel(EgDev d, int min_weight, const int32_t* pair, const int32_t* n_kept,
                                                      const int32_t* off, int capacity, int32_t* edge_i, int32_t* edge_j,
                                                      uint8_t* edge_table) {
    const int g = blockIdx.x * 256 + threadIdx.x, V = d.g.n_keyframes;
    if (g < V) {
        int e = *n_kept + off[g];
        eg_keyframe_edges(d, g, min_weight, pair, *n_kept, [&](int j) {
            if (e < capacity) {
                edge_i[e] = g;
                edge_j[e] = j;
                edge_table[e] = 1;
            }
            e++;
        });
    }
    const long long pad = (long long)*n_kept + off[V] + g;   // past the list
    if (pad < capacity) {
        edge_i[pad] = -1;
        edge_j[pad] = -1;
        edge_table[pad] = 0;
    }
}

}  // namespace orbamd

using namespace orbamd;

namespace {

enum LcUse { LC_ROWS = 1, LC_GRAPH = 2, LC_POINTS = 4 };

orbmm_points lc_points(const orblc_map& m) {
    orbmm_points p{};
    p.n_keyframes = m.n_keyframes; p.n_mappoints = m.n_mappoints; p.kf_cap = m.kf_cap; p.n_obs = m.n_obs; p.n_levels = m.n_levels;
    p.scale_factors = m.scale_factors; p.mp_bad = m.mp_bad; p.mp_xw = m.mp_xw; p.mp_ref_kf = m.mp_ref_kf;
    p.mp_obs_off = m.mp_obs_off; p.mp_obs_kf = m.mp_obs_kf; p.mp_obs_idx = m.mp_obs_idx; p.kf_pose = m.kf_pose; p.kf_n = m.kf_n;
    p.kf_kp_octave = m.kf_kp_octave; p.mp_normal = m.mp_normal; p.mp_max_min = m.mp_max_min;
    return p;
}

// What both forms of an entry check: the tables the entry uses
int lc_check(const orblc_map* m, int use) {
    ORB_CHECK_ARG(m, "null map");
    int rc;
    if (use & (LC_ROWS | LC_GRAPH)) {
        const orbmm_graph g = orblc_graph(m);
        if ((rc = mm_graph_check(&g, !(use & LC_GRAPH)))) return rc;
    }
    if (use & LC_POINTS) {
        ORB_CHECK_ARG(m->conn_cap >= 1, "conn_cap must be at least 1");
        const orbmm_points p = lc_points(*m);
        if ((rc = mm_points_check(&p))) return rc;
        ORB_CHECK_ARG(m->kf_id && m->kf_mappoint, "null keyframe table");
        ORB_CHECK_ARG(m->mp_corrected_by && m->mp_corrected_ref, "null map-point table");
    }
    return ORB_OK;
}

int lc_list_check(const orblc_map* m, const int32_t* connected, int32_t max_connected) {
    ORB_CHECK_ARG(max_connected >= 0 && max_connected <= m->conn_cap + 1, "max_connected outside [0, conn_cap + 1]");
    ORB_CHECK_ARG(connected, "null connected");
    return ORB_OK;
}

int lc_cur_check(const orblc_map* m, int32_t cur) {
    ORB_CHECK_ARG(cur >= 0 && cur < m->n_keyframes, "cur outside [0, n_keyframes)");
    return ORB_OK;
}

}  // namespace

extern "C" int orblc_connected_device(const orblc_map* m, int32_t cur, int32_t* connected, int32_t* n_connected, void* stream) {
    int rc;
    if ((rc = lc_check(m, LC_ROWS))) return rc;
    if ((rc = lc_cur_check(m, cur))) return rc;
    ORB_CHECK_ARG(connected && n_connected, "null output");
    hipLaunchKernelGGL(lc_connected_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, m->n_keyframes, m->conn_cap, m->ord_slot,
                       m->n_ord, cur, connected, n_connected);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orblc_propagate_device(const orblc_map* m, int32_t cur, const float* scw, const int32_t* connected,
                                      int32_t max_connected, float* vertex_sim3, float* edge_sim3, int32_t* point_ref,
                                      int32_t* items, void* stream) {
    int rc;
    if ((rc = lc_check(m, LC_POINTS))) return rc;
    if ((rc = lc_cur_check(m, cur))) return rc;
    if ((rc = lc_list_check(m, connected, max_connected))) return rc;
    ORB_CHECK_ARG(scw && vertex_sim3 && edge_sim3 && (point_ref || m->n_mappoints == 0), "null argument");
    ORB_CHECK_ARG(13LL * m->n_keyframes < MM_MAX_ENTRIES, "a table of 2^31 entries or more");
    if ((rc = g_lc.use_current_device())) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t K = m->n_keyframes, M = m->n_mappoints;
    LcWork w{};
    auto carve = [&](char* base) {
        Carver c{base};
        c.take(w.ow_entry, 3 * K); c.take(w.ow_corr, 3 * K); c.take(w.new_pose, 12 * K); c.take(w.is_conn, K); c.take(w.claim, M);
        return c.off;
    };
    if ((rc = g_lc.ws.reserve(carve(nullptr)))) return rc;
    carve(g_lc.ws.as<char>());
    LcMap t{};
    t.pts.K = m->n_keyframes; t.pts.M = m->n_mappoints; t.pts.kf_cap = m->kf_cap; t.pts.n_obs = m->n_obs; t.pts.n_levels = m->n_levels;
    t.pts.mp_bad = m->mp_bad; t.pts.mp_xw = m->mp_xw; t.pts.mp_ref_kf = m->mp_ref_kf; t.pts.mp_obs_off = m->mp_obs_off;
    t.pts.mp_obs_kf = m->mp_obs_kf; t.pts.mp_obs_idx = m->mp_obs_idx; t.pts.kf_n = m->kf_n; t.pts.kf_kp_octave = m->kf_kp_octave;
    t.pts.kf_ow = w.ow_entry; t.pts.mp_normal = m->mp_normal; t.pts.mp_max_min = m->mp_max_min;
    for (int l = 0; l < m->n_levels; l++) t.pts.scale[l] = m->scale_factors[l];
    t.conn_cap = m->conn_cap; t.kf_id = m->kf_id; t.kf_mappoint = m->kf_mappoint; t.mp_xw = m->mp_xw; t.kf_pose = m->kf_pose;
    t.mp_corrected_by = m->mp_corrected_by; t.mp_corrected_ref = m->mp_corrected_ref;
    const unsigned most = (unsigned)std::max<size_t>(std::max(K, M), 1);
    hipLaunchKernelGGL(lc_keyframe_kernel, dim3(std::min((most + 255) / 256, 1024u)), dim3(256), 0, st, t, w, cur, scw, connected,
                       max_connected, vertex_sim3, edge_sim3, items);
    if (max_connected && M)
        hipLaunchKernelGGL(lc_claim_kernel, dim3((unsigned)max_connected, (unsigned)(m->kf_cap + 255) / 256), dim3(256), 0, st, t, w,
                           cur, connected);
    hipLaunchKernelGGL(lc_point_kernel, dim3((most + 255) / 256), dim3(256), 0, st, t, w, cur, vertex_sim3, edge_sim3, point_ref);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orblc_loop_connections_device(const orblc_map* m, const int32_t* connected, int32_t max_connected,
                                             int32_t* conn_kf, int32_t* conn_begin, int32_t* conn_slot, int32_t* n_connections,
                                             void* stream) {
    int rc;
    if ((rc = lc_check(m, LC_GRAPH))) return rc;
    if ((rc = lc_list_check(m, connected, max_connected))) return rc;
    ORB_CHECK_ARG(conn_kf && conn_begin && conn_slot && n_connections, "null output");
    if ((rc = g_lc.use_current_device())) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t K = m->n_keyframes, cap = m->conn_cap, C = max_connected;
    LcSets s{};
    auto carve = [&](char* base) {
        Carver c{base};
        c.take(s.set, C * cap); c.take(s.count, C); c.take(s.sorted, C + 1); c.take(s.prev, cap); c.take(s.n_prev, 1);
        c.take(s.status, K);
        return c.off;
    };
    if ((rc = g_lc.ws.reserve(carve(nullptr)))) return rc;
    carve(g_lc.ws.as<char>());
    orbmm_graph g = orblc_graph(m);
    g.status = s.status;
    static_assert(ORBMM_OK == 0, "status is cleared with a memset");
    if (K) ORB_HIP_TRY(hipMemsetAsync(m->status, 0, K * sizeof(int32_t), st));
    for (int j = 0; j < max_connected; j++) {
        hipLaunchKernelGGL(lc_snapshot_kernel, dim3(1), dim3(256), 0, st, (int)K, (int)cap, m->ord_slot, m->n_ord, connected, j, s);
        if ((rc = orbmm_update_connections_device(&g, 1, connected + j, stream))) return rc;
        hipLaunchKernelGGL(lc_difference_kernel, dim3(1), dim3(64), 0, st, (int)K, (int)cap, m->conn_slot, m->n_conn, connected,
                           max_connected, j, s, m->status);
    }
    hipLaunchKernelGGL(lc_pack_kernel, dim3(1), dim3(256), 0, st, (int)K, (int)cap, connected, max_connected, s, conn_kf, conn_begin,
                       conn_slot, n_connections);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbba_essential_graph_edges_device(const orbba_eg_tables* g, int32_t n_loop_slots, int32_t n_covis_slots,
                                                  int32_t n_conn_slots, int32_t min_weight, int32_t capacity, int32_t* edge_i,
                                                  int32_t* edge_j, uint8_t* edge_table, int32_t* n_edges, void* stream) {
    ORB_CHECK_ARG(g && n_edges, "null argument");
    ORB_CHECK_ARG(capacity >= 0 && (capacity == 0 || (edge_i && edge_j && edge_table)), "null edge array");
    const int V = g->n_keyframes;
    ORB_CHECK_ARG(V >= 1 && g->n_connections >= 0 && n_loop_slots >= 0 && n_covis_slots >= 0 && n_conn_slots >= 0, "bad sizes");
    ORB_CHECK_ARG(g->kf_id && g->parent && g->loop_begin && g->covis_begin, "null table");
    ORB_CHECK_ARG((n_loop_slots == 0 || g->loop_slot) && (n_covis_slots == 0 || (g->covis_slot && g->covis_weight)), "null table");
    ORB_CHECK_ARG(g->n_connections == 0 || (g->conn_kf && g->conn_begin && (n_conn_slots == 0 || g->conn_slot)),
                  "null connection table");
    ORB_CHECK_ARG(g->curr_slot >= 0 && g->curr_slot < V && g->loop_kf_slot >= 0 && g->loop_kf_slot < V,
                  "curr_slot / loop_kf_slot out of range");
    int rc;
    if ((rc = g_lc.use_current_device())) return rc;
    hipStream_t st = (hipStream_t)stream;
    int32_t *pair, *n_kept, *count;
    auto carve = [&](char* base) {
        Carver c{base};
        c.take(pair, 2 * (size_t)n_conn_slots); c.take(n_kept, 1); c.take(count, (size_t)V + 1);
        return c.off;
    };
    if ((rc = g_lc.ws.reserve(carve(nullptr)))) return rc;
    carve(g_lc.ws.as<char>());
    const EgDev d{*g, n_loop_slots, n_covis_slots, n_conn_slots};
    hipLaunchKernelGGL(eg_loop_edges_kernel, dim3(1), dim3(64 * MM_CULL_WAVES), 0, st, d, min_weight, capacity, edge_i, edge_j,
                       edge_table, pair, n_kept);
    hipLaunchKernelGGL(eg_count_kernel, dim3((V + 255) / 256), dim3(256), 0, st, d, min_weight, pair, n_kept, count);
    hipLaunchKernelGGL(eg_scan_kernel, dim3(1), dim3(256), 0, st, V, count, n_kept, n_edges);
    hipLaunchKernelGGL(eg_fill_kernel, dim3((std::max(V, capacity) + 255) / 256), dim3(256), 0, st, d, min_weight, pair, n_kept, count,
                       capacity, edge_i, edge_j, edge_table);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

// ---------------------------------------------------------------------------------------------- host forms
namespace {

void lc_add_rows(Mirror& io, orblc_map& d, bool out) {
    const size_t K = d.n_keyframes, rows = K * d.conn_cap;
    io.add(d.conn_slot, rows, true, out); io.add(d.conn_weight, rows, true, out); io.add(d.n_conn, K, true, out);
    io.add(d.ord_slot, rows, true, out); io.add(d.ord_weight, rows, true, out); io.add(d.n_ord, K, true, out);
}

int lc_list_check_host(const orblc_map* m, const int32_t* connected, int32_t max_connected) {
    return check_range(connected, max_connected, -1, m->n_keyframes, "connected entry outside [-1, n_keyframes)");
}

}  // namespace

extern "C" int orblc_connected(const orblc_map* m, int32_t cur, int32_t* connected, int32_t* n_connected, int device) {
    int rc;
    if ((rc = lc_check(m, LC_ROWS))) return rc;
    if ((rc = lc_cur_check(m, cur))) return rc;
    ORB_CHECK_ARG(connected && n_connected, "null output");
    const orbmm_graph g = orblc_graph(m);
    if ((rc = mm_graph_rows_check_host(&g))) return rc;   // before any copy
    orblc_map d = *m;
    Mirror io;
    const size_t K = m->n_keyframes;
    io.add(d.ord_slot, K * m->conn_cap, true, false); io.add(d.n_ord, K, true, false);
    io.add(connected, (size_t)m->conn_cap + 1, false, true); io.add(n_connected, 1, false, true);
    return run_host(g_lc, device, io, [&] { return orblc_connected_device(&d, cur, connected, n_connected, nullptr); });
}

extern "C" int orblc_propagate(const orblc_map* m, int32_t cur, const float* scw, const int32_t* connected, int32_t max_connected,
                               float* vertex_sim3, float* edge_sim3, int32_t* point_ref, int32_t* items, int device) {
    int rc;
    if ((rc = lc_check(m, LC_POINTS))) return rc;
    if ((rc = lc_cur_check(m, cur))) return rc;
    if ((rc = lc_list_check(m, connected, max_connected))) return rc;
    ORB_CHECK_ARG(scw && vertex_sim3 && edge_sim3 && (point_ref || m->n_mappoints == 0), "null argument");
    ORB_CHECK_ARG(13LL * m->n_keyframes < MM_MAX_ENTRIES, "a table of 2^31 entries or more");
    for (int i = 0; i < 13; i++) ORB_CHECK_ARG(std::isfinite(scw[i]), "non-finite scw");
    ORB_CHECK_ARG(scw[12] > 0.f, "the scale of scw must be positive");
    const orbmm_points p = lc_points(*m);
    if ((rc = mm_points_check_host(&p))) return rc;   // before any copy
    if ((rc = check_range(m->kf_mappoint, (size_t)m->n_keyframes * m->kf_cap, -1, m->n_mappoints,
                          "kf_mappoint entry outside [-1, n_mappoints)")))
        return rc;
    if ((rc = lc_list_check_host(m, connected, max_connected))) return rc;
    const size_t K = m->n_keyframes, M = m->n_mappoints, n_obs = m->mp_obs_off[M];
    orblc_map d = *m;
    Mirror io;
    io.add(d.kf_id, K, true, false); io.add(d.kf_n, K, true, false); io.add(d.kf_mappoint, K * m->kf_cap, true, false);
    io.add(d.mp_bad, M, true, false); io.add(d.mp_obs_off, M + 1, true, false); io.add(d.mp_obs_kf, n_obs, true, false);
    io.add(d.mp_obs_idx, n_obs, true, false); io.add(d.mp_ref_kf, M, true, false); io.add(d.kf_kp_octave, K * m->kf_cap, true, false);
    io.add(d.mp_xw, M * 3, true, true); io.add(d.kf_pose, K * 12, true, true); io.add(d.mp_normal, M * 3, true, true);
    io.add(d.mp_max_min, M * 2, true, true); io.add(d.mp_corrected_by, M, true, true); io.add(d.mp_corrected_ref, M, true, true);
    io.add(scw, 13, true, false); io.add(connected, (size_t)max_connected, true, false);
    io.add(vertex_sim3, K * 13, false, true); io.add(edge_sim3, K * 13, false, true); io.add(point_ref, M, false, true);
    io.add(items, (size_t)max_connected, false, true);
    return run_host(g_lc, device, io, [&] {
        return orblc_propagate_device(&d, cur, scw, connected, max_connected, vertex_sim3, edge_sim3, point_ref, items, nullptr);
    });
}

extern "C" int orblc_loop_connections(const orblc_map* m, const int32_t* connected, int32_t max_connected, int32_t* conn_kf,
                                      int32_t* conn_begin, int32_t* conn_slot, int32_t* n_connections, int device) {
    int rc;
    if ((rc = lc_check(m, LC_GRAPH))) return rc;
    if ((rc = lc_list_check(m, connected, max_connected))) return rc;
    ORB_CHECK_ARG(conn_kf && conn_begin && conn_slot && n_connections, "null output");
    const orbmm_graph g = orblc_graph(m);
    if (m->n_keyframes && (rc = mm_graph_check_host(&g, 0, nullptr))) return rc;   // before any copy
    if ((rc = lc_list_check_host(m, connected, max_connected))) return rc;
    const size_t K = m->n_keyframes, M = m->n_mappoints, C = max_connected;
    orblc_map d = *m;
    Mirror io;
    io.add(d.kf_id, K, true, false); io.add(d.kf_n, K, true, false); io.add(d.kf_mappoint, K * m->kf_cap, true, false);
    io.add(d.mp_bad, M, true, false); io.add(d.mp_obs_off, M + 1, true, false);
    io.add(d.mp_obs_kf, K ? (size_t)m->mp_obs_off[M] : 0, true, false);
    lc_add_rows(io, d, true);
    io.add(d.kf_first_connection, K, true, true); io.add(d.kf_parent, K, true, true); io.add(d.kf_covis, K * MM_COVIS, true, true);
    io.add(d.status, K, false, true);
    io.add(connected, C, true, false);
    io.add(conn_kf, C, false, true); io.add(conn_begin, C + 1, false, true); io.add(conn_slot, C * m->conn_cap, true, true);
    io.add(n_connections, 1, false, true);
    return run_host(g_lc, device, io, [&] {
        return orblc_loop_connections_device(&d, connected, max_connected, conn_kf, conn_begin, conn_slot, n_connections, nullptr);
    });
}
