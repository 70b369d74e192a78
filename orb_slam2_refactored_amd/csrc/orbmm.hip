// orbmm.hip — map maintenance on gfx950 (include/orbslam2_amd.h, "Map maintenance"): MapPoint::UpdateNormalAndDepth
// batched over map points, KeyFrame::UpdateConnections with AddConnection / UpdateBestCovisibles batched over
// keyframes, the GetChildren() CSR and the packed covisibility tables.
//
// Reference: src/MapPoint.cc:341-380, src/KeyFrame.cc:94-119, 235-309.  The arithmetic is csrc/mm_normal.h's, the
// sequential rules csrc/mm_connect.h's.  Passes, stream-ordered, nothing read back:
//   mm_center_kernel   one thread per keyframe: Ow = (-R^T) t
//   mm_normal_kernel   one thread per point: the float sum over its observations in CSR order
//   mm_count_kernel    one workgroup per item: an LDS histogram (integer atomics) over a window of keyframe slots,
//                      one pass per window, stored as the item's dense counter row
//   mm_item_kernel     one wavefront per item: the largest count, its lowest and highest slot, the threshold flag
//   mm_target_kernel   one wavefront per keyframe: the walk through the batch on a working row, the capacity check,
//                      then the commit (two rank sorts)
//   mm_children_kernel one workgroup: count, scan, fill with kf_parent staged in LDS tiles
//   mm_offsets_kernel  one workgroup: the CSR offsets of the packed rows; mm_pack_kernel fills them
// The culls (src/LocalMapping.cc:335-369, 641-701; the rules are csrc/mm_cull.h's):
//   mm_cull_points_kernel     one thread per entry of the recent list: the decision and SetBadFlag;
//   mm_cull_list_kernel       one workgroup: the stable compaction of the list in place
//   mm_cull_keyframes_kernel  one workgroup walks the targets in order: all lanes over the target's row for the count and
//                             for EraseObservation, one wavefront per neighbour for EraseConnection, one for the tree
//   mm_compact_*_kernel       the observation CSR without erased entries: count per point, one scan, fill
// The observation edits (MapPoint::AddObservation / Replace and the loops that call them; the rules are
// csrc/mm_observe.h's) are orbmm_observe.hip.  The lane groups and the scan both units launch with are
// csrc/mm_groups.h's, the per-thread buffers and the shared table checks csrc/mm_host.h's; the host entries stage with
// common.h's Mirror and run_host.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "mm_connect.h"
#include "mm_cull.h"
#include "mm_groups.h"
#include "mm_host.h"
#include "mm_normal.h"

namespace orbamd {

constexpr int MM_WINDOW_MAX = 8192, MM_WINDOW_MIN = 64;   // int32 counters in LDS: 32 KiB at most
constexpr int MM_TILE = 1024;

__global__ __launch_bounds__(256) void mm_center_kernel(const float* kf_pose, float* kf_ow, int K) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < K) mm_center(kf_pose + 12 * (size_t)k, kf_ow + 3 * (size_t)k);
}

__global__ __launch_bounds__(256) void mm_normal_kernel(MmPoints t, const int32_t* point, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    mm_update_point(t, point ? point[i] : i);
}

__global__ __launch_bounds__(256) void mm_count_kernel(MmGraph t, const int32_t* item, int32_t* cnt, int window) {
    extern __shared__ int32_t s_hist[];
    const int k = item[blockIdx.x], K = t.K;
    int32_t* row = cnt + (size_t)blockIdx.x * K;
    const bool live = k >= 0 && k < K;
    for (int base = 0; base < K; base += window) {
        const int w = ::min(window, K - base);
        for (int s = threadIdx.x; s < w; s += 256) s_hist[s] = 0;
        __syncthreads();
        if (live)
            for (int i = threadIdx.x; i < t.kf_cap; i += 256) {
                const int p = mm_counted_point(t, k, i);
                if (p < 0) continue;
                int e0, e1;
                mm_obs_range(t, p, e0, e1);
                for (int e = e0; e < e1; e++) {
                    const int o = t.mp_obs_kf[e];
                    if (o >= base && o < base + w && mm_counted_observer(t, k, o)) atomicAdd(&s_hist[o - base], 1);
                }
            }
        __syncthreads();
        for (int s = threadIdx.x; s < w; s += 256) row[base + s] = s_hist[s];
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void mm_item_kernel(const int32_t* item, const int32_t* cnt, MmItem* items, int K) {
    const MmWave g{(int)threadIdx.x};
    const MmItem it = mm_item_summary(g, cnt + (size_t)blockIdx.x * K, K, item[blockIdx.x]);
    if (threadIdx.x == 0) items[blockIdx.x] = it;
}

__global__ __launch_bounds__(64) void mm_target_kernel(MmGraph t, int B, const MmItem* items, const int32_t* cnt,
                                                        int32_t* work) {
    const MmWave g{(int)threadIdx.x};
    const int X = blockIdx.x;
    int32_t* ws = work + 2 * (size_t)X * t.conn_cap;
    int32_t* ww = ws + t.conn_cap;
    const MmWalk r = mm_walk(g, t, X, B, items, cnt, ws, ww);
    mm_commit(g, t, X, items, ws, ww, r);
}

// bad (may be NULL): keyframes that are nobody's child
__global__ __launch_bounds__(256) void mm_children_kernel(int K, const int32_t* parent, const uint8_t* bad, int32_t* off,
                                                          int32_t* idx) {
    __shared__ int32_t s_par[MM_TILE];
    // count: off[p] = the number of k with parent[k] == p
    for (int pb = 0; pb < K; pb += 256) {
        const int p = pb + (int)threadIdx.x;
        int c = 0;
        for (int tb = 0; tb < K; tb += MM_TILE) {
            const int w = ::min(MM_TILE, K - tb);
            for (int j = threadIdx.x; j < w; j += 256) s_par[j] = (bad && bad[tb + j]) ? -1 : parent[tb + j];
            __syncthreads();
            if (p < K)
                for (int j = 0; j < w; j++) c += s_par[j] == p ? 1 : 0;
            __syncthreads();
        }
        if (p < K) off[p] = c;
    }
    __syncthreads();
    mm_block_scan<int32_t>(off, K, off, 0, K, 0);
    __syncthreads();
    // fill: k ascending per parent; the lists hold K entries at most in all
    for (int pb = 0; pb < K; pb += 256) {
        const int p = pb + (int)threadIdx.x;
        int pos = p < K ? off[p] : 0;
        for (int tb = 0; tb < K; tb += MM_TILE) {
            const int w = ::min(MM_TILE, K - tb);
            for (int j = threadIdx.x; j < w; j += 256) s_par[j] = (bad && bad[tb + j]) ? -1 : parent[tb + j];
            __syncthreads();
            if (p < K)
                for (int j = 0; j < w; j++)
                    if (s_par[j] == p && pos < K) idx[pos++] = tb + j;
            __syncthreads();
        }
    }
}

// mode 0: the ordered rows of every keyframe; mode 1: the connection rows of the queries (+ 1 with append_self; a
// query outside the table has an empty list)
__global__ __launch_bounds__(256) void mm_offsets_kernel(MmGraph t, orbmm_csr o, int mode, int32_t* q_count) {
    if (mode == 0) {
        mm_block_scan<int32_t>(t.n_ord, t.K, o.covis_begin, 0, t.conn_cap, 0);
        return;
    }
    for (int q = threadIdx.x; q < o.n_queries; q += 256) {
        const int k = o.query[q];
        q_count[q] = (k >= 0 && k < t.K) ? mm_clamp(t.n_conn[k], 0, t.conn_cap) + (o.append_self ? 1 : 0) : 0;
    }
    __syncthreads();
    mm_block_scan<int32_t>(q_count, o.n_queries, o.conn_off, 0, t.conn_cap + 1, 0);
}

__global__ __launch_bounds__(256) void mm_pack_kernel(MmGraph t, orbmm_csr o, int mode) {
    const int cap = t.conn_cap, row = blockIdx.x, j = blockIdx.y * 256 + threadIdx.x;
    if (mode == 0) {
        if (j >= mm_clamp(t.n_ord[row], 0, cap)) return;
        const size_t at = (size_t)o.covis_begin[row] + j;   // <= K * cap: the scan clamps as this does
        const int s = t.ord_slot[(size_t)row * cap + j];
        o.covis_slot[at] = (s >= 0 && s < t.K && !(o.kf_bad && o.kf_bad[s])) ? s : -1;
        o.covis_weight[at] = t.ord_weight[(size_t)row * cap + j];
        return;
    }
    const int k = o.query[row];
    if (k < 0 || k >= t.K) return;
    const int n = mm_clamp(t.n_conn[k], 0, cap);
    const size_t at = (size_t)o.conn_off[row] + j;
    if (j < n)
        o.conn_idx[at] = t.conn_slot[(size_t)k * cap + j];
    else if (j == n && o.append_self)
        o.conn_idx[at] = k;
}

// ---------------------------------------------------------------------------------------------- the culls
__global__ __launch_bounds__(256) void mm_cull_points_kernel(MmCull t, const int32_t* recent, int n, int cur_kf_id, int min_obs,
                                                             uint8_t* keep) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int p = recent[i], d = cull_point_decision(t, p, cur_kf_id, min_obs);
    if (d == CULL_BAD) cull_set_bad(t, p);
    keep[i] = d == CULL_KEEP ? 1 : 0;
}

// recent[0 .. n) without the entries whose keep is 0, in place: a chunk is read before anything of it is written, and
// what is written lies at or below it.
__global__ __launch_bounds__(64 * MM_CULL_WAVES) void mm_cull_list_kernel(int32_t* recent, int n, const uint8_t* keep,
                                                                           int32_t* n_out) {
    __shared__ int32_t s_red[MM_CULL_WAVES];
    const MmBlock b{(int)threadIdx.x, s_red};
    int at = 0;
    for (int base = 0; base < n; base += b.width) {   // uniform trip count
        const int i = base + b.lane;
        const bool flag = i < n && keep[i];
        const int v = i < n ? recent[i] : -1;
        int total;
        const int off = b.prefix(flag, total);   // syncs: every lane has read its entry
        if (flag) recent[at + off] = v;
        at += total;
    }
    if (b.lane == 0) *n_out = at;
}

__global__ __launch_bounds__(64 * MM_CULL_WAVES) void mm_cull_keyframes_kernel(MmCull t, int cur, int monocular, float th_depth,
                                                                                int32_t* culled, int32_t* n_culled,
                                                                                int32_t* status, int32_t* scratch) {
    __shared__ int32_t s_red[MM_CULL_WAVES];
    const MmBlock b{(int)threadIdx.x, s_red};
    MmSubWave w;
    w.lane = (int)threadIdx.x & 63;
    cull_keyframes(b, w, (int)threadIdx.x >> 6, MM_CULL_WAVES, t, cur, monocular != 0, th_depth, culled, n_culled, status, scratch);
}

__global__ __launch_bounds__(256) void mm_compact_count_kernel(int M, int n_obs, const int32_t* off, const int32_t* kf,
                                                               int32_t* out_off) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < M) out_off[p] = cull_compact_point(n_obs, off, kf, nullptr, p, 0, nullptr, nullptr);
}

__global__ __launch_bounds__(256) void mm_compact_scan_kernel(int M, int n_obs, int32_t* out_off) {
    mm_block_scan<int32_t>(out_off, M, out_off, 0, n_obs, 0);
}

__global__ __launch_bounds__(256) void mm_compact_fill_kernel(int M, int n_obs, const int32_t* off, const int32_t* kf,
                                                              const int32_t* idx, const int32_t* out_off, int32_t* out_kf,
                                                              int32_t* out_idx) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < M) cull_compact_point(n_obs, off, kf, idx, p, out_off[p], out_kf, out_idx);
}

}  // namespace orbamd

using namespace orbamd;

namespace {

MmGraph mm_graph(const orbmm_graph& g) {
    return MmGraph{g.n_keyframes, g.n_mappoints, g.kf_cap, g.conn_cap, g.n_obs, g.kf_id, g.kf_n, g.kf_mappoint, g.mp_bad,
                   g.mp_obs_off, g.mp_obs_kf, g.conn_slot, g.conn_weight, g.n_conn, g.ord_slot, g.ord_weight, g.n_ord,
                   g.kf_first_connection, g.kf_parent, g.kf_covis, g.status};
}

int mm_csr_check(const orbmm_graph* g, const orbmm_csr* o, bool& covis, bool& conn) {
    int rc;
    if ((rc = mm_graph_check(g, true))) return rc;
    ORB_CHECK_ARG(o, "null csr");
    covis = o->covis_begin || o->covis_slot || o->covis_weight;
    conn = o->conn_off || o->conn_idx;
    ORB_CHECK_ARG(!covis || (o->covis_begin && o->covis_slot && o->covis_weight), "null covis array");
    ORB_CHECK_ARG(!conn || (o->conn_off && o->conn_idx), "null conn array");
    ORB_CHECK_ARG(!conn || o->n_queries >= 0, "negative sizes");
    ORB_CHECK_ARG(!conn || o->n_queries == 0 || o->query, "null query");
    ORB_CHECK_ARG(!conn || (long long)o->n_queries * (g->conn_cap + 1LL) < MM_MAX_ENTRIES, "a table of 2^31 entries or more");
    return ORB_OK;
}

int mm_window() {   // read per call
    int w = MM_WINDOW_MAX;
    if (const char* e = getenv("ORBMM_WINDOW")) w = atoi(e);
    return std::max(MM_WINDOW_MIN, std::min(MM_WINDOW_MAX, w));
}

}  // namespace

extern "C" int orbmm_update_normal_depth_device(const orbmm_points* p, void* stream) {
    int rc;
    if ((rc = mm_points_check(p))) return rc;
    const int n = p->point ? p->n_points : p->n_mappoints;
    if (n == 0 || p->n_keyframes == 0) return ORB_OK;   // without keyframes no reference slot is in the table
    if ((rc = mm_use_current_device())) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = g_mm.ws.reserve((size_t)p->n_keyframes * 12))) return rc;
    MmPoints t{};
    t.K = p->n_keyframes; t.M = p->n_mappoints; t.kf_cap = p->kf_cap; t.n_obs = p->n_obs; t.n_levels = p->n_levels;
    t.mp_bad = p->mp_bad; t.mp_xw = p->mp_xw; t.mp_ref_kf = p->mp_ref_kf; t.mp_obs_off = p->mp_obs_off;
    t.mp_obs_kf = p->mp_obs_kf; t.mp_obs_idx = p->mp_obs_idx; t.kf_n = p->kf_n; t.kf_kp_octave = p->kf_kp_octave;
    t.kf_ow = g_mm.ws.as<float>(); t.mp_normal = p->mp_normal; t.mp_max_min = p->mp_max_min;
    for (int l = 0; l < p->n_levels; l++) t.scale[l] = p->scale_factors[l];
    hipLaunchKernelGGL(mm_center_kernel, dim3((t.K + 255) / 256), dim3(256), 0, st, p->kf_pose, g_mm.ws.as<float>(), t.K);
    hipLaunchKernelGGL(mm_normal_kernel, dim3((n + 255) / 256), dim3(256), 0, st, t, p->point, n);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbmm_update_connections_device(const orbmm_graph* g, int32_t n_items, const int32_t* item, void* stream) {
    int rc;
    if ((rc = mm_graph_check(g, false))) return rc;
    if ((rc = mm_items_check(g, n_items, item))) return rc;
    if (g->n_keyframes == 0) return ORB_OK;
    if ((rc = mm_use_current_device())) return rc;
    hipStream_t st = (hipStream_t)stream;
    const MmGraph t = mm_graph(*g);
    const size_t K = t.K, B = n_items;
    int32_t *cnt, *work;   // the counters, the item summaries, the working rows
    MmItem* items;
    auto carve = [&](char* base) {
        Carver c{base};
        c.take(cnt, B * K); c.take(items, B); c.take(work, 2 * K * t.conn_cap);
        return c.off;
    };
    if ((rc = g_mm.ws.reserve(carve(nullptr)))) return rc;
    carve(g_mm.ws.as<char>());
    if (B) {
        const int window = std::min(mm_window(), std::max((int)K, MM_WINDOW_MIN));
        hipLaunchKernelGGL(mm_count_kernel, dim3((unsigned)B), dim3(256), (size_t)window * 4, st, t, item, cnt, window);
        hipLaunchKernelGGL(mm_item_kernel, dim3((unsigned)B), dim3(64), 0, st, item, cnt, items, (int)K);
    }
    hipLaunchKernelGGL(mm_target_kernel, dim3((unsigned)K), dim3(64), 0, st, t, (int)B, items, cnt, work);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

namespace {

// kf_bad (may be NULL): keyframes that are nobody's child
int mm_children_device(int32_t n_keyframes, const int32_t* kf_parent, const uint8_t* kf_bad, bool need_bad, int32_t* kf_child_off,
                       int32_t* kf_child_idx, void* stream) {
    ORB_CHECK_ARG(n_keyframes >= 0, "negative sizes");
    ORB_CHECK_ARG(kf_child_off && (n_keyframes == 0 || (kf_parent && (kf_bad || !need_bad) && kf_child_idx)), "null children array");
    hipLaunchKernelGGL(mm_children_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, n_keyframes, kf_parent, kf_bad,
                       kf_child_off, kf_child_idx);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

int mm_children(int32_t n_keyframes, const int32_t* kf_parent, const uint8_t* kf_bad, bool need_bad, int32_t* kf_child_off,
                int32_t* kf_child_idx, int device) {
    ORB_CHECK_ARG(n_keyframes >= 0, "negative sizes");
    ORB_CHECK_ARG(kf_child_off && (n_keyframes == 0 || (kf_parent && (kf_bad || !need_bad) && kf_child_idx)), "null children array");
    int rc;
    if ((rc = check_range(kf_parent, n_keyframes, -1, n_keyframes, "kf_parent outside [-1, n_keyframes)"))) return rc;
    if (n_keyframes == 0) {
        kf_child_off[0] = 0;
        return ORB_OK;
    }
    const size_t K = n_keyframes;
    Mirror io;
    io.add(kf_parent, K, true, false); io.add(kf_bad, K, true, false); io.add(kf_child_off, K + 1, false, true);
    io.add(kf_child_idx, K, true, true);
    return run_host(g_mm, device, io, [&] {
        return mm_children_device(n_keyframes, kf_parent, kf_bad, need_bad, kf_child_off, kf_child_idx, nullptr);
    });
}

}  // namespace

extern "C" int orbmm_children_device(int32_t n_keyframes, const int32_t* kf_parent, int32_t* kf_child_off,
                                     int32_t* kf_child_idx, void* stream) {
    return mm_children_device(n_keyframes, kf_parent, nullptr, false, kf_child_off, kf_child_idx, stream);
}

extern "C" int orbmm_children_live_device(int32_t n_keyframes, const int32_t* kf_parent, const uint8_t* kf_bad,
                                          int32_t* kf_child_off, int32_t* kf_child_idx, void* stream) {
    return mm_children_device(n_keyframes, kf_parent, kf_bad, true, kf_child_off, kf_child_idx, stream);
}

extern "C" int orbmm_covis_csr_device(const orbmm_graph* g, const orbmm_csr* out, void* stream) {
    int rc;
    bool covis = false, conn = false;
    if ((rc = mm_csr_check(g, out, covis, conn))) return rc;
    if ((rc = mm_use_current_device())) return rc;
    hipStream_t st = (hipStream_t)stream;
    const MmGraph t = mm_graph(*g);
    const unsigned cols = (unsigned)(t.conn_cap + 1 + 255) / 256;
    if (covis) {
        hipLaunchKernelGGL(mm_offsets_kernel, dim3(1), dim3(256), 0, st, t, *out, 0, (int32_t*)nullptr);
        if (t.K) hipLaunchKernelGGL(mm_pack_kernel, dim3((unsigned)t.K, cols), dim3(256), 0, st, t, *out, 0);
    }
    if (conn) {
        if ((rc = g_mm.ws.reserve(std::max<size_t>((size_t)out->n_queries * 4, 256)))) return rc;
        hipLaunchKernelGGL(mm_offsets_kernel, dim3(1), dim3(256), 0, st, t, *out, 1, g_mm.ws.as<int32_t>());
        if (out->n_queries) hipLaunchKernelGGL(mm_pack_kernel, dim3((unsigned)out->n_queries, cols), dim3(256), 0, st, t, *out, 1);
    }
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbmm_update_normal_depth(const orbmm_points* p, int device) {
    int rc;
    if ((rc = mm_points_check(p))) return rc;
    const int n = p->point ? p->n_points : p->n_mappoints;
    if (n == 0 || p->n_keyframes == 0) return ORB_OK;
    if ((rc = mm_points_check_host(p))) return rc;   // before any copy
    const size_t K = p->n_keyframes, M = p->n_mappoints, n_obs = p->mp_obs_off[M];
    orbmm_points d = *p;
    Mirror io;
    io.add(d.mp_bad, M, true, false); io.add(d.mp_xw, M * 3, true, false); io.add(d.mp_ref_kf, M, true, false);
    io.add(d.mp_obs_off, M + 1, true, false); io.add(d.mp_obs_kf, n_obs, true, false); io.add(d.mp_obs_idx, n_obs, true, false);
    io.add(d.kf_pose, K * 12, true, false); io.add(d.kf_n, K, true, false); io.add(d.kf_kp_octave, K * p->kf_cap, true, false);
    io.add(d.point, (size_t)p->n_points, true, false);
    io.add(d.mp_normal, M * 3, true, true); io.add(d.mp_max_min, M * 2, true, true);
    return run_host(g_mm, device, io, [&] { return orbmm_update_normal_depth_device(&d, nullptr); });
}

namespace {

void mm_add_rows(Mirror& io, orbmm_graph& d, bool out) {
    const size_t K = d.n_keyframes, rows = K * d.conn_cap;
    io.add(d.conn_slot, rows, true, out); io.add(d.conn_weight, rows, true, out); io.add(d.n_conn, K, true, out);
    io.add(d.ord_slot, rows, true, out); io.add(d.ord_weight, rows, true, out); io.add(d.n_ord, K, true, out);
}

}  // namespace

extern "C" int orbmm_update_connections(const orbmm_graph* g, int32_t n_items, const int32_t* item, int device) {
    int rc;
    if ((rc = mm_graph_check(g, false))) return rc;
    if ((rc = mm_items_check(g, n_items, item))) return rc;
    if (g->n_keyframes == 0) return ORB_OK;
    if ((rc = mm_graph_check_host(g, n_items, item))) return rc;   // before any copy
    const size_t K = g->n_keyframes, M = g->n_mappoints;
    orbmm_graph d = *g;
    const int32_t* d_item = item;
    Mirror io;
    io.add(d.kf_id, K, true, false); io.add(d.kf_n, K, true, false); io.add(d.kf_mappoint, K * g->kf_cap, true, false);
    io.add(d.mp_bad, M, true, false); io.add(d.mp_obs_off, M + 1, true, false);
    io.add(d.mp_obs_kf, (size_t)g->mp_obs_off[M], true, false);
    mm_add_rows(io, d, true);
    io.add(d.kf_first_connection, K, true, true); io.add(d.kf_parent, K, true, true); io.add(d.kf_covis, K * MM_COVIS, true, true);
    io.add(d.status, K, false, true);
    io.add(d_item, (size_t)n_items, true, false);
    return run_host(g_mm, device, io, [&] { return orbmm_update_connections_device(&d, n_items, d_item, nullptr); });
}

extern "C" int orbmm_children(int32_t n_keyframes, const int32_t* kf_parent, int32_t* kf_child_off, int32_t* kf_child_idx,
                              int device) {
    return mm_children(n_keyframes, kf_parent, nullptr, false, kf_child_off, kf_child_idx, device);
}

extern "C" int orbmm_children_live(int32_t n_keyframes, const int32_t* kf_parent, const uint8_t* kf_bad, int32_t* kf_child_off,
                                   int32_t* kf_child_idx, int device) {
    return mm_children(n_keyframes, kf_parent, kf_bad, true, kf_child_off, kf_child_idx, device);
}

extern "C" int orbmm_covis_csr(const orbmm_graph* g, const orbmm_csr* out, int device) {
    int rc;
    bool covis = false, conn = false;
    if ((rc = mm_csr_check(g, out, covis, conn))) return rc;
    if ((rc = mm_graph_rows_check_host(g))) return rc;   // before any copy
    if (conn && (rc = check_range(out->query, out->n_queries, 0, g->n_keyframes, "query outside [0, n_keyframes)"))) return rc;
    const size_t K = g->n_keyframes, rows = K * g->conn_cap, Q = conn ? out->n_queries : 0;
    orbmm_graph d = *g;
    orbmm_csr o = *out;
    Mirror io;
    mm_add_rows(io, d, false);
    io.add(o.kf_bad, K, true, false);
    if (covis) {
        io.add(o.covis_begin, K + 1, false, true); io.add(o.covis_slot, rows, true, true);
        io.add(o.covis_weight, rows, true, true);
    }
    if (conn) {
        io.add(o.query, Q, true, false); io.add(o.conn_off, Q + 1, false, true);
        io.add(o.conn_idx, Q * (g->conn_cap + 1), true, true);
    }
    return run_host(g_mm, device, io, [&] { return orbmm_covis_csr_device(&d, &o, nullptr); });
}

// ---------------------------------------------------------------------------------------------- the culls: entries
namespace {

MmCull mm_cull(const orbmm_cull& c) {
    return MmCull{c.n_keyframes, c.n_mappoints, c.kf_cap, c.conn_cap, c.n_obs, c.kf_id, c.kf_n, c.kf_mappoint, c.kf_kp_octave,
                  c.kf_uright, c.kf_depth, c.kf_pose, c.kf_bad, c.kf_not_erase, c.kf_to_be_erased, c.kf_tcp, c.mp_bad, c.mp_nobs,
                  c.mp_found, c.mp_visible, c.mp_first_kf_id, c.mp_ref_kf, c.mp_obs_off, c.mp_obs_kf, c.mp_obs_idx, c.conn_slot,
                  c.conn_weight, c.n_conn, c.ord_slot, c.ord_weight, c.n_ord, c.kf_parent, c.kf_covis};
}

int mm_cull_check(const orbmm_cull* c, bool keyframes) {
    ORB_CHECK_ARG(c, "null cull tables");
    ORB_CHECK_ARG(c->n_keyframes >= 0 && c->n_mappoints >= 0 && c->n_obs >= 0, "negative sizes");
    ORB_CHECK_ARG(c->kf_cap >= 1, "kf_cap must be at least 1");
    ORB_CHECK_ARG(!keyframes || c->conn_cap >= 1, "conn_cap must be at least 1");
    ORB_CHECK_ARG((long long)c->n_keyframes * c->kf_cap < MM_MAX_ENTRIES && 12LL * c->n_keyframes < MM_MAX_ENTRIES &&
                      (!keyframes || (long long)c->n_keyframes * c->conn_cap < MM_MAX_ENTRIES / 2),
                  "a table of 2^31 entries or more");
    ORB_CHECK_ARG(c->kf_mappoint && c->mp_bad && c->mp_nobs && c->mp_obs_off && c->mp_obs_kf && c->mp_obs_idx, "null map-point table");
    if (!keyframes) {
        ORB_CHECK_ARG(c->mp_found && c->mp_visible && c->mp_first_kf_id, "null map-point table");
        return ORB_OK;
    }
    ORB_CHECK_ARG(c->mp_ref_kf, "null map-point table");
    ORB_CHECK_ARG(c->kf_id && c->kf_n && c->kf_kp_octave && c->kf_uright && c->kf_depth && c->kf_pose && c->kf_bad &&
                      c->kf_not_erase && c->kf_to_be_erased && c->kf_tcp && c->kf_parent && c->kf_covis,
                  "null keyframe table");
    ORB_CHECK_ARG(c->conn_slot && c->conn_weight && c->n_conn && c->ord_slot && c->ord_weight && c->n_ord, "null row array");
    return ORB_OK;
}

// The host entries' checks of the tables both culls read.
int mm_cull_check_host(const orbmm_cull* c, bool keyframes) {
    const int K = c->n_keyframes, M = c->n_mappoints;
    int rc;
    if ((rc = check_csr(c->mp_obs_off, M, c->n_obs, "mp_obs"))) return rc;
    const size_t n_obs = c->mp_obs_off[M];
    if ((rc = check_range(c->mp_obs_kf, n_obs, 0, K, "mp_obs_kf entry outside [0, n_keyframes)"))) return rc;
    if ((rc = check_range(c->mp_obs_idx, n_obs, 0, c->kf_cap, "mp_obs_idx entry outside [0, kf_cap)"))) return rc;
    if ((rc = check_range(c->kf_mappoint, (size_t)K * c->kf_cap, -1, M, "kf_mappoint entry outside [-1, n_mappoints)"))) return rc;
    std::vector<int32_t> seen(K, -1);   // a keyframe twice in a point's observations
    for (int p = 0; p < M; p++)
        for (int e = c->mp_obs_off[p]; e < c->mp_obs_off[p + 1]; e++) {
            ORB_CHECK_ARG(seen[c->mp_obs_kf[e]] != p, "a keyframe twice in a map point's observations");
            seen[c->mp_obs_kf[e]] = p;
        }
    if (!keyframes) return ORB_OK;
    if ((rc = check_range(c->kf_n, K, 0, c->kf_cap + 1, "kf_n outside [0, kf_cap]"))) return rc;
    if ((rc = mm_check_rows_distinct(K, M, c->kf_cap, c->kf_n, c->kf_mappoint))) return rc;
    if ((rc = check_range(c->mp_ref_kf, M, -1, K, "mp_ref_kf outside [-1, n_keyframes)"))) return rc;
    if ((rc = check_range(c->kf_parent, K, -1, K, "kf_parent outside [-1, n_keyframes)"))) return rc;
    return mm_rows_check_host(K, c->conn_cap, c->conn_slot, c->n_conn, c->ord_slot, c->n_ord);
}

void mm_cull_add(Mirror& io, orbmm_cull& d, bool keyframes) {
    const size_t K = d.n_keyframes, M = d.n_mappoints, n_obs = d.mp_obs_off[M], rows = K * (keyframes ? d.conn_cap : 0);
    io.add(d.kf_mappoint, K * d.kf_cap, true, true); io.add(d.mp_bad, M, true, true); io.add(d.mp_nobs, M, true, keyframes);
    io.add(d.mp_obs_kf, n_obs, true, true); io.add(d.mp_obs_idx, n_obs, true, false);
    if (!keyframes) {
        io.add(d.mp_found, M, true, false); io.add(d.mp_visible, M, true, false); io.add(d.mp_first_kf_id, M, true, false);
        io.add(d.mp_obs_off, M + 1, true, false);
        return;
    }
    io.add(d.mp_ref_kf, M, true, true);
    io.add(d.kf_id, K, true, false); io.add(d.kf_n, K, true, false); io.add(d.kf_kp_octave, K * d.kf_cap, true, false);
    io.add(d.kf_uright, K * d.kf_cap, true, false); io.add(d.kf_depth, K * d.kf_cap, true, false);
    io.add(d.kf_pose, K * 12, true, false); io.add(d.kf_bad, K, true, true); io.add(d.kf_not_erase, K, true, false);
    io.add(d.kf_to_be_erased, K, true, true); io.add(d.kf_tcp, K * 12, true, true);
    io.add(d.conn_slot, rows, true, true); io.add(d.conn_weight, rows, true, true); io.add(d.n_conn, K, true, true);
    io.add(d.ord_slot, rows, true, true); io.add(d.ord_weight, rows, true, true); io.add(d.n_ord, K, true, true);
    io.add(d.kf_parent, K, true, true); io.add(d.kf_covis, K * MM_COVIS, true, true);
    io.add(d.mp_obs_off, M + 1, true, false);
}

}  // namespace

extern "C" int orbmm_cull_map_points_device(const orbmm_cull* c, int32_t n_recent, int32_t* recent, int32_t cur_kf_id,
                                            int32_t monocular, int32_t* n_recent_out, void* stream) {
    int rc;
    if ((rc = mm_cull_check(c, false))) return rc;
    ORB_CHECK_ARG(n_recent >= 0, "negative sizes");
    ORB_CHECK_ARG(n_recent_out && (n_recent == 0 || recent), "null recent list");
    if ((rc = mm_use_current_device())) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = g_mm.ws.reserve(std::max<size_t>(n_recent, 256)))) return rc;
    uint8_t* keep = g_mm.ws.as<uint8_t>();
    if (n_recent)
        hipLaunchKernelGGL(mm_cull_points_kernel, dim3((n_recent + 255) / 256), dim3(256), 0, st, mm_cull(*c), recent, n_recent,
                           cur_kf_id, monocular ? 2 : 3, keep);
    hipLaunchKernelGGL(mm_cull_list_kernel, dim3(1), dim3(64 * MM_CULL_WAVES), 0, st, recent, n_recent, keep, n_recent_out);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbmm_cull_keyframes_device(const orbmm_cull* c, int32_t cur, int32_t monocular, float th_depth, int32_t* culled,
                                           int32_t* n_culled, int32_t* status, void* stream) {
    int rc;
    if ((rc = mm_cull_check(c, true))) return rc;
    ORB_CHECK_ARG(culled && n_culled && status, "null output");
    if ((rc = mm_use_current_device())) return rc;
    if ((rc = g_mm.ws.reserve(4 * cull_scratch_entries(c->n_keyframes, c->conn_cap, MM_CULL_WAVES)))) return rc;
    hipLaunchKernelGGL(mm_cull_keyframes_kernel, dim3(1), dim3(64 * MM_CULL_WAVES), 0, (hipStream_t)stream, mm_cull(*c), cur,
                       monocular, th_depth, culled, n_culled, status, g_mm.ws.as<int32_t>());
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

namespace {

int mm_compact_check(int32_t M, int32_t n_obs, const int32_t* off, const int32_t* kf, const int32_t* idx, int32_t* out_off,
                     int32_t* out_kf, int32_t* out_idx) {
    ORB_CHECK_ARG(M >= 0 && n_obs >= 0, "negative sizes");
    ORB_CHECK_ARG(off && out_off && (n_obs == 0 || (kf && idx && out_kf && out_idx)), "null observation array");
    return ORB_OK;
}

}  // namespace

extern "C" int orbmm_compact_observations_device(int32_t n_mappoints, int32_t n_obs, const int32_t* mp_obs_off,
                                                 const int32_t* mp_obs_kf, const int32_t* mp_obs_idx, int32_t* out_off,
                                                 int32_t* out_kf, int32_t* out_idx, void* stream) {
    int rc;
    if ((rc = mm_compact_check(n_mappoints, n_obs, mp_obs_off, mp_obs_kf, mp_obs_idx, out_off, out_kf, out_idx))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int M = n_mappoints;
    const dim3 grid((M + 255) / 256);
    if (M) hipLaunchKernelGGL(mm_compact_count_kernel, grid, dim3(256), 0, st, M, n_obs, mp_obs_off, mp_obs_kf, out_off);
    hipLaunchKernelGGL(mm_compact_scan_kernel, dim3(1), dim3(256), 0, st, M, n_obs, out_off);
    if (M)
        hipLaunchKernelGGL(mm_compact_fill_kernel, grid, dim3(256), 0, st, M, n_obs, mp_obs_off, mp_obs_kf, mp_obs_idx, out_off,
                           out_kf, out_idx);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbmm_cull_map_points(const orbmm_cull* c, int32_t n_recent, int32_t* recent, int32_t cur_kf_id,
                                     int32_t monocular, int32_t* n_recent_out, int device) {
    int rc;
    if ((rc = mm_cull_check(c, false))) return rc;
    ORB_CHECK_ARG(n_recent >= 0, "negative sizes");
    ORB_CHECK_ARG(n_recent_out && (n_recent == 0 || recent), "null recent list");
    if ((rc = mm_cull_check_host(c, false))) return rc;   // before any copy
    if ((rc = check_range(recent, n_recent, 0, c->n_mappoints, "recent entry outside [0, n_mappoints)"))) return rc;
    orbmm_cull d = *c;
    Mirror io;
    mm_cull_add(io, d, false);
    io.add(recent, (size_t)n_recent, true, true); io.add(n_recent_out, 1, false, true);
    return run_host(g_mm, device, io, [&] {
        return orbmm_cull_map_points_device(&d, n_recent, recent, cur_kf_id, monocular, n_recent_out, nullptr);
    });
}

extern "C" int orbmm_cull_keyframes(const orbmm_cull* c, int32_t cur, int32_t monocular, float th_depth, int32_t* culled,
                                    int32_t* n_culled, int32_t* status, int device) {
    int rc;
    if ((rc = mm_cull_check(c, true))) return rc;
    ORB_CHECK_ARG(culled && n_culled && status, "null output");
    if ((rc = mm_cull_check_host(c, true))) return rc;   // before any copy
    ORB_CHECK_ARG(cur >= 0 && cur < c->n_keyframes, "cur outside [0, n_keyframes)");
    orbmm_cull d = *c;
    Mirror io;
    mm_cull_add(io, d, true);
    io.add(culled, (size_t)c->conn_cap, false, true); io.add(n_culled, 1, false, true); io.add(status, 1, false, true);
    return run_host(g_mm, device, io, [&] {
        return orbmm_cull_keyframes_device(&d, cur, monocular, th_depth, culled, n_culled, status, nullptr);
    });
}

extern "C" int orbmm_compact_observations(int32_t n_mappoints, int32_t n_obs, const int32_t* mp_obs_off, const int32_t* mp_obs_kf,
                                          const int32_t* mp_obs_idx, int32_t* out_off, int32_t* out_kf, int32_t* out_idx,
                                          int device) {
    int rc;
    if ((rc = mm_compact_check(n_mappoints, n_obs, mp_obs_off, mp_obs_kf, mp_obs_idx, out_off, out_kf, out_idx))) return rc;
    if ((rc = check_csr(mp_obs_off, n_mappoints, n_obs, "mp_obs"))) return rc;   // before any copy
    const size_t M = n_mappoints, n = n_obs;
    Mirror io;
    io.add(mp_obs_off, M + 1, true, false); io.add(mp_obs_kf, n, true, false); io.add(mp_obs_idx, n, true, false);
    io.add(out_off, M + 1, false, true); io.add(out_kf, n, true, true); io.add(out_idx, n, true, true);
    return run_host(g_mm, device, io, [&] {
        return orbmm_compact_observations_device(n_mappoints, n_obs, mp_obs_off, mp_obs_kf, mp_obs_idx, out_off, out_kf, out_idx,
                                                 nullptr);
    });
}
