// orbbamap.hip — Optimizer::LocalBundleAdjustment on the device-resident map (include/orbslam2_amd.h, "LocalBundleAdjustment
// ... as a whole"; the rules are csrc/ba_window.h's).  The lane groups and the scan are csrc/mm_groups.h's.
//   baw_init_kernel     grid: the per-slot "first position" words, marks and vertex indices of the workspace
//   baw_lists_kernel    one workgroup: the three lists in the sequential order.  Per list the candidates put their
//                       position into their slot's word with an integer atomicMin (the minimum does not depend on the
//                       order the lanes run in), a barrier, then flag = "my position is my slot's word", scan and a
//                       stable compaction.  The local keyframes take positions in cur's row, the local points (list
//                       index of the keyframe, index in its row), the fixed cameras the running count of live
//                       observations over the local points (one lane per point walks its CSR row; an exclusive scan of
//                       the per-point counts gives each row its base).  The per-point edge counts are scanned the same
//                       way.  Everything goes to the workspace; the window gets the counts and the status.
//   baw_emit_kernel     grid, only when everything fits: vertices, points and one lane per point for its edges
//   baw_erase_kernel    grid, one lane per point (the one on the point's first edge): its outlier edges in order
//   baw_store_kernel    grid: poses and points narrowed into the tables; the point list for UpdateNormalAndDepth
// The LM between gather and write-back is orbba.hip's (orbba_run_window).
#include <algorithm>
#include <vector>

#include "common.h"
#include "ba_window.h"
#include "mm_groups.h"
#include "mm_host.h"

namespace orbamd {

static_assert(sizeof(BaKeypoint) == sizeof(orbx_keypoint), "BaKeypoint is orbx_keypoint");

constexpr int BAW_NO_POS = 0x7fffffff;

struct BaWork {   // the workspace, int32 each
    int32_t* nb_first;    // K: first position in cur's row
    int32_t* kf_first;    // K: first position among the live observations of the local points
    int32_t* kf_mark;     // K: BAW_LOCAL for cur and its neighbours
    int32_t* kf_vertex;   // K: index into local ++ fixed, or -1
    int32_t* pt_first;    // M: first position in the local keyframes' rows
    int32_t* list_kf;     // conn_cap + 1
    int32_t* list_fixed;  // K
    int32_t* list_pt;     // M
    int32_t* pt_walk;     // M + 1: live observations before each local point (+ 1: the in-place scan stores its total)
    int32_t* pt_edge;     // M + 1: edges before each local point
    int32_t* pt_nfix;     // M + 1: fixed cameras first met before each local point
    int32_t* up_point;    // M: the point list UpdateNormalAndDepth takes
    size_t carve(char* base, size_t K, size_t M, size_t conn_cap) {
        Carver c{base};
        c.take(nb_first, K); c.take(kf_first, K); c.take(kf_mark, K); c.take(kf_vertex, K); c.take(pt_first, M);
        c.take(list_kf, conn_cap + 1); c.take(list_fixed, K); c.take(list_pt, M); c.take(pt_walk, M + 1);
        c.take(pt_edge, M + 1); c.take(pt_nfix, M + 1); c.take(up_point, M);
        return c.off;
    }
};

__global__ __launch_bounds__(256) void baw_init_kernel(BaWork s, int K, int M) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < K) {
        s.nb_first[i] = s.kf_first[i] = BAW_NO_POS;
        s.kf_mark[i] = BAW_NONE;
        s.kf_vertex[i] = -1;
    }
    if (i < M) s.pt_first[i] = BAW_NO_POS;
}

// is the observer o of a local point, met at walk position pos, a fixed camera's first occurrence
__device__ __forceinline__ bool baw_first_fixed(const BaMap& t, const BaWork& s, int o, int pos) {
    return o >= 0 && s.kf_mark[o] == BAW_NONE && s.kf_first[o] == pos && !t.kf_bad[o];
}

__global__ __launch_bounds__(64 * MM_CULL_WAVES) void baw_lists_kernel(BaMap t, int cur, BaWindow w, BaWork s) {
    __shared__ int32_t s_red[MM_CULL_WAVES];
    const MmBlock b{(int)threadIdx.x, s_red};
    if (cur < 0 || cur >= t.K) {   // uniform
        if (b.lane < BAW_COUNTS) w.counts[b.lane] = b.lane == BAW_ONE_CAM ? 1 : 0;
        return;
    }
    // ---- local keyframes (:496-504)
    for (int i = b.lane; i < t.conn_cap; i += b.width) {
        const int nb = baw_neighbour(t, cur, i);
        if (nb >= 0) atomicMin(&s.nb_first[nb], i);
    }
    if (b.lane == 0) {
        s.list_kf[0] = cur;
        s.kf_mark[cur] = BAW_LOCAL;
        s.kf_vertex[cur] = 0;
    }
    b.sync();
    int n_local = 1;
    for (int base = 0; base < t.conn_cap; base += b.width) {   // uniform trip count
        const int i = base + b.lane;
        const int nb = i < t.conn_cap ? baw_neighbour(t, cur, i) : -1;
        const bool first = nb >= 0 && s.nb_first[nb] == i;
        if (first) s.kf_mark[nb] = BAW_LOCAL;   // a bad neighbour too
        const bool flag = first && !t.kf_bad[nb];
        int total;
        const int off = b.prefix(flag, total);
        if (flag) {
            s.list_kf[n_local + off] = nb;
            s.kf_vertex[nb] = n_local + off;
        }
        n_local += total;
    }
    b.sync();
    // ---- local points (:507-521): position = list index of the keyframe * kf_cap + index in its row
    for (int j = 0; j < n_local; j++) {
        const int k = s.list_kf[j];
        for (int i = b.lane; i < t.kf_cap; i += b.width) {
            const int p = baw_row_point(t, k, i);
            if (p >= 0) atomicMin(&s.pt_first[p], j * t.kf_cap + i);
        }
    }
    b.sync();
    int n_points = 0;
    for (int j = 0; j < n_local; j++) {
        const int k = s.list_kf[j];
        for (int base = 0; base < t.kf_cap; base += b.width) {
            const int i = base + b.lane;
            const int p = i < t.kf_cap ? baw_row_point(t, k, i) : -1;
            const bool flag = p >= 0 && s.pt_first[p] == j * t.kf_cap + i;
            int total;
            const int off = b.prefix(flag, total);
            if (flag) s.list_pt[n_points + off] = p;
            n_points += total;
        }
    }
    b.sync();
    // ---- per point: live observations and edges, then their exclusive scans
    for (int j = b.lane; j < n_points; j += b.width) {
        int e0, e1, n_walk = 0, n_edge = 0;
        baw_obs_range(t, s.list_pt[j], e0, e1);
        for (int e = e0; e < e1; e++) {
            n_walk += baw_observer(t, e) >= 0 ? 1 : 0;
            n_edge += baw_is_edge(t, e) ? 1 : 0;
        }
        s.pt_walk[j] = n_walk;
        s.pt_edge[j] = n_edge;
    }
    b.sync();
    mm_block_scan<int>(s.pt_walk, n_points, s.pt_walk, 0, BAW_NO_POS, 0);
    b.sync();
    const int n_edges = mm_block_scan<int>(s.pt_edge, n_points, s.pt_edge, 0, BAW_NO_POS, 0);
    b.sync();
    // ---- fixed cameras (:524-537): position = the count of live observations walked before
    for (int j = b.lane; j < n_points; j += b.width) {
        int e0, e1, pos = s.pt_walk[j];
        baw_obs_range(t, s.list_pt[j], e0, e1);
        for (int e = e0; e < e1; e++) {
            const int o = baw_observer(t, e);
            if (o < 0) continue;
            if (s.kf_mark[o] == BAW_NONE) atomicMin(&s.kf_first[o], pos);
            pos++;
        }
    }
    b.sync();
    for (int j = b.lane; j < n_points; j += b.width) {
        int e0, e1, pos = s.pt_walk[j], n = 0;
        baw_obs_range(t, s.list_pt[j], e0, e1);
        for (int e = e0; e < e1; e++) {
            const int o = baw_observer(t, e);
            if (o < 0) continue;
            n += baw_first_fixed(t, s, o, pos) ? 1 : 0;
            pos++;
        }
        s.pt_nfix[j] = n;
    }
    b.sync();
    const int n_fixed = mm_block_scan<int>(s.pt_nfix, n_points, s.pt_nfix, 0, BAW_NO_POS, 0);
    b.sync();
    for (int j = b.lane; j < n_points; j += b.width) {
        int e0, e1, pos = s.pt_walk[j], at = s.pt_nfix[j];
        baw_obs_range(t, s.list_pt[j], e0, e1);
        for (int e = e0; e < e1; e++) {
            const int o = baw_observer(t, e);
            if (o < 0) continue;
            if (baw_first_fixed(t, s, o, pos)) {
                if (at >= 0 && at < t.K) {   // (offsets that overlap can wrap the 32-bit positions)
                    s.list_fixed[at] = o;
                    s.kf_vertex[o] = n_local + at;
                }
                at++;
            }
            pos++;
        }
    }
    if (b.lane == 0) {
        w.counts[BAW_N_LOCAL] = n_local;
        w.counts[BAW_N_FIXED] = n_fixed;
        w.counts[BAW_N_POINTS] = n_points;
        w.counts[BAW_N_EDGES] = n_edges;
        w.counts[BAW_STATUS] = (n_local + n_fixed > w.cap_poses || n_points > w.cap_points || n_edges > w.cap_edges) ? BAW_OVERFLOW : BAW_OK;
        w.counts[BAW_ONE_CAM] = 1;
        w.counts[6] = w.counts[7] = 0;
    }
}

__global__ __launch_bounds__(256) void baw_emit_kernel(BaMap t, int cur, BaWindow w, BaWork s) {
    if (cur < 0 || cur >= t.K || w.counts[BAW_STATUS] != BAW_OK) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n_local = w.counts[BAW_N_LOCAL], n_fixed = w.counts[BAW_N_FIXED], n_points = w.counts[BAW_N_POINTS];
    if (i < n_local + n_fixed && i < w.cap_poses) {
        const int k = i < n_local ? s.list_kf[i] : s.list_fixed[i - n_local];
        w.pose_kf[i] = k;
        w.pose_fixed[i] = i < n_local ? t.kf_id[k] == 0 : 1;
    }
    if (i < n_points && i < w.cap_points) {
        const int p = s.list_pt[i];
        w.point[i] = p;
        int e0, e1, at = s.pt_edge[i];
        baw_obs_range(t, p, e0, e1);
        bool one_cam = true;
        for (int e = e0; e < e1; e++) {
            if (!baw_is_edge(t, e) || at < 0 || at >= w.cap_edges) continue;
            one_cam = baw_edge_record(t, w, at, e, i, s.kf_vertex[t.mp_obs_kf[e]], t.kf_camera + 6 * (size_t)cur) && one_cam;
            at++;
        }
        if (!one_cam) atomicAnd(&w.counts[BAW_ONE_CAM], 0);
    }
}

__global__ __launch_bounds__(256) void baw_erase_kernel(BaMap t, BaWindow w, const uint8_t* outlier) {
    if (w.counts[BAW_STATUS] != BAW_OK) return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    const int n_points = ::min(w.counts[BAW_N_POINTS], w.cap_points), n_edges = ::min(w.counts[BAW_N_EDGES], w.cap_edges);
    if (e >= n_edges) return;
    if (e == 0 || w.edge_point[e - 1] != w.edge_point[e]) baw_erase_point(t, w, n_points, n_edges, outlier, e);
}

__global__ __launch_bounds__(256) void baw_store_kernel(BaMap t, BaWindow w, const double* pose_R, const double* pose_t,
                                                        const double* points, int32_t* up_point) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool ok = w.counts[BAW_STATUS] == BAW_OK;
    const int n_local = ok ? ::min(w.counts[BAW_N_LOCAL], w.cap_poses) : 0, n_points = ok ? ::min(w.counts[BAW_N_POINTS], w.cap_points) : 0;
    if (i < n_local) baw_store_pose(t, w.pose_kf[i], pose_R + 9 * (size_t)i, pose_t + 3 * (size_t)i);
    if (i < n_points) baw_store_point(t, w.point[i], points + 3 * (size_t)i);
    if (i < w.cap_points) up_point[i] = i < n_points ? w.point[i] : -1;
}

}  // namespace orbamd

using namespace orbamd;

namespace {

struct BawScratch : Scratch {
    DevBuf window;   // orbba_local_ba_map's window
protected:
    void device_changed() override { window.release(); }
};
thread_local BawScratch g_baw;

BaMap baw_map(const orbba_window_map& m) {
    BaMap t{};
    t.K = m.n_keyframes; t.M = m.n_mappoints; t.kf_cap = m.kf_cap; t.conn_cap = m.conn_cap; t.n_obs = m.n_obs; t.n_levels = m.n_levels;
    t.kf_id = m.kf_id; t.kf_n = m.kf_n; t.kf_bad = m.kf_bad; t.kf_mappoint = m.kf_mappoint;
    t.kf_keypoint = reinterpret_cast<const BaKeypoint*>(m.kf_keypoint); t.kf_uright = m.kf_uright; t.kf_camera = m.kf_camera;
    t.kf_pose = m.kf_pose; t.ord_slot = m.ord_slot; t.n_ord = m.n_ord; t.mp_bad = m.mp_bad; t.mp_xw = m.mp_xw; t.mp_nobs = m.mp_nobs;
    t.mp_ref_kf = m.mp_ref_kf; t.mp_obs_off = m.mp_obs_off; t.mp_obs_kf = m.mp_obs_kf; t.mp_obs_idx = m.mp_obs_idx;
    for (int l = 0; l < m.n_levels; l++) t.inv_sigma2[l] = m.inv_sigma2[l];
    return t;
}

BaWindow baw_window(const orbba_window& w) {
    return BaWindow{w.cap_poses, w.cap_points, w.cap_edges, w.counts, w.pose_kf, w.pose_fixed, w.point, w.edge_point,
                    w.edge_pose, w.edge_kf, w.edge_idx, w.edge_obs, w.edge_inv_sigma2, w.edge_cam};
}

constexpr int BAW_GATHER = 1, BAW_APPLY = 2;

int baw_check(const orbba_window_map* m, const orbba_window* w, int parts) {
    ORB_CHECK_ARG(m && w, "null argument");
    ORB_CHECK_ARG(m->n_keyframes >= 0 && m->n_mappoints >= 0 && m->n_obs >= 0, "negative sizes");
    ORB_CHECK_ARG(m->kf_cap >= 1 && m->conn_cap >= 1, "kf_cap and conn_cap must be at least 1");
    ORB_CHECK_ARG(m->n_levels >= 1 && m->n_levels <= MM_MAX_LEVELS, "n_levels must be in [1, 32]");
    ORB_CHECK_ARG((long long)m->n_keyframes * m->kf_cap < MM_MAX_ENTRIES && (long long)m->n_keyframes * m->conn_cap < MM_MAX_ENTRIES &&
                      ((long long)m->conn_cap + 1) * m->kf_cap < MM_MAX_ENTRIES && 3LL * m->n_mappoints < MM_MAX_ENTRIES &&
                      12LL * m->n_keyframes < MM_MAX_ENTRIES,
                  "a table of 2^31 entries or more");
    ORB_CHECK_ARG(m->inv_sigma2, "null inv_sigma2");
    ORB_CHECK_ARG(m->kf_id && m->kf_n && m->kf_bad && m->kf_mappoint && m->kf_keypoint && m->kf_uright && m->kf_camera && m->ord_slot &&
                      m->n_ord,
                  "null keyframe table");
    ORB_CHECK_ARG(m->mp_bad && m->mp_obs_off && m->mp_obs_kf && m->mp_obs_idx, "null map-point table");
    if (parts & BAW_APPLY) {
        ORB_CHECK_ARG(m->scale_factors, "null scale_factors");
        ORB_CHECK_ARG(m->kf_kp_octave && m->kf_pose, "null keyframe table");
        ORB_CHECK_ARG(m->mp_xw && m->mp_nobs && m->mp_ref_kf && m->mp_normal && m->mp_max_min, "null map-point table");
    }
    ORB_CHECK_ARG(w->cap_poses >= 0 && w->cap_points >= 0 && w->cap_edges >= 0, "negative capacities");
    ORB_CHECK_ARG(5LL * w->cap_edges < MM_MAX_ENTRIES && 9LL * w->cap_poses < MM_MAX_ENTRIES && 3LL * w->cap_points < MM_MAX_ENTRIES,
                  "a window of 2^31 entries or more");
    ORB_CHECK_ARG(w->counts && (w->cap_poses == 0 || (w->pose_kf && w->pose_fixed)) && (w->cap_points == 0 || w->point), "null window array");
    ORB_CHECK_ARG(w->cap_edges == 0 || (w->edge_point && w->edge_pose && w->edge_kf && w->edge_idx && w->edge_obs && w->edge_inv_sigma2 &&
                                        w->edge_cam),
                  "null window array");
    return ORB_OK;
}

// The host entries' checks of the tables.
int baw_check_host(const orbba_window_map* m, int cur, bool has_cur, int parts) {
    const int K = m->n_keyframes, M = m->n_mappoints;
    int rc;
    ORB_CHECK_ARG(!has_cur || (cur >= 0 && cur < K), "cur outside [0, n_keyframes)");
    if ((rc = check_csr(m->mp_obs_off, M, m->n_obs, "mp_obs"))) return rc;
    if ((rc = check_range(m->kf_n, K, 0, m->kf_cap + 1, "kf_n outside [0, kf_cap]"))) return rc;
    if ((rc = check_range(m->kf_mappoint, (size_t)K * m->kf_cap, -1, M, "kf_mappoint entry outside [-1, n_mappoints)"))) return rc;
    if ((rc = check_range(m->n_ord, K, 0, m->conn_cap + 1, "n_ord outside [0, conn_cap]"))) return rc;
    for (int k = 0; k < K; k++)
        if ((rc = check_range(m->ord_slot + (size_t)k * m->conn_cap, m->n_ord[k], 0, K, "ord_slot entry outside [0, n_keyframes)"))) return rc;
    if ((parts & BAW_APPLY) && (rc = check_range(m->mp_ref_kf, M, -1, K, "mp_ref_kf outside [-1, n_keyframes)"))) return rc;
    std::vector<int32_t> seen(K, -1);
    for (int p = 0; p < M; p++)
        for (int e = m->mp_obs_off[p]; e < m->mp_obs_off[p + 1]; e++) {
            const int k = m->mp_obs_kf[e], idx = m->mp_obs_idx[e];
            if (k == -1) continue;
            ORB_CHECK_ARG(k >= 0 && k < K, "mp_obs_kf entry outside [-1, n_keyframes)");
            ORB_CHECK_ARG(idx >= 0 && idx < m->kf_cap, "mp_obs_idx entry outside [0, kf_cap)");
            const int octave = m->kf_keypoint[(size_t)k * m->kf_cap + idx].octave;
            ORB_CHECK_ARG(octave >= 0 && octave < m->n_levels, "the octave of an observed keypoint is outside [0, n_levels)");
            ORB_CHECK_ARG(seen[k] != p, "a keyframe twice in a map point's observations");
            seen[k] = p;
        }
    return mm_check_rows_distinct(K, M, m->kf_cap, m->kf_n, m->kf_mappoint);
}

int baw_check_window_host(const orbba_window_map* m, const orbba_window* w) {
    const int32_t* c = w->counts;
    ORB_CHECK_ARG(c[BAW_STATUS] == BAW_OK || c[BAW_STATUS] == BAW_OVERFLOW, "unknown window status");
    if (c[BAW_STATUS] != BAW_OK) return ORB_OK;
    ORB_CHECK_ARG(c[0] >= 0 && c[1] >= 0 && c[2] >= 0 && c[3] >= 0 && (long long)c[0] + c[1] <= w->cap_poses && c[2] <= w->cap_points &&
                      c[3] <= w->cap_edges,
                  "window counts outside the capacities");
    int rc;
    if ((rc = check_range(w->pose_kf, (size_t)c[0] + c[1], 0, m->n_keyframes, "pose_kf outside [0, n_keyframes)"))) return rc;
    if ((rc = check_range(w->point, c[2], 0, m->n_mappoints, "point outside [0, n_mappoints)"))) return rc;
    if ((rc = check_range(w->edge_point, c[3], 0, c[2], "edge_point outside [0, n_points)"))) return rc;
    if ((rc = check_range(w->edge_pose, c[3], 0, c[0] + c[1], "edge_pose outside [0, n_poses)"))) return rc;
    if ((rc = check_range(w->edge_kf, c[3], 0, m->n_keyframes, "edge_kf outside [0, n_keyframes)"))) return rc;
    return check_range(w->edge_idx, c[3], 0, m->kf_cap, "edge_idx outside [0, kf_cap)");
}

int baw_workspace(const orbba_window_map* m, BaWork& s) {
    int rc;
    if ((rc = g_baw.use_current_device())) return rc;
    const size_t K = m->n_keyframes, M = m->n_mappoints, cap = m->conn_cap;
    if ((rc = g_baw.ws.reserve(s.carve(nullptr, K, M, cap)))) return rc;
    s.carve(g_baw.ws.as<char>(), K, M, cap);
    return ORB_OK;
}

void baw_add_map(Mirror& io, orbba_window_map& d, int parts) {
    const size_t K = d.n_keyframes, M = d.n_mappoints, n_obs = d.n_obs, rows = K * d.kf_cap;
    const bool ap = (parts & BAW_APPLY) != 0;
    io.add(d.kf_id, K, true, false); io.add(d.kf_n, K, true, false); io.add(d.kf_bad, K, true, false);
    io.add(d.kf_mappoint, rows, true, ap); io.add(d.kf_keypoint, rows, true, false); io.add(d.kf_kp_octave, rows, true, false);
    io.add(d.kf_uright, rows, true, false); io.add(d.kf_camera, K * 6, true, false); io.add(d.kf_pose, K * 12, true, ap);
    io.add(d.ord_slot, K * d.conn_cap, true, false); io.add(d.n_ord, K, true, false);
    io.add(d.mp_bad, M, true, ap); io.add(d.mp_xw, M * 3, true, ap); io.add(d.mp_nobs, M, true, ap); io.add(d.mp_ref_kf, M, true, ap);
    io.add(d.mp_obs_off, M + 1, true, false); io.add(d.mp_obs_kf, n_obs, true, ap); io.add(d.mp_obs_idx, n_obs, true, false);
    io.add(d.mp_normal, M * 3, true, ap); io.add(d.mp_max_min, M * 2, true, ap);
}

void baw_add_window(Mirror& io, orbba_window& w, bool in, bool out) {
    const size_t P = w.cap_poses, N = w.cap_points, E = w.cap_edges;
    io.add(w.counts, BAW_COUNTS, in, out); io.add(w.pose_kf, P, true, out); io.add(w.pose_fixed, P, true, out);
    io.add(w.point, N, true, out); io.add(w.edge_point, E, true, out); io.add(w.edge_pose, E, true, out);
    io.add(w.edge_kf, E, true, out); io.add(w.edge_idx, E, true, out); io.add(w.edge_obs, 3 * E, true, out);
    io.add(w.edge_inv_sigma2, E, true, out); io.add(w.edge_cam, 5 * E, true, out);
}

}  // namespace

extern "C" int orbba_local_window_device(const orbba_window_map* m, int32_t cur, const orbba_window* w, void* stream) {
    int rc;
    if ((rc = baw_check(m, w, BAW_GATHER))) return rc;
    BaWork s;
    if ((rc = baw_workspace(m, s))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const BaMap t = baw_map(*m);
    const BaWindow bw = baw_window(*w);
    const int n_init = std::max(std::max(t.K, t.M), 1), n_emit = std::max(std::max(w->cap_poses, w->cap_points), 1);
    hipLaunchKernelGGL(baw_init_kernel, dim3((n_init + 255) / 256), dim3(256), 0, st, s, t.K, t.M);
    hipLaunchKernelGGL(baw_lists_kernel, dim3(1), dim3(64 * MM_CULL_WAVES), 0, st, t, cur, bw, s);
    hipLaunchKernelGGL(baw_emit_kernel, dim3((n_emit + 255) / 256), dim3(256), 0, st, t, cur, bw, s);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbba_local_ba_apply_device(const orbba_window_map* m, const orbba_window* w, const uint8_t* outlier,
                                           const double* pose_R, const double* pose_t, const double* points, void* stream) {
    int rc;
    if ((rc = baw_check(m, w, BAW_APPLY))) return rc;
    ORB_CHECK_ARG((w->cap_edges == 0 || outlier) && (w->cap_poses == 0 || (pose_R && pose_t)) && (w->cap_points == 0 || points),
                  "null estimates");
    BaWork s;
    if ((rc = baw_workspace(m, s))) return rc;
    hipStream_t st = (hipStream_t)stream;
    const BaMap t = baw_map(*m);
    const BaWindow bw = baw_window(*w);
    if (w->cap_edges) hipLaunchKernelGGL(baw_erase_kernel, dim3((w->cap_edges + 255) / 256), dim3(256), 0, st, t, bw, outlier);
    const int n_store = std::max(w->cap_poses, w->cap_points);
    if (n_store)
        hipLaunchKernelGGL(baw_store_kernel, dim3((n_store + 255) / 256), dim3(256), 0, st, t, bw, pose_R, pose_t, points, s.up_point);
    ORB_HIP_TRY(hipGetLastError());
    // UpdateNormalAndDepth over the local points (:734); a list entry of -1 and a bad point are left as they are
    const int n_up = std::min(w->cap_points, m->n_mappoints);   // (the list holds distinct points)
    orbmm_points up{};
    up.n_keyframes = m->n_keyframes; up.n_mappoints = m->n_mappoints; up.kf_cap = m->kf_cap; up.n_obs = m->n_obs; up.n_levels = m->n_levels;
    up.scale_factors = m->scale_factors; up.mp_bad = m->mp_bad; up.mp_xw = m->mp_xw; up.mp_ref_kf = m->mp_ref_kf;
    up.mp_obs_off = m->mp_obs_off; up.mp_obs_kf = m->mp_obs_kf; up.mp_obs_idx = m->mp_obs_idx; up.kf_pose = m->kf_pose; up.kf_n = m->kf_n;
    up.kf_kp_octave = m->kf_kp_octave; up.n_points = n_up; up.point = s.up_point; up.mp_normal = m->mp_normal; up.mp_max_min = m->mp_max_min;
    return orbmm_update_normal_depth_device(&up, stream);
}

extern "C" int orbba_local_ba_map_device(const orbba_window_map* m, int32_t cur, const orbba_window* w, orbba_map_result* res,
                                         const volatile int32_t* stop_flag, void* stream) {
    int rc;
    ORB_CHECK_ARG(res, "null result");
    if ((rc = baw_check(m, w, BAW_GATHER | BAW_APPLY))) return rc;
    *res = orbba_map_result{};
    if ((rc = orbba_local_window_device(m, cur, w, stream))) return rc;
    hipStream_t st = (hipStream_t)stream;
    int32_t c[BAW_COUNTS];
    ORB_HIP_TRY(hipMemcpyAsync(c, w->counts, sizeof c, hipMemcpyDeviceToHost, st));
    ORB_HIP_TRY(hipStreamSynchronize(st));
    for (int i = 0; i < 4; i++) res->counts[i] = c[i];
    res->status = c[BAW_STATUS];
    if (c[BAW_STATUS] != BAW_OK) return ORB_OK;
    BaWindowRun r{};
    r.w = baw_window(*w);
    r.K = m->n_keyframes; r.M = m->n_mappoints;
    r.kf_pose = m->kf_pose; r.mp_xw = m->mp_xw;
    r.n_local = c[BAW_N_LOCAL]; r.n_fixed = c[BAW_N_FIXED]; r.n_points = c[BAW_N_POINTS]; r.n_edges = c[BAW_N_EDGES];
    r.one_cam = c[BAW_ONE_CAM] != 0;
    if ((rc = orbba_run_window(r, stop_flag, stream))) return rc;
    for (int k = 0; k < 2; k++) {
        res->iterations[k] = r.iterations[k];
        res->chi2[k] = r.chi2[k];
    }
    res->ran = r.ran;
    if (!r.ran) return ORB_OK;   // :633-634
    return orbba_local_ba_apply_device(m, w, r.outlier, r.pose_R, r.pose_t, r.points, stream);
}

extern "C" int orbba_local_window(const orbba_window_map* m, int32_t cur, const orbba_window* w, int device) {
    int rc;
    if ((rc = baw_check(m, w, BAW_GATHER))) return rc;
    if ((rc = baw_check_host(m, cur, true, BAW_GATHER))) return rc;   // before any copy
    orbba_window_map d = *m;
    d.kf_kp_octave = nullptr; d.kf_pose = nullptr; d.mp_xw = nullptr; d.mp_nobs = nullptr; d.mp_ref_kf = nullptr;
    d.mp_normal = d.mp_max_min = nullptr;
    orbba_window dw = *w;
    Mirror io;
    baw_add_map(io, d, BAW_GATHER);
    baw_add_window(io, dw, false, true);
    return run_host(g_baw, device, io, [&] { return orbba_local_window_device(&d, cur, &dw, nullptr); });
}

extern "C" int orbba_local_ba_apply(const orbba_window_map* m, const orbba_window* w, const uint8_t* outlier, const double* pose_R,
                                    const double* pose_t, const double* points, int device) {
    int rc;
    if ((rc = baw_check(m, w, BAW_APPLY))) return rc;
    ORB_CHECK_ARG((w->cap_edges == 0 || outlier) && (w->cap_poses == 0 || (pose_R && pose_t)) && (w->cap_points == 0 || points),
                  "null estimates");
    if ((rc = baw_check_host(m, 0, false, BAW_APPLY))) return rc;   // before any copy
    if ((rc = baw_check_window_host(m, w))) return rc;
    orbba_window_map d = *m;
    orbba_window dw = *w;
    Mirror io;
    baw_add_map(io, d, BAW_APPLY);
    baw_add_window(io, dw, true, false);
    const size_t P = w->cap_poses, N = w->cap_points, E = w->cap_edges;
    io.add(outlier, E, true, false); io.add(pose_R, 9 * P, true, false); io.add(pose_t, 3 * P, true, false); io.add(points, 3 * N, true, false);
    return run_host(g_baw, device, io, [&] { return orbba_local_ba_apply_device(&d, &dw, outlier, pose_R, pose_t, points, nullptr); });
}

extern "C" int orbba_local_ba_map(const orbba_window_map* m, int32_t cur, orbba_map_result* res, const volatile int32_t* stop_flag,
                                  int device) {
    int rc;
    ORB_CHECK_ARG(m && res, "null argument");
    orbba_window w{};
    int32_t counts[BAW_COUNTS];
    w.counts = counts;   // the only window array checked for null at capacity 0
    orbba_window probe = w;
    if ((rc = baw_check(m, &probe, BAW_GATHER | BAW_APPLY))) return rc;
    if ((rc = baw_check_host(m, cur, true, BAW_GATHER | BAW_APPLY))) return rc;   // before any copy
    ORB_CHECK_ARG(5LL * m->n_obs < MM_MAX_ENTRIES, "a window of 2^31 entries or more");
    // the window stays on the device: a buffer of this thread's beside the slab the tables are staged in
    ORB_HIP_TRY(hipSetDevice(device));
    if ((rc = g_baw.use_device(device))) return rc;
    const size_t P = m->n_keyframes, N = m->n_mappoints, E = m->n_obs;
    w.cap_poses = (int32_t)P; w.cap_points = (int32_t)N; w.cap_edges = (int32_t)E;
    auto carve = [&](char* base) {
        Carver c{base};
        c.take(w.counts, BAW_COUNTS); c.take(w.pose_kf, P); c.take(w.pose_fixed, P); c.take(w.point, N); c.take(w.edge_point, E);
        c.take(w.edge_pose, E); c.take(w.edge_kf, E); c.take(w.edge_idx, E); c.take(w.edge_obs, 3 * E); c.take(w.edge_inv_sigma2, E);
        c.take(w.edge_cam, 5 * E);
        return c.off;
    };
    if ((rc = g_baw.window.reserve(carve(nullptr)))) return rc;
    carve(g_baw.window.as<char>());
    orbba_window_map d = *m;
    Mirror io;
    baw_add_map(io, d, BAW_GATHER | BAW_APPLY);
    return run_host(g_baw, device, io, [&] { return orbba_local_ba_map_device(&d, cur, &w, res, stop_flag, nullptr); });
}
