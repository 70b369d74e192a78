// Optimizer::LocalBundleAdjustment's window (src/Optimizer.cc:493-631) and its write-back (:677-735) on slot tables:
// what one list entry, one edge and one erasure are.  Compiles for host and device; orbbamap.hip runs the per-element
// rules from its kernels; baw_gather_seq / baw_apply_seq are the same rules one after another for a CPU build, and
// tests/local_ba_window_ref.py restates them in numpy.
//   local keyframes   cur, then ord_slot[cur][0 .. n_ord[cur]) in row order without the bad ones; a bad neighbour is
//                     still marked local (BALocalForKF), so it is never a fixed camera
//   local points      the local keyframes in list order, kf_mappoint[k][0 .. kf_n[k]) in index order: not null, not
//                     bad, first occurrence
//   fixed cameras     the local points in list order, their observations in CSR order without the erased ones: neither
//                     marked local nor marked fixed yet; a bad keyframe is marked, not listed
//   edges             point-major; a point's observations in CSR order without erased entries and bad keyframes
// Departure (the one mm_normal.h and mm_cull.h make): GetObservations() is a std::map<KeyFrame*, size_t> walked in pointer
// order; here that order is the CSR's.  A slot, an offset or an index outside its table is skipped: a neighbour equal to
// cur or met before in the row, an observation whose keypoint index or octave is outside its table (no edge; it still
// marks its keyframe).
#pragma once

#include "mm_cull.h"
#include "mm_normal.h"

namespace orbamd {

constexpr int BAW_OK = 0, BAW_OVERFLOW = 1;   // ORBBA_WINDOW_*
constexpr int BAW_NONE = 0, BAW_LOCAL = 1;
// counts: n_local, n_fixed, n_points, n_edges, status, one camera for every edge
constexpr int BAW_N_LOCAL = 0, BAW_N_FIXED = 1, BAW_N_POINTS = 2, BAW_N_EDGES = 3, BAW_STATUS = 4, BAW_ONE_CAM = 5, BAW_COUNTS = 8;

struct BaKeypoint {   // orbx_keypoint
    float x, y, size, angle, response;
    int32_t octave, class_id;
};

struct BaMap {
    int K, M, kf_cap, conn_cap, n_obs, n_levels;
    const int32_t* kf_id;
    const int32_t* kf_n;
    const uint8_t* kf_bad;
    int32_t* kf_mappoint;
    const BaKeypoint* kf_keypoint;
    const float* kf_uright;
    const float* kf_camera;   // [K][6]
    float* kf_pose;
    const int32_t* ord_slot;
    const int32_t* n_ord;
    uint8_t* mp_bad;
    float* mp_xw;
    int32_t* mp_nobs;
    int32_t* mp_ref_kf;
    const int32_t* mp_obs_off;
    int32_t* mp_obs_kf;
    const int32_t* mp_obs_idx;
    float inv_sigma2[MM_MAX_LEVELS];
};

struct BaWindow {
    int cap_poses, cap_points, cap_edges;
    int32_t* counts;       // BAW_COUNTS
    int32_t* pose_kf;      // keyframe slot per vertex: local, then fixed
    uint8_t* pose_fixed;
    int32_t* point;        // map-point slot per point vertex
    int32_t *edge_point, *edge_pose, *edge_kf, *edge_idx;
    float* edge_obs;       // x 3: u, v, ur
    float* edge_inv_sigma2;
    float* edge_cam;       // x 5: fx, fy, cx, cy, bf
};

// entry i of cur's ordered row as a neighbour, or -1
MM_HD int baw_neighbour(const BaMap& t, int cur, int i) {
    if (i >= mm_clamp(t.n_ord[cur], 0, t.conn_cap)) return -1;
    const int s = t.ord_slot[(size_t)cur * t.conn_cap + i];
    return (s >= 0 && s < t.K && s != cur) ? s : -1;
}

// entry i of keyframe k's row as a local-point candidate (:510-513), or -1
MM_HD int baw_row_point(const BaMap& t, int k, int i) {
    if (i >= mm_clamp(t.kf_n[k], 0, t.kf_cap)) return -1;
    const int p = t.kf_mappoint[(size_t)k * t.kf_cap + i];
    return (p >= 0 && p < t.M && !t.mp_bad[p]) ? p : -1;
}

MM_HD void baw_obs_range(const BaMap& t, int p, int& e0, int& e1) {
    e0 = t.mp_obs_off[p];
    e1 = t.mp_obs_off[p + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > t.n_obs) e1 = t.n_obs;
}

// the keyframe of observation e as :527-536 walk it (erased entries are not in the map), or -1
MM_HD int baw_observer(const BaMap& t, int e) {
    const int o = t.mp_obs_kf[e];
    return (o >= 0 && o < t.K) ? o : -1;
}

// does observation e give an edge (:583-588)
MM_HD bool baw_is_edge(const BaMap& t, int e) {
    const int o = baw_observer(t, e), idx = t.mp_obs_idx[e];
    if (o < 0 || t.kf_bad[o] || idx < 0 || idx >= t.kf_cap) return false;
    const int octave = t.kf_keypoint[(size_t)o * t.kf_cap + idx].octave;
    return octave >= 0 && octave < t.n_levels;
}

// The edge of observation e at position at of the window (:590-629).  Returns whether its camera is cam0's, bit for bit.
MM_HD bool baw_edge_record(const BaMap& t, const BaWindow& w, int at, int e, int point_index, int vertex, const float* cam0) {
    const int o = t.mp_obs_kf[e], idx = t.mp_obs_idx[e];
    const BaKeypoint& kp = t.kf_keypoint[(size_t)o * t.kf_cap + idx];
    w.edge_point[at] = point_index;
    w.edge_pose[at] = vertex;
    w.edge_kf[at] = o;
    w.edge_idx[at] = idx;
    w.edge_obs[3 * (size_t)at] = kp.x;
    w.edge_obs[3 * (size_t)at + 1] = kp.y;
    w.edge_obs[3 * (size_t)at + 2] = t.kf_uright[(size_t)o * t.kf_cap + idx];
    w.edge_inv_sigma2[at] = t.inv_sigma2[kp.octave];
    bool same = true;
    for (int i = 0; i < 5; i++) {
        const float c = t.kf_camera[6 * (size_t)o + i];
        w.edge_cam[5 * (size_t)at + i] = c;
        same = same && c == cam0[i];
    }
    return same;
}

MM_HD MmCull baw_cull_tables(const BaMap& t) {
    MmCull c{};
    c.K = t.K; c.M = t.M; c.kf_cap = t.kf_cap; c.conn_cap = t.conn_cap; c.n_obs = t.n_obs;
    c.kf_mappoint = t.kf_mappoint; c.kf_uright = t.kf_uright; c.mp_bad = t.mp_bad; c.mp_nobs = t.mp_nobs;
    c.mp_ref_kf = t.mp_ref_kf; c.mp_obs_off = t.mp_obs_off; c.mp_obs_kf = t.mp_obs_kf; c.mp_obs_idx = t.mp_obs_idx;
    return c;
}

// One entry of toErase (:709-715): EraseMapPointMatch(point) clears the cell GetIndexInKeyFrame names, EraseObservation
// follows.  A point that has gone bad observes nothing any more, so both do nothing.  One lane.
MM_HD void baw_erase(const BaMap& t, int p, int k) {
    if (p < 0 || p >= t.M || k < 0 || k >= t.K) return;
    int e0, e1, at = -1;
    baw_obs_range(t, p, e0, e1);
    for (int e = e0; e < e1 && at < 0; e++)
        if (t.mp_obs_kf[e] == k) at = e;
    if (at < 0) return;
    const int idx = t.mp_obs_idx[at];
    if (idx >= 0 && idx < t.kf_cap) t.kf_mappoint[(size_t)k * t.kf_cap + idx] = -1;
    cull_erase_observation(baw_cull_tables(t), p, k);
}

// The erasures of the edges [e, ..) of one point, in edge order; e is the point's first edge.  One lane.
MM_HD void baw_erase_point(const BaMap& t, const BaWindow& w, int n_points, int n_edges, const uint8_t* outlier, int e) {
    const int j = w.edge_point[e];
    if (j < 0 || j >= n_points) return;
    const int p = w.point[j];
    for (int f = e; f < n_edges && w.edge_point[f] == j; f++)
        if (outlier[f]) baw_erase(t, p, w.edge_kf[f]);
}

// FromSE3Quat / FromVector3d (:725, :733): the estimates narrowed element by element
MM_HD void baw_store_pose(const BaMap& t, int k, const double* R, const double* tr) {
    if (k < 0 || k >= t.K) return;
    for (int i = 0; i < 9; i++) t.kf_pose[12 * (size_t)k + i] = (float)R[i];
    for (int i = 0; i < 3; i++) t.kf_pose[12 * (size_t)k + 9 + i] = (float)tr[i];
}
MM_HD void baw_store_point(const BaMap& t, int p, const double* X) {
    if (p < 0 || p >= t.M) return;
    for (int i = 0; i < 3; i++) t.mp_xw[3 * (size_t)p + i] = (float)X[i];
}

#if !defined(__HIP_DEVICE_COMPILE__)
// Scratch of baw_gather_seq: mark, vertex and list_fixed K entries, seen and list_pt M, list_kf conn_cap + 1.
struct BaSeqScratch {
    int32_t *mark, *vertex, *seen, *list_kf, *list_pt, *list_fixed;
};

// The whole gather, one entry after another.  Returns the status; on BAW_OVERFLOW only counts is written.
inline int baw_gather_seq(const BaMap& t, int cur, const BaWindow& w, const BaSeqScratch& s) {
    for (int i = 0; i < BAW_COUNTS; i++) w.counts[i] = 0;
    w.counts[BAW_ONE_CAM] = 1;
    if (cur < 0 || cur >= t.K) return BAW_OK;
    for (int k = 0; k < t.K; k++) s.mark[k] = BAW_NONE, s.vertex[k] = -1;
    for (int p = 0; p < t.M; p++) s.seen[p] = 0;
    int n_local = 0, n_points = 0, n_fixed = 0, n_edges = 0;
    s.mark[cur] = BAW_LOCAL;
    s.list_kf[n_local++] = cur;
    for (int i = 0; i < t.conn_cap; i++) {
        const int nb = baw_neighbour(t, cur, i);
        if (nb < 0 || s.mark[nb] != BAW_NONE) continue;
        s.mark[nb] = BAW_LOCAL;
        if (!t.kf_bad[nb]) s.list_kf[n_local++] = nb;
    }
    for (int j = 0; j < n_local; j++)
        for (int i = 0; i < t.kf_cap; i++) {
            const int p = baw_row_point(t, s.list_kf[j], i);
            if (p < 0 || s.seen[p]) continue;
            s.seen[p] = 1;
            s.list_pt[n_points++] = p;
        }
    for (int j = 0; j < n_points; j++) {
        int e0, e1;
        baw_obs_range(t, s.list_pt[j], e0, e1);
        for (int e = e0; e < e1; e++) {
            if (baw_is_edge(t, e)) n_edges++;
            const int o = baw_observer(t, e);
            if (o < 0 || s.mark[o] != BAW_NONE) continue;
            s.mark[o] = BAW_LOCAL + 1;   // BAFixedForKF
            if (!t.kf_bad[o]) s.list_fixed[n_fixed++] = o;
        }
    }
    w.counts[BAW_N_LOCAL] = n_local; w.counts[BAW_N_FIXED] = n_fixed; w.counts[BAW_N_POINTS] = n_points;
    w.counts[BAW_N_EDGES] = n_edges;
    if (n_local + n_fixed > w.cap_poses || n_points > w.cap_points || n_edges > w.cap_edges)
        return w.counts[BAW_STATUS] = BAW_OVERFLOW;
    for (int i = 0; i < n_local + n_fixed; i++) {
        const int k = i < n_local ? s.list_kf[i] : s.list_fixed[i - n_local];
        s.vertex[k] = i;
        w.pose_kf[i] = k;
        w.pose_fixed[i] = i < n_local ? t.kf_id[k] == 0 : 1;
    }
    bool one_cam = true;
    int at = 0;
    for (int j = 0; j < n_points; j++) {
        w.point[j] = s.list_pt[j];
        int e0, e1;
        baw_obs_range(t, s.list_pt[j], e0, e1);
        for (int e = e0; e < e1; e++)
            if (baw_is_edge(t, e)) {
                one_cam = baw_edge_record(t, w, at, e, j, s.vertex[t.mp_obs_kf[e]], t.kf_camera + 6 * (size_t)cur) && one_cam;
                at++;
            }
    }
    w.counts[BAW_ONE_CAM] = one_cam ? 1 : 0;
    return BAW_OK;
}

// The write-back but for UpdateNormalAndDepth (mm_normal.h's, over w.point): erasures in edge order, then poses and
// points.  pose_R x 9, pose_t x 3 per vertex, points x 3 per point vertex.
inline void baw_apply_seq(const BaMap& t, const BaWindow& w, const uint8_t* outlier, const double* pose_R, const double* pose_t,
                          const double* points) {
    if (w.counts[BAW_STATUS] != BAW_OK) return;
    const int n_local = w.counts[BAW_N_LOCAL], n_points = w.counts[BAW_N_POINTS], n_edges = w.counts[BAW_N_EDGES];
    for (int e = 0; e < n_edges; e++)
        if (e == 0 || w.edge_point[e - 1] != w.edge_point[e]) baw_erase_point(t, w, n_points, n_edges, outlier, e);
    for (int i = 0; i < n_local; i++) baw_store_pose(t, w.pose_kf[i], pose_R + 9 * (size_t)i, pose_t + 3 * (size_t)i);
    for (int j = 0; j < n_points; j++) baw_store_point(t, w.point[j], points + 3 * (size_t)j);
}
#endif

// LocalBA on a gathered window in HBM (orbba.hip's second staging path), between orbbamap.hip's gather and apply.
struct BaWindowRun {
    BaWindow w;                // device arrays
    int K, M;
    const float* kf_pose;      // device
    const float* mp_xw;        // device
    int n_local, n_fixed, n_points, n_edges;   // the window's counts, on the host
    bool one_cam;
    // out: the final classification and estimates in HBM, in the window's order (the calling thread's buffers)
    const uint8_t* outlier;
    const double *pose_R, *pose_t, *points;
    int32_t iterations[2];
    double chi2[2];
    int32_t ran;
};
int orbba_run_window(BaWindowRun& r, const volatile int32_t* stop_flag, void* stream);

}  // namespace orbamd
