// What the host side of orbmm.hip, orbmm_observe.hip and orblc.hip shares: the per-thread buffers and the table checks of
// their host entries (check_csr and check_range are common.h's).
#pragma once
#include <algorithm>
#include <vector>

#include "common.h"
#include "mm_connect.h"
#include "mm_normal.h"

namespace orbamd {

inline thread_local Scratch g_mm;

inline int mm_use_current_device() { return g_mm.use_current_device(); }

constexpr long long MM_MAX_ENTRIES = 0x7fffffffLL;

// The connection rows and the ordered rows of K keyframes, conn_cap entries each.
inline int mm_rows_check_host(int K, int cap, const int32_t* conn_slot, const int32_t* n_conn, const int32_t* ord_slot,
                              const int32_t* n_ord) {
    for (int k = 0; k < K; k++) {
        ORB_CHECK_ARG(n_conn[k] >= 0 && n_conn[k] <= cap, "n_conn outside [0, conn_cap]");
        ORB_CHECK_ARG(n_ord[k] >= 0 && n_ord[k] <= cap, "n_ord outside [0, conn_cap]");
        int rc;
        if ((rc = check_range(conn_slot + (size_t)k * cap, n_conn[k], 0, K, "conn_slot entry outside [0, n_keyframes)"))) return rc;
        if ((rc = check_range(ord_slot + (size_t)k * cap, n_ord[k], 0, K, "ord_slot entry outside [0, n_keyframes)"))) return rc;
    }
    return ORB_OK;
}

// The argument checks of orbmm_update_normal_depth and orbmm_update_connections (orblc.hip runs them on its own map):
// *_check what both forms of an entry check, *_check_host what the host form checks before anything is copied.
inline int mm_points_check(const orbmm_points* p) {
    ORB_CHECK_ARG(p, "null points");
    ORB_CHECK_ARG(p->n_keyframes >= 0 && p->n_mappoints >= 0 && p->n_obs >= 0 && (!p->point || p->n_points >= 0), "negative sizes");
    ORB_CHECK_ARG(p->kf_cap >= 1, "kf_cap must be at least 1");
    ORB_CHECK_ARG(p->n_levels >= 1 && p->n_levels <= MM_MAX_LEVELS, "n_levels must be in [1, 32]");
    ORB_CHECK_ARG((long long)p->n_keyframes * p->kf_cap < MM_MAX_ENTRIES && 3LL * p->n_mappoints < MM_MAX_ENTRIES &&
                      12LL * p->n_keyframes < MM_MAX_ENTRIES,
                  "a table of 2^31 entries or more");
    ORB_CHECK_ARG(p->scale_factors, "null scale_factors");
    ORB_CHECK_ARG(p->mp_bad && p->mp_xw && p->mp_ref_kf && p->mp_obs_off && p->mp_obs_kf && p->mp_obs_idx && p->mp_normal &&
                      p->mp_max_min,
                  "null map-point table");
    ORB_CHECK_ARG(p->kf_pose && p->kf_n && p->kf_kp_octave, "null keyframe table");
    return ORB_OK;
}

inline int mm_points_check_host(const orbmm_points* p) {
    const int K = p->n_keyframes, M = p->n_mappoints;
    int rc;
    if ((rc = check_csr(p->mp_obs_off, M, p->n_obs, "mp_obs"))) return rc;
    const size_t n_obs = p->mp_obs_off[M];
    if ((rc = check_range(p->mp_obs_kf, n_obs, 0, K, "mp_obs_kf entry outside [0, n_keyframes)"))) return rc;
    if ((rc = check_range(p->mp_obs_idx, n_obs, 0, p->kf_cap, "mp_obs_idx entry outside [0, kf_cap)"))) return rc;
    if ((rc = check_range(p->mp_ref_kf, M, -1, K, "mp_ref_kf outside [-1, n_keyframes)"))) return rc;
    if ((rc = check_range(p->kf_n, K, 0, p->kf_cap + 1, "kf_n outside [0, kf_cap]"))) return rc;
    for (int k = 0; k < K; k++)
        if ((rc = check_range(p->kf_kp_octave + (size_t)k * p->kf_cap, p->kf_n[k], 0, p->n_levels,
                                 "kf_kp_octave entry outside [0, n_levels)")))
            return rc;
    if (p->point && (rc = check_range(p->point, p->n_points, 0, M, "point outside [0, n_mappoints)"))) return rc;
    return ORB_OK;
}

inline int mm_graph_check(const orbmm_graph* g, bool rows_only) {
    ORB_CHECK_ARG(g, "null graph");
    ORB_CHECK_ARG(g->n_keyframes >= 0 && g->n_mappoints >= 0 && g->n_obs >= 0, "negative sizes");
    ORB_CHECK_ARG(g->kf_cap >= 1 || rows_only, "kf_cap must be at least 1");
    ORB_CHECK_ARG(g->conn_cap >= 1, "conn_cap must be at least 1");
    ORB_CHECK_ARG((long long)g->n_keyframes * std::max(g->kf_cap, 1) < MM_MAX_ENTRIES &&
                      (long long)g->n_keyframes * g->conn_cap < MM_MAX_ENTRIES / 2,
                  "a table of 2^31 entries or more");
    ORB_CHECK_ARG(g->conn_slot && g->conn_weight && g->n_conn && g->ord_slot && g->ord_weight && g->n_ord, "null row array");
    if (rows_only) return ORB_OK;
    ORB_CHECK_ARG(g->kf_id && g->kf_n && g->kf_mappoint && g->kf_first_connection && g->kf_parent && g->kf_covis && g->status,
                  "null keyframe table");
    ORB_CHECK_ARG(g->mp_bad && g->mp_obs_off && g->mp_obs_kf, "null map-point table");
    return ORB_OK;
}

inline int mm_items_check(const orbmm_graph* g, int32_t n_items, const int32_t* item) {
    ORB_CHECK_ARG(n_items >= 0, "negative sizes");
    ORB_CHECK_ARG(n_items == 0 || item, "null item");
    ORB_CHECK_ARG((long long)n_items * std::max(g->n_keyframes, 1) < MM_MAX_ENTRIES, "a table of 2^31 entries or more");
    return ORB_OK;
}

inline int mm_graph_rows_check_host(const orbmm_graph* g) {
    return mm_rows_check_host(g->n_keyframes, g->conn_cap, g->conn_slot, g->n_conn, g->ord_slot, g->n_ord);
}

inline int mm_graph_check_host(const orbmm_graph* g, int32_t n_items, const int32_t* item) {
    const int K = g->n_keyframes, M = g->n_mappoints;
    int rc;
    if ((rc = check_range(g->kf_n, K, 0, g->kf_cap + 1, "kf_n outside [0, kf_cap]"))) return rc;
    if ((rc = check_range(g->kf_mappoint, (size_t)K * g->kf_cap, -1, M, "kf_mappoint entry outside [-1, n_mappoints)"))) return rc;
    if ((rc = check_csr(g->mp_obs_off, M, g->n_obs, "mp_obs"))) return rc;
    if ((rc = check_range(g->mp_obs_kf, g->mp_obs_off[M], 0, K, "mp_obs_kf entry outside [0, n_keyframes)"))) return rc;
    if ((rc = mm_graph_rows_check_host(g))) return rc;
    if ((rc = check_range(g->kf_parent, K, -1, K, "kf_parent outside [-1, n_keyframes)"))) return rc;
    if ((rc = check_range(g->kf_covis, (size_t)K * MM_COVIS, -1, K, "kf_covis entry outside [-1, n_keyframes)"))) return rc;
    return check_range(item, n_items, 0, K, "item outside [0, n_keyframes)");
}

// kf_mappoint (entries in [-1, M), kf_n in [0, kf_cap]): no map point twice in a keyframe's row.
inline int mm_check_rows_distinct(int K, int M, int kf_cap, const int32_t* kf_n, const int32_t* kf_mappoint) {
    std::vector<int32_t> seen(M, -1);
    for (int k = 0; k < K; k++)
        for (int i = 0; i < kf_n[k]; i++) {
            const int p = kf_mappoint[(size_t)k * kf_cap + i];
            if (p < 0) continue;
            ORB_CHECK_ARG(seen[p] != k, "a map point twice in a keyframe's row");
            seen[p] = k;
        }
    return ORB_OK;
}

}  // namespace orbamd
