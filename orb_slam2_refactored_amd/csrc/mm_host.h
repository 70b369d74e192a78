// What the host side of orbmm.hip and orbmm_observe.hip shares: the per-thread buffers and the table checks of their
// host entries (check_csr and check_range are common.h's).
#pragma once
#include <vector>

#include "common.h"

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
