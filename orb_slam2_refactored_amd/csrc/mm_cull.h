// LocalMapping::MapPointCulling and KeyFrameCulling (src/LocalMapping.cc:335-369, 641-701) with MapPoint::SetBadFlag,
// MapPoint::EraseObservation (src/MapPoint.cc:124-182), KeyFrame::SetBadFlag and EraseConnection (src/KeyFrame.cc:379-489)
// on slot tables, in place.  Compiles for host and device over the groups of mm_connect.h: cull_keyframes takes a wide
// group B (the workgroup; every lane of it enters and takes every branch on a reduced or uniformly loaded value together)
// and a narrow group W, one of n_sub that partition B (a wavefront), for the work that is split by neighbour and for the
// tree loop.  On the CPU both are MmOne.  An erased observation is a -1 in mp_obs_kf; every reader skips it.
//
// Phases of one culled target, a B.sync() between them: EraseConnection on the neighbours (one W each: a row has one
// writer), EraseObservation over the target's row (one lane per entry: a point has one writer on tables where no point
// is twice in a row), the target's rows cleared, the spanning tree by sub-group 0.
#pragma once

#include "gba_update.h"
#include "mm_connect.h"

namespace orbamd {

struct MmCull {
    int K, M, kf_cap, conn_cap, n_obs;
    const int32_t* kf_id;
    const int32_t* kf_n;
    int32_t* kf_mappoint;
    const int32_t* kf_kp_octave;
    const float* kf_uright;
    const float* kf_depth;
    const float* kf_pose;
    uint8_t* kf_bad;
    const uint8_t* kf_not_erase;
    uint8_t* kf_to_be_erased;
    float* kf_tcp;
    uint8_t* mp_bad;
    int32_t* mp_nobs;
    const int32_t* mp_found;
    const int32_t* mp_visible;
    const int32_t* mp_first_kf_id;
    int32_t* mp_ref_kf;
    const int32_t* mp_obs_off;
    int32_t* mp_obs_kf;
    const int32_t* mp_obs_idx;
    int32_t *conn_slot, *conn_weight, *n_conn, *ord_slot, *ord_weight, *n_ord, *kf_parent, *kf_covis;
};

constexpr int CULL_KEEP = 0, CULL_DROP = 1, CULL_BAD = 2;
constexpr int CULL_MIN_OBS = 3;   // KeyFrameCulling's minObservations

// int32 entries of cull_keyframes' scratch with n_sub narrow groups
MM_HD size_t cull_scratch_entries(int K, int conn_cap, int n_sub) {
    return (size_t)conn_cap * (1 + 2 * (size_t)n_sub) + 2 * (size_t)K + 1;
}

MM_HD void cull_obs_range(const MmCull& t, int p, int& e0, int& e1) {
    e0 = t.mp_obs_off[p];
    e1 = t.mp_obs_off[p + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > t.n_obs) e1 = t.n_obs;
}

// MapPoint::SetBadFlag (MapPoint.cc:164-182); nobservations_ stays.  One lane.
MM_HD void cull_set_bad(const MmCull& t, int p) {
    t.mp_bad[p] = 1;
    int e0, e1;
    cull_obs_range(t, p, e0, e1);
    for (int e = e0; e < e1; e++) {
        const int o = t.mp_obs_kf[e], idx = t.mp_obs_idx[e];
        if (o >= 0 && o < t.K && idx >= 0 && idx < t.kf_cap) t.kf_mappoint[(size_t)o * t.kf_cap + idx] = -1;   // EraseMapPointMatch(idx)
        t.mp_obs_kf[e] = -1;
    }
}

// One entry of recentAddedMapPoints_ (LocalMapping.cc:344-367).  A slot outside the table is dropped.  One lane.
MM_HD int cull_point_decision(const MmCull& t, int p, int cur_kf_id, int min_obs) {
    if (p < 0 || p >= t.M) return CULL_DROP;
    if (t.mp_bad[p]) return CULL_DROP;
    const long long age = (long long)cur_kf_id - t.mp_first_kf_id[p];
    if ((float)t.mp_found[p] / (float)t.mp_visible[p] < 0.25f) return CULL_BAD;   // GetFoundRatio()
    if (age >= 2 && t.mp_nobs[p] <= min_obs) return CULL_BAD;
    if (age >= 3) return CULL_DROP;
    return CULL_KEEP;
}

// The counts of KeyFrameCulling for target k (LocalMapping.cc:655-696).
template <class G>
MM_HD void cull_count(const G& g, const MmCull& t, int k, bool monocular, float th_depth, int& npoints, int& nredundant) {
    const int n = mm_clamp(t.kf_n[k], 0, t.kf_cap);
    int np = 0, nr = 0;
    for (int i1 = g.lane; i1 < n; i1 += g.width) {
        const int p = t.kf_mappoint[(size_t)k * t.kf_cap + i1];
        if (p < 0 || p >= t.M || t.mp_bad[p]) continue;
        if (!monocular) {
            const float d = t.kf_depth[(size_t)k * t.kf_cap + i1];
            if (d > th_depth || d < 0) continue;
        }
        np++;
        if (t.mp_nobs[p] > CULL_MIN_OBS) {
            const long long target_scale = t.kf_kp_octave[(size_t)k * t.kf_cap + i1];
            int nobs = 0, e0, e1;
            cull_obs_range(t, p, e0, e1);
            for (int e = e0; e < e1 && nobs < CULL_MIN_OBS; e++) {
                const int o = t.mp_obs_kf[e], i2 = t.mp_obs_idx[e];
                if (o < 0 || o >= t.K || o == k || i2 < 0 || i2 >= t.kf_cap) continue;
                if (t.kf_kp_octave[(size_t)o * t.kf_cap + i2] <= target_scale + 1) nobs++;
            }
            if (nobs >= CULL_MIN_OBS) nr++;
        }
    }
    npoints = g.sum(np);
    nredundant = g.sum(nr);
}

// KeyFrame::EraseConnection(k) on v (KeyFrame.cc:478-489): k leaves v's connection row, UpdateBestCovisibles follows.
// ws / ww: conn_cap entries each, this group's own.
template <class G>
MM_HD void cull_erase_connection(const G& g, const MmCull& t, int v, int k, int32_t* ws, int32_t* ww) {
    const int cap = t.conn_cap, n = mm_clamp(t.n_conn[v], 0, cap);
    const int32_t* cs = t.conn_slot + (size_t)v * cap;
    const int32_t* cw = t.conn_weight + (size_t)v * cap;
    int pos = MM_NO_POS;
    for (int e = g.lane; e < n; e += g.width)
        if (cs[e] == k && e < pos) pos = e;
    pos = g.min(pos);
    if (pos >= n) return;   // connectionTo_.count(keyframe) == 0
    for (int e = g.lane; e < n; e += g.width)
        if (e != pos) {
            ws[e - (e > pos ? 1 : 0)] = cs[e];
            ww[e - (e > pos ? 1 : 0)] = cw[e];
        }
    g.sync();
    MmGraph m{};
    m.K = t.K; m.conn_cap = cap;
    m.conn_slot = t.conn_slot; m.conn_weight = t.conn_weight; m.n_conn = t.n_conn;
    m.ord_slot = t.ord_slot; m.ord_weight = t.ord_weight; m.n_ord = t.n_ord; m.covis = t.kf_covis;
    MmItem none;
    none.kf = -1; none.any = 1; none.max_slot = -1; none.front = -1; none.max_count = 0;
    mm_commit_rows(g, m, v, none, MM_FORM_ALL, ws, ww, n - 1);
    g.sync();
}

// MapPoint::EraseObservation(k) on p (MapPoint.cc:124-150).  One lane.
MM_HD void cull_erase_observation(const MmCull& t, int p, int k) {
    int e0, e1, at = -1;
    cull_obs_range(t, p, e0, e1);
    for (int e = e0; e < e1 && at < 0; e++)
        if (t.mp_obs_kf[e] == k) at = e;
    if (at < 0) return;
    const int idx = t.mp_obs_idx[at];
    const bool stereo = idx >= 0 && idx < t.kf_cap && t.kf_uright[(size_t)k * t.kf_cap + idx] >= 0;
    const int nobs = t.mp_nobs[p] - (stereo ? 2 : 1);
    t.mp_nobs[p] = nobs;
    t.mp_obs_kf[at] = -1;
    if (t.mp_ref_kf[p] == k) {
        int first = -1;
        for (int e = e0; e < e1 && first < 0; e++) {
            const int o = t.mp_obs_kf[e];
            if (o >= 0 && o < t.K) first = o;
        }
        t.mp_ref_kf[p] = first;
    }
    if (nobs <= 2) cull_set_bad(t, p);
}

// The spanning tree around the culled k (KeyFrame.cc:408-465), Tcp and the flag.  children: K entries, cand: K + 1.
template <class G>
MM_HD void cull_update_tree(const G& g, const MmCull& t, int k, int32_t* children, int32_t* cand) {
    const int K = t.K, cap = t.conn_cap, parent = t.kf_parent[k];
    int n_child = 0, n_cand = 0;
    for (int base = 0; base < K; base += g.width) {   // uniform trip count; ascending slots
        const int c = base + g.lane;
        const bool flag = c < K && c != k && t.kf_parent[c] == k && !t.kf_bad[c];
        int total;
        const int off = g.prefix(flag, total);
        if (flag) children[n_child + off] = c;
        n_child += total;
    }
    if (g.lane == 0 && parent >= 0 && parent < K) cand[0] = parent;
    if (parent >= 0 && parent < K) n_cand = 1;
    g.sync();
    for (int left = n_child; left > 0 && n_cand > 0; left--) {
        int best_w = -1, best_at = MM_NO_POS;   // at = child position * cap + entry: the order the reference meets them in
        for (int j = 0; j < n_child; j++) {
            const int c = children[j];
            if (c < 0) continue;   // has its parent
            const int n_ord = mm_clamp(t.n_ord[c], 0, cap), n_conn = mm_clamp(t.n_conn[c], 0, cap);
            for (int e = g.lane; e < n_ord; e += g.width) {
                const int s = t.ord_slot[(size_t)c * cap + e];
                if (s < 0 || s >= K) continue;
                bool is_cand = false;
                for (int q = 0; q < n_cand && !is_cand; q++) is_cand = t.kf_id[s] == t.kf_id[cand[q]];
                if (!is_cand) continue;
                int w = 0;   // GetWeight
                for (int x = 0; x < n_conn; x++)
                    if (t.conn_slot[(size_t)c * cap + x] == s) {
                        w = t.conn_weight[(size_t)c * cap + x];
                        break;
                    }
                if (w > best_w) {
                    best_w = w;
                    best_at = j * cap + e;
                }
            }
        }
        const int w = g.max(best_w);
        if (w < 0) break;   // !found
        const int at = g.min(best_w == w ? best_at : MM_NO_POS);
        const int j = at / cap, c = children[j];
        g.sync();   // every lane has read children[j] and cand
        if (g.lane == 0) {
            t.kf_parent[c] = t.ord_slot[(size_t)c * cap + at % cap];   // ChangeParent
            cand[n_cand] = c;
            children[j] = -1;
        }
        n_cand++;
        g.sync();
    }
    for (int j = g.lane; j < n_child; j += g.width)
        if (children[j] >= 0) t.kf_parent[children[j]] = parent;
    if (g.lane == 0) {
        if (parent >= 0 && parent < K) {
            float inv[12], tcp[12];
            gba_pose_inverse(t.kf_pose + 12 * (size_t)parent, inv);
            gba_pose_mul(t.kf_pose + 12 * (size_t)k, inv, tcp);
            for (int i = 0; i < 12; i++) t.kf_tcp[12 * (size_t)k + i] = tcp[i];
        }
        t.kf_bad[k] = 1;
    }
    g.sync();
}

// KeyFrame::SetBadFlag on k past the notErase_ test (KeyFrame.cc:394-465).
template <class GB, class GW>
MM_HD void cull_keyframe(const GB& b, const GW& w, int sub, int n_sub, const MmCull& t, int k, int32_t* scratch) {
    const int cap = t.conn_cap;
    int32_t* rows = scratch + cap;
    int32_t* children = rows + 2 * (size_t)n_sub * cap;
    int32_t* cand = children + t.K;
    const int n_conn = mm_clamp(t.n_conn[k], 0, cap);
    for (int e = sub; e < n_conn; e += n_sub) {
        const int v = t.conn_slot[(size_t)k * cap + e];
        if (v < 0 || v >= t.K || v == k) continue;
        cull_erase_connection(w, t, v, k, rows + 2 * (size_t)sub * cap, rows + (2 * (size_t)sub + 1) * cap);
    }
    b.sync();
    const int n = mm_clamp(t.kf_n[k], 0, t.kf_cap);
    for (int i = b.lane; i < n; i += b.width) {
        const int p = t.kf_mappoint[(size_t)k * t.kf_cap + i];
        if (p >= 0 && p < t.M) cull_erase_observation(t, p, k);
    }
    for (int e = b.lane; e < cap; e += b.width) {
        t.conn_slot[(size_t)k * cap + e] = t.ord_slot[(size_t)k * cap + e] = -1;
        t.conn_weight[(size_t)k * cap + e] = t.ord_weight[(size_t)k * cap + e] = 0;
    }
    for (int e = b.lane; e < MM_COVIS; e += b.width) t.kf_covis[(size_t)k * MM_COVIS + e] = -1;
    if (b.lane == 0) t.n_conn[k] = t.n_ord[k] = 0;
    b.sync();
    if (sub == 0) cull_update_tree(w, t, k, children, cand);
    b.sync();
}

// KeyFrameCulling(cur).  culled: conn_cap entries; scratch: cull_scratch_entries.  Every lane of b enters.
template <class GB, class GW>
MM_HD void cull_keyframes(const GB& b, const GW& w, int sub, int n_sub, const MmCull& t, int cur, bool monocular,
                          float th_depth, int32_t* culled, int32_t* n_culled, int32_t* status, int32_t* scratch) {
    const int cap = t.conn_cap;
    int32_t* targets = scratch;
    int n_targets = 0, n_out = 0;
    for (int e = b.lane; e < cap; e += b.width) culled[e] = -1;
    if (cur >= 0 && cur < t.K) {
        n_targets = mm_clamp(t.n_ord[cur], 0, cap);
        for (int e = b.lane; e < n_targets; e += b.width) targets[e] = t.ord_slot[(size_t)cur * cap + e];   // the copy iterated
    }
    b.sync();
    for (int i = 0; i < n_targets; i++) {
        const int k = targets[i];
        if (k < 0 || k >= t.K || t.kf_id[k] == 0 || t.kf_bad[k]) continue;
        int npoints, nredundant;
        cull_count(b, t, k, monocular, th_depth, npoints, nredundant);
        if (!(nredundant > 0.9 * npoints)) continue;
        if (t.kf_not_erase[k]) {
            if (b.lane == 0) t.kf_to_be_erased[k] = 1;
            continue;
        }
        cull_keyframe(b, w, sub, n_sub, t, k, scratch);
        if (b.lane == 0) culled[n_out] = k;
        n_out++;
    }
    if (b.lane == 0) {
        *n_culled = n_out;
        *status = MM_OK;
    }
}

// The live entries of p's observations; out_* may be NULL (count only).  One lane.
MM_HD int cull_compact_point(int n_obs, const int32_t* off, const int32_t* kf, const int32_t* idx, int p, int at,
                             int32_t* out_kf, int32_t* out_idx) {
    int e0 = off[p], e1 = off[p + 1], n = 0;
    if (e0 < 0) e0 = 0;
    if (e1 > n_obs) e1 = n_obs;
    for (int e = e0; e < e1; e++) {
        if (kf[e] == -1) continue;
        if (out_kf && at >= 0 && n < n_obs - at) {   // offsets that overlap can sum past the arrays
            out_kf[at + n] = kf[e];
            out_idx[at + n] = idx[e];
        }
        n++;
    }
    return n;
}

}  // namespace orbamd
