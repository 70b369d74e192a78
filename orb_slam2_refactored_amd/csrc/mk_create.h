// Where the map grows: KeyFrame::KeyFrame(const Frame&, ...) (src/KeyFrame.cc:51-64) and MapPoint::MapPoint(Xw, referenceKF,
// map) (src/MapPoint.cc:44-56) with the calls that follow a construction: AddObservation, ComputeDistinctiveDescriptors on
// one or two observations, KeyFrame::AddMapPoint, Map::AddMapPoint (src/Tracking.cc:724-736, :981-997, :1104-1126,
// src/LocalMapping.cc:562-575), on slot tables, in place.  Per-element rules only: integers and copied float bits.
// Compiles for host and device; orbmk.hip runs them from its kernels, tests/native/creation_check.cpp one after another.
//
// Slot numbers: the valid entries of a list batch are numbered in creation order (items ascending, list position
// ascending); entry number r takes slot base + r.  The numbering is a count per chunk of MK_CHUNK list positions, one
// scan over the chunks (csrc/mm_groups.h on the device), then the fill.  Everything is decided before anything is written
// (mk_decide's rules): the fill runs only when every slot exists, every taken row holds its observations and the list
// fits `recent`.
#pragma once

#include "mm_connect.h"

namespace orbamd {

constexpr int MK_OK = 0, MK_OVERFLOW = 1;   // ORBMK_*
constexpr int MK_CHUNK = 256;               // list positions per count: one workgroup
constexpr int MK_COVIS = MM_COVIS;

struct alignas(16) MkDesc {
    uint32_t w[8];
};

struct MkKeypoint {   // orbx_keypoint
    float x, y, size, angle, response;
    int32_t octave, class_id;
};

struct MkFrames {
    int F, kp_cap;
    const int32_t* frame_n;
    const int32_t* frame_mappoint;
    const MkKeypoint* kp_un;
    const int32_t* kp_octave;
    const float *kp_uright, *kp_depth;
    const MkDesc* kp_desc;
    const float *pose, *camera;
};

struct MkKeyframes {
    int K, kf_cap, conn_cap;
    int32_t *kf_id, *kf_n, *kf_mappoint;
    MkKeypoint* kf_keypoint;
    int32_t* kf_kp_octave;
    float *kf_uright, *kf_depth;
    MkDesc* kf_desc;
    float *kf_pose, *kf_camera;
    uint8_t *kf_bad, *kf_not_erase, *kf_to_be_erased;
    int32_t* kf_parent;
    uint8_t* kf_first_connection;
    int32_t *conn_slot, *conn_weight, *n_conn, *ord_slot, *ord_weight, *n_ord, *kf_covis;
};

struct MkItems {
    int n_items;
    const int32_t *frame, *kf, *id;
    const float* baseline;
};

// Item `it` of the batch: the frame and the keyframe slot, or false when either is outside its table.
MM_HD bool mk_item(const MkFrames& fr, const MkKeyframes& t, const MkItems& a, int it, int& f, int& k) {
    f = a.frame[it];
    k = a.kf[it];
    return f >= 0 && f < fr.F && k >= 0 && k < t.K;
}

// Keypoint row i < kf_cap of item (f, k): the copied columns below frame_n[f], kf_mappoint = -1 from there on.
MM_HD void mk_insert_keypoint(const MkFrames& fr, const MkKeyframes& t, int f, int k, int i) {
    const int n = mm_clamp(fr.frame_n[f], 0, fr.kp_cap);   // kp_cap <= kf_cap
    const size_t to = (size_t)k * t.kf_cap + i, from = (size_t)f * fr.kp_cap + i;
    if (i >= n) {
        if (t.kf_mappoint) t.kf_mappoint[to] = -1;
        return;
    }
    if (t.kf_mappoint) t.kf_mappoint[to] = fr.frame_mappoint[from];   // outliers included: mappoints_(frame.mappoints)
    if (t.kf_keypoint) t.kf_keypoint[to] = fr.kp_un[from];
    if (t.kf_kp_octave) t.kf_kp_octave[to] = fr.kp_octave[from];
    if (t.kf_uright) t.kf_uright[to] = fr.kp_uright[from];
    if (t.kf_depth) t.kf_depth[to] = fr.kp_depth[from];
    if (t.kf_desc) t.kf_desc[to] = fr.kp_desc[from];
}

// Entry q < MK_HEAD_ENTRIES + conn_cap of the keyframe's own state: the constructor's initialisers and SetPose.
constexpr int MK_HEAD_ENTRIES = 12 + 6 + MK_COVIS + 1;
MM_HD void mk_insert_head(const MkFrames& fr, const MkKeyframes& t, const MkItems& a, int it, int f, int k, int q) {
    if (q < 12) {
        if (t.kf_pose) t.kf_pose[12 * (size_t)k + q] = fr.pose[12 * (size_t)f + q];
    } else if (q < 18) {
        const int c = q - 12;
        if (t.kf_camera) t.kf_camera[6 * (size_t)k + c] = c < 5 ? fr.camera[5 * (size_t)f + c] : a.baseline[it];
    } else if (q < 18 + MK_COVIS) {
        if (t.kf_covis) t.kf_covis[MK_COVIS * (size_t)k + (q - 18)] = -1;
    } else if (q == 18 + MK_COVIS) {
        if (t.kf_n) t.kf_n[k] = mm_clamp(fr.frame_n[f], 0, fr.kp_cap);
        if (t.kf_id) t.kf_id[k] = a.id[it];
        if (t.kf_bad) t.kf_bad[k] = 0;
        if (t.kf_not_erase) t.kf_not_erase[k] = 0;
        if (t.kf_to_be_erased) t.kf_to_be_erased[k] = 0;
        if (t.kf_parent) t.kf_parent[k] = -1;
        if (t.kf_first_connection) t.kf_first_connection[k] = 1;
        if (t.n_conn) t.n_conn[k] = 0;
        if (t.n_ord) t.n_ord[k] = 0;
    } else {
        const size_t at = (size_t)k * t.conn_cap + (q - MK_HEAD_ENTRIES);
        if (t.conn_slot) t.conn_slot[at] = -1;
        if (t.conn_weight) t.conn_weight[at] = 0;
        if (t.ord_slot) t.ord_slot[at] = -1;
        if (t.ord_weight) t.ord_weight[at] = 0;
    }
}

struct MkMap {
    int K, M, kf_cap, n_obs;
    const int32_t *kf_id, *kf_n;
    int32_t* kf_mappoint;
    const float* kf_uright;
    const uint8_t* kf_bad;
    const MkDesc* kf_desc;
    uint8_t* mp_bad;
    float *mp_xw, *mp_normal, *mp_max_min;
    int32_t *mp_nobs, *mp_found, *mp_visible, *mp_replaced, *mp_first_kf_id, *mp_ref_kf;
    MkDesc* mp_desc;
    const int32_t* mp_obs_off;
    int32_t *mp_obs_kf, *mp_obs_idx;
};

struct MkLists {
    int n_items, list_cap, by_keypoint;
    const int32_t *kf1, *kf2, *n_list, *idx1, *idx2;
    const float *xw, *normal, *max_distance, *min_distance;
    int F, kp_cap;
    const int32_t* item_frame;
    int32_t* frame_mappoint;
};

struct MkOut {
    int32_t *alloc, *status, *needed, *created, *n_created, *recent, *n_recent;
    int recent_cap;
};

MM_HD int mk_chunks(int list_cap) { return (list_cap + MK_CHUNK - 1) / MK_CHUNK; }

MM_HD int mk_list_n(const MkLists& l, int i) { return mm_clamp(l.n_list[i], 0, l.list_cap); }

// The item's second keyframe: -1 for the one-observation form (kf2 NULL or -1), -2 for a slot outside the table.
MM_HD int mk_second(const MkMap& t, const MkLists& l, int i) {
    const int k2 = l.kf2 ? l.kf2[i] : -1;
    return k2 == -1 ? -1 : (k2 >= 0 && k2 < t.K ? k2 : -2);
}

// The observations a point of item i takes in its row.
MM_HD int mk_need(const MkLists& l, int i) { return l.kf2 && l.kf2[i] != -1 ? 2 : 1; }

// Entry j < mk_list_n of item i: the keyframe slot(s) inside the table, the keypoints below kf_n, kf1 != kf2; addressed by
// keypoint, idx1 also inside the value row.
MM_HD bool mk_entry_valid(const MkMap& t, const MkLists& l, int i, int j) {
    const int k1 = l.kf1[i], k2 = mk_second(t, l, i);
    if (k1 < 0 || k1 >= t.K || k2 == -2 || k1 == k2) return false;
    const size_t at = (size_t)i * l.list_cap + j;
    const int i1 = l.idx1[at];
    if (i1 < 0 || i1 >= mm_clamp(t.kf_n[k1], 0, t.kf_cap) || (l.by_keypoint && i1 >= l.list_cap)) return false;
    if (k2 < 0) return true;
    const int i2 = l.idx2[at];
    return i2 >= 0 && i2 < mm_clamp(t.kf_n[k2], 0, t.kf_cap);
}

MM_HD void mk_row(const MkMap& t, int p, int& e0, int& e1) {
    e0 = mm_clamp(t.mp_obs_off[p], 0, t.n_obs);
    e1 = mm_clamp(t.mp_obs_off[p + 1], e0, t.n_obs);
}

// Slot p in [0, M) holds `need` observations.
MM_HD bool mk_row_fits(const MkMap& t, int p, int need) {
    int e0, e1;
    mk_row(t, p, e0, e1);
    return e1 - e0 >= need;
}

MM_HD int mk_base(const MkMap& t, const MkOut& o) { return mm_clamp(o.alloc[0], 0, t.M); }
MM_HD int mk_recent_base(const MkOut& o) { return o.recent ? mm_clamp(o.n_recent[0], 0, o.recent_cap) : 0; }

// What one lane decides once the total and the first short row (-1: none) are known; status, needed, alloc and n_recent.
MM_HD int mk_decide(const MkMap& t, const MkOut& o, int base, int recent_base, long long total, int short_slot) {
    const bool fits = base + total <= t.M;
    const bool ok = fits && short_slot < 0 && (!o.recent || recent_base + total <= o.recent_cap);
    const long long want = base + total;
    o.needed[0] = (int32_t)(want < 0x7fffffffLL ? want : 0x7fffffffLL);
    o.needed[1] = fits ? short_slot : -1;
    o.status[0] = ok ? MK_OK : MK_OVERFLOW;
    if (ok) {
        o.alloc[0] = (int32_t)want;
        if (o.recent) o.n_recent[0] = recent_base + (int32_t)total;
    }
    return ok ? MK_OK : MK_OVERFLOW;
}

// The constructor and the calls after it for valid entry (i, j), number r of the batch, on slot p = base + r in [0, M)
// whose row fits.  One lane; no other entry writes what this one writes unless a keypoint is listed twice.
MM_HD void mk_create_point(const MkMap& t, const MkLists& l, const MkOut& o, int i, int j, int p, int recent_at) {
    const size_t at = (size_t)i * l.list_cap + j;
    const int k1 = l.kf1[i], k2 = mk_second(t, l, i), i1 = l.idx1[at], i2 = k2 >= 0 ? l.idx2[at] : -1;
    const size_t v = (size_t)i * l.list_cap + (l.by_keypoint ? i1 : j);
    for (int c = 0; c < 3; c++) {
        t.mp_xw[3 * (size_t)p + c] = l.xw[3 * v + c];
        if (t.mp_normal) t.mp_normal[3 * (size_t)p + c] = l.normal ? l.normal[3 * v + c] : 0.f;
    }
    if (t.mp_max_min) {
        t.mp_max_min[2 * (size_t)p] = l.max_distance ? l.max_distance[v] : 0.f;
        t.mp_max_min[2 * (size_t)p + 1] = l.min_distance ? l.min_distance[v] : 0.f;
    }
    t.mp_bad[p] = 0;
    t.mp_replaced[p] = -1;
    t.mp_found[p] = t.mp_visible[p] = 1;
    t.mp_first_kf_id[p] = t.kf_id[k1];
    t.mp_ref_kf[p] = k1;
    // the row ascends in keyframe slot (mm_observe.h's rule)
    const bool swap = k2 >= 0 && k2 < k1;
    const int ka = swap ? k2 : k1, ia = swap ? i2 : i1, kb = swap ? k1 : k2, ib = swap ? i1 : i2;
    int e0, e1;
    mk_row(t, p, e0, e1);
    t.mp_obs_kf[e0] = ka;
    t.mp_obs_idx[e0] = ia;
    if (kb >= 0) {
        t.mp_obs_kf[e0 + 1] = kb;
        t.mp_obs_idx[e0 + 1] = ib;
    }
    for (int e = e0 + (kb >= 0 ? 2 : 1); e < e1; e++) t.mp_obs_kf[e] = t.mp_obs_idx[e] = -1;
    int nobs = t.kf_uright[(size_t)ka * t.kf_cap + ia] >= 0 ? 2 : 1;   // MapPoint.cc:118-121
    if (kb >= 0) nobs += t.kf_uright[(size_t)kb * t.kf_cap + ib] >= 0 ? 2 : 1;
    t.mp_nobs[p] = nobs;
    t.kf_mappoint[(size_t)k1 * t.kf_cap + i1] = p;
    if (k2 >= 0) t.kf_mappoint[(size_t)k2 * t.kf_cap + i2] = p;
    if (t.mp_desc) {   // MapPoint.cc:300-314 for N <= 2: both medians are 0, the first row that is not bad stays
        const bool a_bad = t.kf_bad && t.kf_bad[ka], b_bad = kb < 0 || (t.kf_bad && t.kf_bad[kb]);
        if (!a_bad) t.mp_desc[p] = t.kf_desc[(size_t)ka * t.kf_cap + ia];
        else if (!b_bad) t.mp_desc[p] = t.kf_desc[(size_t)kb * t.kf_cap + ib];
    }
    if (l.frame_mappoint) {
        const int f = l.item_frame[i];
        if (f >= 0 && f < l.F && i1 < l.kp_cap) l.frame_mappoint[(size_t)f * l.kp_cap + i1] = p;
    }
    if (o.created) o.created[at] = p;
    if (o.recent) o.recent[recent_at] = p;   // recent_at < recent_cap: decided
}

}  // namespace orbamd
