// LoopCorrector::Correct (src/LoopClosing.cc:546-676) on the slot tables of orbmm_points / orbmm_graph: the rules and the
// float arithmetic of the propagation of Scw to the current keyframe's neighbours (:554-613), of the connected list
// (:550-552) and of the LoopConnections sets (:661-676).  Compiles for host and device (-ffp-contract=off, as the whole
// library): orblc.hip runs it one lane per keyframe / row entry / point, tests/native/loop_correct_check.cpp on the CPU,
// tests/loop_correct_ref.py restates it in numpy.  The Sim3 class is eg_edge.h's F3, the CameraPose algebra
// gba_update.h's, UpdateNormalAndDepth mm_normal.h's.
//   per keyframe k  edge_sim3[k] = Sim3(Tkw) (scale 1); vertex_sim3[k] the same, or for a connected keyframe
//                   Sim3(Tkw * Twc) * Scw (Scw itself for cur); the camera centre of the entry pose; for a connected
//                   keyframe the pose (R, (1. / s) * t) of its vertex row (1. / s and the product in double, each
//                   component narrowed) and that pose's centre.  Everything from the poses as they are on entry.
//   claim           a point listed in kf_mappoint[k][0 .. kf_n[k]) of a connected k, not null, inside its table, not bad
//                   and not carrying kf_id[cur], belongs to the lowest such k (the reference walks CorrectedSim3, a
//                   std::map<KeyFrame*, ...>: here in ascending slot order).
//   per point p     claimed by k: Xw = (CorrectedSwk * Skw).Map(Xw) (Inverse, the product, Map, in float),
//                   mp_corrected_by = kf_id[cur], mp_corrected_ref = k, then UpdateNormalAndDepth where observer o (and
//                   the reference keyframe) stands at the centre of its corrected pose if it is connected and o < k
//                   (its SetPose ran earlier in the walk) and at that of its entry pose otherwise.
//                   point_ref[p] = -1 (bad), mp_corrected_ref[p] where mp_corrected_by[p] == kf_id[cur], else mp_ref_kf[p].
// A slot or an index outside its table is skipped.
#pragma once

#include <cstdint>

#include "eg_edge.h"
#include "gba_update.h"
#include "mm_normal.h"

namespace orbamd {

constexpr int32_t LC_UNCLAIMED = 0x7fffffff;

struct LcMap {
    MmPoints pts;   // kf_ow: the centres of the entry poses (LcWork::ow_entry)
    int conn_cap;
    const int32_t* kf_id;
    const int32_t* kf_mappoint;
    float* mp_xw;
    float* kf_pose;
    int32_t* mp_corrected_by;
    int32_t* mp_corrected_ref;
};

// Per call, every array written before it is read
struct LcWork {
    float* ow_entry;     // [K][3]
    float* ow_corr;      // [K][3] connected keyframes only
    float* new_pose;     // [K][12] connected keyframes only
    uint8_t* is_conn;    // [K]
    int32_t* claim;      // [M] LC_UNCLAIMED or the claiming slot
};

MM_HD bool lc_listed(const int32_t* list, int n, int k) {
    bool hit = false;
    for (int j = 0; j < n; j++) hit = hit || list[j] == k;
    return hit;
}

MM_HD int lc_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

MM_HD void lc_sim3_of_pose(const float* T, F3& o) {
    for (int i = 0; i < 9; i++) o.R[i] = T[i];
    for (int i = 0; i < 3; i++) o.t[i] = T[9 + i];
    o.s = 1.f;
}

MM_HD void lc_store(const F3& a, float* row) {
    for (int i = 0; i < 9; i++) row[i] = a.R[i];
    for (int i = 0; i < 3; i++) row[9 + i] = a.t[i];
    row[12] = a.s;
}

// :554-576 and the pose of :605-609 for keyframe k; cur in [0, K)
MM_HD void lc_keyframe(const LcMap& t, const LcWork& w, int k, int cur, const float* scw, const int32_t* connected,
                       int max_connected, float* vertex_sim3, float* edge_sim3) {
    const float* Tiw = t.kf_pose + 12 * (size_t)k;
    F3 non;
    lc_sim3_of_pose(Tiw, non);
    lc_store(non, edge_sim3 + 13 * (size_t)k);
    mm_center(Tiw, w.ow_entry + 3 * (size_t)k);
    const bool conn = lc_listed(connected, max_connected, k);
    w.is_conn[k] = conn ? 1 : 0;
    if (!conn) {
        lc_store(non, vertex_sim3 + 13 * (size_t)k);
        return;
    }
    F3 corr;
    if (k == cur) {
        f3_load(scw, corr);
    } else {
        float Twc[12], Tic[12];
        gba_pose_inverse(t.kf_pose + 12 * (size_t)cur, Twc);
        gba_pose_mul(Tiw, Twc, Tic);
        F3 sic, s;
        lc_sim3_of_pose(Tic, sic);
        f3_load(scw, s);
        f3_mul(sic, s, corr);
    }
    lc_store(corr, vertex_sim3 + 13 * (size_t)k);
    float* pose = w.new_pose + 12 * (size_t)k;
    const double invs = 1. / corr.s;
    for (int i = 0; i < 9; i++) pose[i] = corr.R[i];
    for (int i = 0; i < 3; i++) pose[9 + i] = (float)(corr.t[i] * invs);
    mm_center(pose, w.ow_corr + 3 * (size_t)k);
}

// The point entry i of connected keyframe k offers to the claim, or -1 (:587-590)
MM_HD int lc_claimed_point(const LcMap& t, int k, int i, int cur_id) {
    if (i >= lc_clamp(t.pts.kf_n[k], 0, t.pts.kf_cap)) return -1;
    const int p = t.kf_mappoint[(size_t)k * t.pts.kf_cap + i];
    if (p < 0 || p >= t.pts.M || t.pts.mp_bad[p] || t.mp_corrected_by[p] == cur_id) return -1;
    return p;
}

// The centre of observer o while the points of keyframe `claimer` are corrected
struct LcCenter {
    const float* ow_entry;
    const float* ow_corr;
    const uint8_t* is_conn;
    int claimer;
    MM_HD const float* operator()(int o) const {
        return (is_conn[o] && o < claimer) ? ow_corr + 3 * (size_t)o : ow_entry + 3 * (size_t)o;
    }
};

// :583-599 for point p and its point_ref entry
MM_HD void lc_point(const LcMap& t, const LcWork& w, int p, int cur_id, const float* vertex_sim3, const float* edge_sim3,
                    int32_t* point_ref) {
    const int k = w.claim[p];
    if (k != LC_UNCLAIMED) {
        F3 csiw, siw, cswi, corr;
        f3_load(vertex_sim3 + 13 * (size_t)k, csiw);
        f3_load(edge_sim3 + 13 * (size_t)k, siw);
        f3_inverse(csiw, cswi);
        f3_mul(cswi, siw, corr);
        float* X = t.mp_xw + 3 * (size_t)p;
        const float P[3] = {X[0], X[1], X[2]};
        float o[3];
        f3_map(corr, P, o);
        for (int i = 0; i < 3; i++) X[i] = o[i];
        t.mp_corrected_by[p] = cur_id;
        t.mp_corrected_ref[p] = k;
        mm_update_point_at(t.pts, p, LcCenter{w.ow_entry, w.ow_corr, w.is_conn, k});
    }
    point_ref[p] = t.pts.mp_bad[p] ? -1 : (t.mp_corrected_by[p] == cur_id ? t.mp_corrected_ref[p] : t.pts.mp_ref_kf[p]);
}

// :669-675: whether slot s of a connection row stays in the LoopConnections set
MM_HD bool lc_new_link(int s, int K, const int32_t* prev, int n_prev, const int32_t* connected, int max_connected) {
    return s >= 0 && s < K && !lc_listed(prev, n_prev, s) && !lc_listed(connected, max_connected, s);
}

}  // namespace orbamd
