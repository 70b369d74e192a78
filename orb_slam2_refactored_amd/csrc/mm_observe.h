// The insert half of the observation graph: MapPoint::AddObservation and MapPoint::Replace (src/MapPoint.cc:109-122,
// 191-230) on slot tables, in place, and the three loops that use them: ProcessNewKeyFrame's (src/LocalMapping.cc:309-326),
// Fuse's apply loops (src/ORBmatcher.cc:957-976, 1070-1084 with src/LoopClosing.cc:652-657) and CorrectLoop's matched
// points (src/LoopClosing.cc:617-634).  The erase half is mm_cull.h's.  Compiles for host and device over the groups of
// mm_connect.h: the walk takes one group G (the workgroup; MmOne on the CPU), and every lane of it takes every branch on
// a reduced or uniformly loaded value together.
//
// A point's row is [mp_obs_off[p], mp_obs_off[p + 1]); an entry whose keyframe is outside [0, K) is free (-1 is what an
// erased entry is).  An insert packs the row's live entries to its front and fills the rest with -1; mp_obs_off never
// changes.  Departures from the reference, beside mm_cull.h's "first remaining observation in CSR order": a row is kept
// ascending in keyframe slot, which stands in for the pointer order of std::map<KeyFrame*, size_t> (the new entry goes
// before the first live entry with a greater slot); the survivor's descriptor is not recomputed inside Replace: the walk
// reports the touched points and the caller recomputes once, on the final observations.
#pragma once

#include "mm_connect.h"

namespace orbamd {

constexpr int MM_OBS_OVERFLOW = 2;   // ORBMM_OBS_OVERFLOW
constexpr int MM_APPLY_FUSE = 0, MM_APPLY_FUSE_SIM3 = 1, MM_APPLY_LOOP_MATCHED = 2;   // ORBMM_APPLY_*
constexpr int OBS_PRESENT = -1;      // AddObservation of a keyframe the point has
constexpr int OBS_NONE = 0, OBS_ADDED = 1, OBS_RECENT = 2;   // what an entry of ProcessNewKeyFrame's loop did

struct MmObserve {
    int K, M, kf_cap, n_obs;
    const int32_t* kf_n;
    int32_t* kf_mappoint;
    const float* kf_uright;
    uint8_t* mp_bad;
    int32_t *mp_nobs, *mp_found, *mp_visible, *mp_replaced;
    const int32_t* mp_obs_off;
    int32_t *mp_obs_kf, *mp_obs_idx;
};

struct MmApply {
    int mode, n_items, n_entries;
    const int32_t *item_kf, *mp_begin, *point, *best_idx;
    int32_t *replace_point, *n_fused, *touched, *n_touched, *progress, *status;
};

// int32 entries of the walk's scratch: Replace's flags of the loser's row and the union, M touched flags
MM_HD size_t obs_scratch_entries(int M, int n_obs) { return 3 * (size_t)n_obs + (size_t)M; }

MM_HD void obs_range(const MmObserve& t, int p, int& e0, int& e1) {
    e0 = mm_clamp(t.mp_obs_off[p], 0, t.n_obs);
    e1 = mm_clamp(t.mp_obs_off[p + 1], e0, t.n_obs);
}

MM_HD bool obs_live(const MmObserve& t, int o) { return o >= 0 && o < t.K; }

MM_HD int obs_weight(const MmObserve& t, int k, int idx) {   // MapPoint.cc:118-121
    return idx >= 0 && idx < t.kf_cap && t.kf_uright[(size_t)k * t.kf_cap + idx] >= 0 ? 2 : 1;
}

// MapPoint::IsInKeyFrame(k), k in [0, K).
template <class G>
MM_HD bool obs_observes(const G& g, const MmObserve& t, int p, int k) {
    int e0, e1, hit = 0;
    obs_range(t, p, e0, e1);
    for (int e = e0 + g.lane; e < e1; e += g.width) hit |= t.mp_obs_kf[e] == k ? 1 : 0;
    return g.max(hit) > 0;
}

// MapPoint::AddObservation(k, idx) on p, k in [0, K): MM_OK, OBS_PRESENT or MM_OBS_OVERFLOW (nothing written).  One lane.
MM_HD int obs_add(const MmObserve& t, int p, int k, int idx) {
    int e0, e1, n = 0;
    obs_range(t, p, e0, e1);
    for (int e = e0; e < e1; e++) {
        const int o = t.mp_obs_kf[e];
        if (o == k) return OBS_PRESENT;
        n += obs_live(t, o) ? 1 : 0;
    }
    if (n == e1 - e0) return MM_OBS_OVERFLOW;
    int w = e0, ins = -1;
    for (int e = e0; e < e1; e++) {   // pack: w <= e
        const int o = t.mp_obs_kf[e], i = t.mp_obs_idx[e];
        if (!obs_live(t, o)) continue;
        if (ins < 0 && o > k) ins = w;
        t.mp_obs_kf[w] = o;
        t.mp_obs_idx[w] = i;
        w++;
    }
    if (ins < 0) ins = w;
    for (int e = w; e > ins; e--) {
        t.mp_obs_kf[e] = t.mp_obs_kf[e - 1];
        t.mp_obs_idx[e] = t.mp_obs_idx[e - 1];
    }
    t.mp_obs_kf[ins] = k;
    t.mp_obs_idx[ins] = idx;
    for (int e = w + 1; e < e1; e++) t.mp_obs_kf[e] = t.mp_obs_idx[e] = -1;
    t.mp_nobs[p] += obs_weight(t, k, idx);
    return MM_OK;
}

// obs_add by lane 0, its result on every lane; the group has passed its reads of the step.
template <class G>
MM_HD int obs_add_uniform(const G& g, const MmObserve& t, int p, int k, int idx) {
    int rc = -MM_NO_POS;
    if (g.lane == 0) rc = obs_add(t, p, k, idx);
    rc = g.max(rc);
    g.sync();
    return rc;
}

// MapPoint::Replace(loser -> survivor), both in [0, M): MM_OK or MM_OBS_OVERFLOW (nothing written).  On ascending rows the
// survivor's new row is the sorted union: every entry is placed at its rank.  ws: the loser's row length + twice the
// survivor's.  Ends in a sync.
template <class G>
MM_HD int obs_replace(const G& g, const MmObserve& t, int loser, int surv, int32_t* ws) {
    if (loser == surv) return MM_OK;   // mappoint->id == this->id
    int l0, l1, s0, s1;
    obs_range(t, loser, l0, l1);
    obs_range(t, surv, s0, s1);
    const int len = l1 - l0, cap = s1 - s0;
    int32_t* where = ws;   // per entry of the loser's row: -2 free, -1 the survivor has the keyframe, else the survivor's entries below it
    int32_t* out_kf = ws + len;
    int32_t* out_idx = out_kf + cap;
    int moved = 0, n_surv = 0;
    for (int e = g.lane; e < len; e += g.width) {
        const int o = t.mp_obs_kf[l0 + e];
        int w = -2;
        if (obs_live(t, o)) {
            bool has = false;
            int below = 0;
            for (int f = s0; f < s1; f++) {
                const int s = t.mp_obs_kf[f];
                if (!obs_live(t, s)) continue;
                has |= s == o;
                below += s < o ? 1 : 0;
            }
            w = has ? -1 : below;
            moved += has ? 0 : 1;
        }
        where[e] = w;
    }
    for (int f = g.lane; f < cap; f += g.width) {
        n_surv += obs_live(t, t.mp_obs_kf[s0 + f]) ? 1 : 0;
        out_kf[f] = out_idx[f] = -1;
    }
    moved = g.sum(moved);
    n_surv = g.sum(n_surv);
    g.sync();
    if (moved > 0 && n_surv + moved > cap) return MM_OBS_OVERFLOW;
    int add = 0;
    if (moved > 0) {
        for (int base = 0, at = 0; base < len; base += g.width) {   // uniform trip count
            const int e = base + g.lane;
            const bool flag = e < len && where[e] >= 0;
            int total;
            const int off = g.prefix(flag, total);
            if (flag) {
                const int pos = where[e] + at + off;   // < n_surv + moved
                out_kf[pos] = t.mp_obs_kf[l0 + e];
                out_idx[pos] = t.mp_obs_idx[l0 + e];
            }
            at += total;
        }
        for (int base = 0, at = 0; base < cap; base += g.width) {
            const int f = base + g.lane;
            const int s = f < cap ? t.mp_obs_kf[s0 + f] : -1;
            const bool flag = f < cap && obs_live(t, s);
            int total;
            const int off = g.prefix(flag, total);
            if (flag) {
                int below = 0;
                for (int e = 0; e < len; e++) below += where[e] >= 0 && t.mp_obs_kf[l0 + e] < s ? 1 : 0;
                out_kf[at + off + below] = s;
                out_idx[at + off + below] = t.mp_obs_idx[s0 + f];
            }
            at += total;
        }
    }
    for (int e = g.lane; e < len; e += g.width) {
        const int w = where[e];
        if (w < -1) continue;
        const int o = t.mp_obs_kf[l0 + e], idx = t.mp_obs_idx[l0 + e];
        if (idx >= 0 && idx < t.kf_cap) t.kf_mappoint[(size_t)o * t.kf_cap + idx] = w >= 0 ? surv : -1;   // Replace- / EraseMapPointMatch
        if (w >= 0) add += obs_weight(t, o, idx);
    }
    add = g.sum(add);
    g.sync();   // the union is complete, both rows have been read
    if (moved > 0)
        for (int f = g.lane; f < cap; f += g.width) {
            t.mp_obs_kf[s0 + f] = out_kf[f];
            t.mp_obs_idx[s0 + f] = out_idx[f];
        }
    for (int e = g.lane; e < len; e += g.width) t.mp_obs_kf[l0 + e] = -1;   // observations_.clear()
    if (g.lane == 0) {
        t.mp_nobs[surv] += add;
        t.mp_found[surv] += t.mp_found[loser];
        t.mp_visible[surv] += t.mp_visible[loser];
        t.mp_bad[loser] = 1;
        t.mp_replaced[loser] = surv;
    }
    g.sync();
    return MM_OK;
}

// One entry of ProcessNewKeyFrame's loop (LocalMapping.cc:312-325) for keyframe cur in [0, K).  One lane.
MM_HD int obs_new_keyframe_entry(const MmObserve& t, int cur, int i, int32_t& status) {
    status = MM_OK;
    if (i >= mm_clamp(t.kf_n[cur], 0, t.kf_cap)) return OBS_NONE;
    const int p = t.kf_mappoint[(size_t)cur * t.kf_cap + i];
    if (p < 0 || p >= t.M || t.mp_bad[p]) return OBS_NONE;
    const int rc = obs_add(t, p, cur, i);
    if (rc == OBS_PRESENT) return OBS_RECENT;
    if (rc == MM_OK) return OBS_ADDED;
    status = rc;
    return OBS_NONE;
}

// One hit of the walk: entry m of an item on keyframe kf in [0, K), phase ph.  MM_OK, or MM_OBS_OVERFLOW with nothing
// written and the point whose row is full in ovf.  flags: M touched flags.  Every lane enters.
template <class G>
MM_HD int obs_step(const G& g, const MmObserve& t, const MmApply& a, int kf, int ph, int m, int32_t* flags, int32_t* ws,
                   int& nf, int& ovf) {
    const int p = a.point[m];
    if (p < 0 || p >= t.M) return MM_OK;
    int loser = -1, surv = -1, rc = MM_OK;
    if (a.mode == MM_APPLY_FUSE_SIM3 && ph == 1) {   // LoopClosing.cc:652-657
        loser = a.replace_point[m];
        surv = p;
        if (loser < 0 || loser >= t.M) return MM_OK;
    } else {
        const int b = a.best_idx[m];
        if (b < 0 || b >= t.kf_cap) return MM_OK;
        const size_t at = (size_t)kf * t.kf_cap + b;
        if (a.mode != MM_APPLY_LOOP_MATCHED && t.mp_bad[p]) return MM_OK;
        if (a.mode == MM_APPLY_FUSE && obs_observes(g, t, p, kf)) return MM_OK;
        const int in_kf = t.kf_mappoint[at];
        if (in_kf >= t.M) return MM_OK;
        const bool in_bad = in_kf >= 0 && t.mp_bad[in_kf];
        const int n_in = in_kf >= 0 ? t.mp_nobs[in_kf] : 0, n_p = t.mp_nobs[p];
        g.sync();   // every lane has read what the step decides on
        if (in_kf < 0) {   // AddObservation, AddMapPoint
            rc = obs_add_uniform(g, t, p, kf, b);
            if (rc == MM_OBS_OVERFLOW) {
                ovf = p;
                return rc;
            }
            if (g.lane == 0) {
                t.kf_mappoint[at] = p;
                if (a.mode == MM_APPLY_LOOP_MATCHED) flags[p] = 1;
            }
            nf++;
            g.sync();
            return MM_OK;
        }
        if (a.mode == MM_APPLY_LOOP_MATCHED) {   // currMP->Replace(loopMP): no bad test
            loser = in_kf;
            surv = p;
        } else if (in_bad) {
            nf++;
            return MM_OK;
        } else if (a.mode == MM_APPLY_FUSE_SIM3) {
            if (g.lane == 0) a.replace_point[m] = in_kf;
            nf++;
            return MM_OK;
        } else if (n_in > n_p) {   // ORBmatcher.cc:964-967
            loser = p;
            surv = in_kf;
        } else {
            loser = in_kf;
            surv = p;
        }
    }
    rc = obs_replace(g, t, loser, surv, ws);
    if (rc == MM_OBS_OVERFLOW) {
        ovf = surv;
        return rc;
    }
    if (g.lane == 0 && loser != surv) flags[surv] = 1;   // the survivor's ComputeDistinctiveDescriptors
    if (!(a.mode == MM_APPLY_FUSE_SIM3 && ph == 1)) nf++;
    g.sync();
    return MM_OK;
}

// The walk.  chunk: g.width entries the group shares; ws: obs_scratch_entries.  Every lane of g enters.
template <class G>
MM_HD void obs_fuse_apply(const G& g, const MmObserve& t, const MmApply& a, int32_t* chunk, int32_t* ws) {
    int32_t* flags = ws + 3 * (size_t)t.n_obs;
    const int it0 = mm_clamp(a.progress[0], 0, a.n_items), ph0 = mm_clamp(a.progress[1], 0, 1), en0 = a.progress[2] < 0 ? 0 : a.progress[2];
    const bool resumed = it0 > 0 || ph0 > 0 || en0 > 0;
    const int n_seed = resumed ? mm_clamp(*a.n_touched, 0, t.M) : 0;
    for (int p = g.lane; p < t.M; p += g.width) flags[p] = 0;
    g.sync();
    for (int i = g.lane; i < n_seed; i += g.width) {   // what an interrupted walk had touched
        const int p = a.touched[i];
        if (p >= 0 && p < t.M) flags[p] = 1;
    }
    g.sync();
    int stop_item = a.n_items, stop_phase = 0, stop_entry = 0, ovf = -1, status = MM_OK;
    const int n_phase = a.mode == MM_APPLY_FUSE_SIM3 ? 2 : 1;
    for (int i = it0; i < a.n_items && status == MM_OK; i++) {
        const int kf = a.item_kf[i];
        const int b0 = mm_clamp(a.mp_begin[i], 0, a.n_entries), b1 = mm_clamp(a.mp_begin[i + 1], b0, a.n_entries);
        const bool first = i == it0 && resumed;
        int nf = first ? a.n_fused[i] : 0;
        if (kf >= 0 && kf < t.K)
            for (int ph = first ? ph0 : 0; ph < n_phase && status == MM_OK; ph++) {
                const int start = first && ph == ph0 ? (en0 < b1 - b0 ? b0 + en0 : b1) : b0;
                for (int base = start; base < b1 && status == MM_OK; base += g.width) {   // uniform trip count
                    const int m = base + g.lane;
                    const bool hit = m < b1 && (ph == 0 ? a.best_idx[m] >= 0 : a.replace_point[m] >= 0);
                    int total;
                    const int off = g.prefix(hit, total);
                    if (hit) chunk[off] = m;
                    g.sync();
                    for (int c = 0; c < total && status == MM_OK; c++) {
                        const int mc = chunk[c];
                        status = obs_step(g, t, a, kf, ph, mc, flags, ws, nf, ovf);
                        if (status != MM_OK) {
                            stop_item = i;
                            stop_phase = ph;
                            stop_entry = mc - b0;
                        }
                    }
                    g.sync();   // every lane has read the chunk
                }
            }
        if (g.lane == 0) a.n_fused[i] = nf;
    }
    g.sync();
    int at = 0;
    for (int base = 0; base < t.M; base += g.width) {   // uniform trip count
        const int p = base + g.lane;
        const bool flag = p < t.M && flags[p] && !t.mp_bad[p];
        int total;
        const int off = g.prefix(flag, total);
        if (flag) a.touched[at + off] = p;
        at += total;
    }
    for (int p = at + g.lane; p < t.M; p += g.width) a.touched[p] = -1;   // a reader of all M entries skips the padding
    if (g.lane == 0) {
        *a.n_touched = at;
        a.progress[0] = stop_item;
        a.progress[1] = stop_phase;
        a.progress[2] = stop_entry;
        a.progress[3] = ovf;
        *a.status = status;
    }
}

// p's row of the grown CSR: its live entries (mm_cull.h's rule: not -1) in order, then free entries up to `room`.
// out_* may be NULL (count only); nothing is written at or past n_out.  One lane.
MM_HD int obs_grow_point(int n_obs, const int32_t* off, const int32_t* kf, const int32_t* idx, int p, int slack, long long at,
                         int n_out, int32_t* out_kf, int32_t* out_idx) {
    int e0 = off[p], e1 = off[p + 1], n = 0;
    if (e0 < 0) e0 = 0;
    if (e1 > n_obs) e1 = n_obs;
    for (int e = e0; e < e1; e++) {
        if (kf[e] == -1) continue;
        if (out_kf && at + n < n_out) {
            out_kf[at + n] = kf[e];
            out_idx[at + n] = idx[e];
        }
        n++;
    }
    if (out_kf)
        for (int j = 0; j < slack; j++)
            if (at + n + j < n_out) out_kf[at + n + j] = out_idx[at + n + j] = -1;
    return n;
}

}  // namespace orbamd
