// KeyFrame::UpdateConnections with AddConnection / UpdateBestCovisibles (src/KeyFrame.cc:94-119, 235-309) on slot
// tables: which observers count, which counts are pairs, the walk of one target keyframe through a batch and the two
// sorts.  Integer rules only.  Compiles for host and device; every routine is written for a group G of lanes that
// share the work: MmOne (one lane, below) on the CPU, one wavefront in orbmm.hip (the device groups are
// mm_groups.h's).  A group gives lane, width, sync(),
// the reductions sum / min / max over its lanes and prefix(flag, total): the number of set flags on lower lanes.
// Every branch on a reduced value or on a value all lanes load from one address is taken by the whole group.
//
// The counts of an item never depend on the connection state, so the final state of a keyframe X depends only on the
// events that reach X, in batch order: an item that is X replaces X's row by its counter (the own update), an item
// that holds X among its pairs is an AddConnection on X.  mm_walk applies them to a working row; mm_commit sorts once:
// the last event decides whether the ordered row is the item's pairs or the whole row.
#pragma once

#include <cstddef>
#include <cstdint>

#ifndef MM_HD
#if defined(__HIPCC__)
#define MM_HD __host__ __device__ __forceinline__
#else
#define MM_HD inline
#endif
#endif

namespace orbamd {

constexpr int MM_THRESHOLD = 15;   // ORBMM_THRESHOLD
constexpr int MM_COVIS = 10;       // ORBDB_COVIS
constexpr int MM_OK = 0, MM_CONN_OVERFLOW = 1;   // ORBMM_*
constexpr int MM_FORM_NONE = 0, MM_FORM_PAIRS = 1, MM_FORM_ALL = 2;
constexpr int MM_NO_POS = 0x7fffffff;

struct MmGraph {
    int K, M, kf_cap, conn_cap, n_obs;
    const int32_t* kf_id;
    const int32_t* kf_n;
    const int32_t* kf_mappoint;
    const uint8_t* mp_bad;
    const int32_t* mp_obs_off;
    const int32_t* mp_obs_kf;
    int32_t *conn_slot, *conn_weight, *n_conn, *ord_slot, *ord_weight, *n_ord;
    uint8_t* first;
    int32_t *parent, *covis, *status;
};

// What the walk needs of one item's counter.
struct MmItem {
    int32_t kf;         // the item's keyframe; -1 when it is outside the table or its counter is empty
    int32_t any;        // a count reached the threshold
    int32_t max_slot;   // the lowest slot holding the largest count: the only pair when none reached it (:277-293)
    int32_t front;      // the front of the sorted pairs: the largest (count, slot)
    int32_t max_count;
};

struct MmWalk {
    int32_t n, form, own, parent, first, status;
};

struct MmOne {
    static constexpr int lane = 0, width = 1;
    void sync() const {}
    int sum(int v) const { return v; }
    int min(int v) const { return v; }
    int max(int v) const { return v; }
    int prefix(bool flag, int& total) const { total = flag ? 1 : 0; return 0; }
};

MM_HD int mm_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The map point at (k, i) if UpdateConnections walks it (:246-249), or -1.
MM_HD int mm_counted_point(const MmGraph& t, int k, int i) {
    if (i >= mm_clamp(t.kf_n[k], 0, t.kf_cap)) return -1;
    const int p = t.kf_mappoint[(size_t)k * t.kf_cap + i];
    return (p >= 0 && p < t.M && !t.mp_bad[p]) ? p : -1;
}

// Is the observer o counted for keyframe k (:254)?
MM_HD bool mm_counted_observer(const MmGraph& t, int k, int o) { return o >= 0 && o < t.K && t.kf_id[o] != t.kf_id[k]; }

// The observation range of p, clamped to the table.
MM_HD void mm_obs_range(const MmGraph& t, int p, int& e0, int& e1) {
    e0 = t.mp_obs_off[p];
    e1 = t.mp_obs_off[p + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > t.n_obs) e1 = t.n_obs;
}

// std::greater<std::pair<int, KeyFrame*>> with the slot for the pointer
MM_HD bool mm_greater(int w1, int s1, int w2, int s2) { return w1 > w2 || (w1 == w2 && s1 > s2); }

MM_HD bool mm_is_pair(const MmItem& it, int count, int slot) {
    return count >= MM_THRESHOLD || (!it.any && count > 0 && slot == it.max_slot);
}

// cnt: the item's counter over all K slots (0: not a key).
template <class G>
MM_HD MmItem mm_item_summary(const G& g, const int32_t* cnt, int K, int kf) {
    int cmax = 0, lo = MM_NO_POS, hi = -1;
    if (kf >= 0 && kf < K)
        for (int s = g.lane; s < K; s += g.width) {
            const int c = cnt[s];
            if (c > cmax) {
                cmax = c;
                lo = hi = s;
            } else if (c == cmax && c > 0) {
                hi = s;
            }
        }
    const int m = g.max(cmax);
    lo = g.min(cmax == m && m > 0 ? lo : MM_NO_POS);
    hi = g.max(cmax == m && m > 0 ? hi : -1);
    MmItem it;
    it.kf = m > 0 ? kf : -1;
    it.any = m >= MM_THRESHOLD ? 1 : 0;
    it.max_slot = m > 0 ? lo : -1;
    it.front = m > 0 ? (it.any ? hi : lo) : -1;
    it.max_count = m;
    return it;
}

// The events of items[0 .. B) that reach X, applied to the working row ws / ww (conn_cap entries each).  cnt is
// [B][K].  Nothing of the graph is written.
template <class G>
MM_HD MmWalk mm_walk(const G& g, const MmGraph& t, int X, int B, const MmItem* items, const int32_t* cnt, int32_t* ws,
                     int32_t* ww) {
    const int cap = t.conn_cap, K = t.K;
    MmWalk r;
    r.n = mm_clamp(t.n_conn[X], 0, cap);
    r.form = MM_FORM_NONE;
    r.own = -1;
    r.parent = t.parent[X];
    r.first = t.first[X] ? 1 : 0;
    r.status = MM_OK;
    for (int e = g.lane; e < r.n; e += g.width) {
        ws[e] = t.conn_slot[(size_t)X * cap + e];
        ww[e] = t.conn_weight[(size_t)X * cap + e];
    }
    g.sync();
    for (int i = 0; i < B; i++) {
        const MmItem it = items[i];
        if (it.kf < 0) continue;   // KFcounter.empty(): return (:261)
        const int32_t* row = cnt + (size_t)i * K;
        if (it.kf == X) {          // connectionTo_ = KFcounter, the pairs, the parent (:297-308)
            int size = 0;
            for (int s = g.lane; s < K; s += g.width) size += row[s] > 0 ? 1 : 0;
            size = g.sum(size);
            if (size > cap) {
                r.status = MM_CONN_OVERFLOW;
                return r;
            }
            int pos = 0;
            for (int base = 0; base < K; base += g.width) {   // uniform trip count
                const int s = base + g.lane;
                const bool flag = s < K && row[s] > 0;
                int total;
                const int off = g.prefix(flag, total);
                if (flag) {
                    ws[pos + off] = s;
                    ww[pos + off] = row[s];
                }
                pos += total;
            }
            g.sync();
            r.n = size;
            r.form = MM_FORM_PAIRS;
            r.own = i;
            if (r.first && t.kf_id[X] != 0) {
                r.parent = it.front;
                r.first = 0;
            }
        } else {                   // AddConnection(it.kf, c) on X (:94-105)
            const int c = row[X];
            if (!mm_is_pair(it, c, X)) continue;
            int pos = MM_NO_POS;
            for (int e = g.lane; e < r.n; e += g.width)
                if (ws[e] == it.kf) pos = e;
            pos = g.min(pos);
            if (pos < r.n) {
                if (ww[pos] == c) continue;
                g.sync();   // every lane has read ww[pos]
                if (g.lane == 0) ww[pos] = c;
            } else {
                if (r.n == cap) {
                    r.status = MM_CONN_OVERFLOW;
                    return r;
                }
                if (g.lane == 0) {
                    ws[r.n] = it.kf;
                    ww[r.n] = c;
                }
                r.n++;
            }
            r.form = MM_FORM_ALL;
            g.sync();
        }
    }
    return r;
}

// Writes X's rows from a working row of n entries: the connection row ascending by slot, the ordered row descending by
// (weight, slot), each entry placed at its rank (slots are distinct, so ranks are), the padding, kf_covis and both
// counts.  form MM_FORM_ALL orders the whole row (UpdateBestCovisibles), MM_FORM_PAIRS the pairs of `it`.
template <class G>
MM_HD void mm_commit_rows(const G& g, const MmGraph& t, int X, const MmItem& it, int form, const int32_t* ws,
                          const int32_t* ww, int n) {
    const int cap = t.conn_cap;
    int32_t* cs = t.conn_slot + (size_t)X * cap;
    int32_t* cw = t.conn_weight + (size_t)X * cap;
    int32_t* os = t.ord_slot + (size_t)X * cap;
    int32_t* ow = t.ord_weight + (size_t)X * cap;
    int n_ord = 0;
    for (int e = g.lane; e < n; e += g.width) {
        const int s = ws[e], w = ww[e];
        const bool in = form == MM_FORM_ALL || mm_is_pair(it, w, s);
        int below = 0, above = 0;
        for (int j = 0; j < n; j++) {
            const int sj = ws[j], wj = ww[j];
            below += sj < s ? 1 : 0;
            if ((form == MM_FORM_ALL || mm_is_pair(it, wj, sj)) && mm_greater(wj, sj, w, s)) above++;
        }
        cs[below] = s;
        cw[below] = w;
        if (in) {
            os[above] = s;
            ow[above] = w;
            n_ord++;
        }
    }
    n_ord = g.sum(n_ord);
    for (int e = n + g.lane; e < cap; e += g.width) {
        cs[e] = -1;
        cw[e] = 0;
    }
    for (int e = n_ord + g.lane; e < cap; e += g.width) {
        os[e] = -1;
        ow[e] = 0;
    }
    g.sync();
    for (int e = g.lane; e < MM_COVIS; e += g.width) t.covis[(size_t)X * MM_COVIS + e] = e < n_ord ? os[e] : -1;
    if (g.lane == 0) {
        t.n_conn[X] = n;
        t.n_ord[X] = n_ord;
    }
}

// Writes X's rows from the walk's working row, and the parent.
template <class G>
MM_HD void mm_commit(const G& g, const MmGraph& t, int X, const MmItem* items, const int32_t* ws, const int32_t* ww,
                     const MmWalk& r) {
    if (g.lane == 0) t.status[X] = r.status;
    if (r.status != MM_OK || r.form == MM_FORM_NONE) return;
    MmItem it;
    it.kf = -1; it.any = 1; it.max_slot = -1; it.front = -1; it.max_count = 0;
    if (r.form == MM_FORM_PAIRS) it = items[r.own];
    mm_commit_rows(g, t, X, it, r.form, ws, ww, r.n);
    if (g.lane == 0) {
        t.parent[X] = r.parent;
        t.first[X] = r.first ? 1 : 0;
    }
}

}  // namespace orbamd
