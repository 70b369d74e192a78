// orbx_quadtree.h — stage 3 of orbx.hip: QuadTreeSuppression (:542-693) with the reference's std::list
// order and libstdc++ introsort ties (qt_sort.h).  quadtree_kernel: one workgroup per (frame, level), or
// one wavefront per small level (ORBX_QT_WAVE=1); partitions run wave-parallel, list bookkeeping in LDS.
// qt_sort_test_kernel exposes the sort to tests/test_qt_sort.py.
#pragma once
#include "orbx_geom.h"
#include "qt_sort.h"

namespace orbamd {

struct QtNode {
    short tlx, tly, brx, bry;
    int beg, cnt;
};

__device__ __forceinline__ int kp_x(uint32_t k) { return (int)(k & 0xfff); }
__device__ __forceinline__ int kp_y(uint32_t k) { return (int)((k >> 12) & 0xfff); }
__device__ __forceinline__ int kp_s(uint32_t k) { return (int)(k >> 24); }

// QTreeNode::divide (:404-452): children TL/BR and the stable 4-way split of the node's points.
__device__ __forceinline__ void qt_child_geom(const QtNode& n, int c, QtNode& ch) {
    const int xm = n.tlx + (n.brx - n.tlx + 1) / 2;   // TL.x + RoundUp(0.5*(BR.x-TL.x)), d >= 0
    const int ym = n.tly + (n.bry - n.tly + 1) / 2;
    ch.tlx = (short)((c & 1) ? xm : n.tlx);
    ch.brx = (short)((c & 1) ? n.brx : xm);
    ch.tly = (short)((c & 2) ? ym : n.tly);
    ch.bry = (short)((c & 2) ? n.bry : ym);
}

// One wave splits one node: counts per child (returned) and stable scatter into T.  A node of at
// most 512 points is loaded once (8 independent loads per lane) and split from registers.
__device__ int4 qt_wave_split(const QtNode& n, const uint32_t* __restrict__ P, uint32_t* __restrict__ T) {
    const int xm = n.tlx + (n.brx - n.tlx + 1) / 2;
    const int ym = n.tly + (n.bry - n.tly + 1) / 2;
    int c[4] = {0, 0, 0, 0};
    if (n.cnt <= 512) {
        const int lane = lane_id();
        uint32_t k[8];
        int q[8];
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const int j = 64 * t + lane;
            k[t] = j < n.cnt ? P[n.beg + j] : 0u;
        }
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const int j = 64 * t + lane;
            q[t] = j < n.cnt ? (kp_x(k[t]) < xm ? (kp_y(k[t]) < ym ? 0 : 2) : (kp_y(k[t]) < ym ? 1 : 3)) : -1;
            if (64 * t < n.cnt) {   // wave-uniform
#pragma unroll
                for (int qq = 0; qq < 4; qq++) c[qq] += popc64(__ballot(q[t] == qq));
            }
        }
        int o[4] = {n.beg, n.beg + c[0], n.beg + c[0] + c[1], n.beg + c[0] + c[1] + c[2]};
#pragma unroll
        for (int t = 0; t < 8; t++) {
            if (64 * t >= n.cnt) break;   // wave-uniform
#pragma unroll
            for (int qq = 0; qq < 4; qq++) {
                const unsigned long long m = __ballot(q[t] == qq);
                if (q[t] == qq) T[o[qq] + rank64(m)] = k[t];
                o[qq] += popc64(m);
            }
        }
        return make_int4(c[0], c[1], c[2], c[3]);
    }
    for (int b = 0; b < n.cnt; b += 64) {
        const int j = b + lane_id();
        int q = -1;
        if (j < n.cnt) {
            const uint32_t k = P[n.beg + j];
            q = kp_x(k) < xm ? (kp_y(k) < ym ? 0 : 2) : (kp_y(k) < ym ? 1 : 3);
        }
#pragma unroll
        for (int qq = 0; qq < 4; qq++) c[qq] += popc64(__ballot(q == qq));
    }
    int o[4] = {n.beg, n.beg + c[0], n.beg + c[0] + c[1], n.beg + c[0] + c[1] + c[2]};
    for (int b = 0; b < n.cnt; b += 64) {
        const int j = b + lane_id();
        int q = -1;
        uint32_t k = 0;
        if (j < n.cnt) {
            k = P[n.beg + j];
            q = kp_x(k) < xm ? (kp_y(k) < ym ? 0 : 2) : (kp_y(k) < ym ? 1 : 3);
        }
#pragma unroll
        for (int qq = 0; qq < 4; qq++) {
            const unsigned long long m = __ballot(q == qq);
            if (q == qq) T[o[qq] + rank64(m)] = k;
            o[qq] += popc64(m);
        }
    }
    return make_int4(c[0], c[1], c[2], c[3]);
}

// A 16-lane group splits one node of at most 16 points (group = lane >> 4): the same stable 4-way
// scatter as qt_wave_split with the ballots cut to the group's 16 bits.  Every lane of the
// wavefront must call it (ballots); lanes of a group without a node pass cnt = 0.
template <bool SCATTER = true>
__device__ int4 qt_group16_split(const QtNode& n, int cnt, const uint32_t* __restrict__ P, uint32_t* __restrict__ T) {
    const int lane = lane_id(), sh = lane & 48, gl = lane & 15;
    const unsigned lt16 = (1u << gl) - 1u;
    const int xm = n.tlx + (n.brx - n.tlx + 1) / 2;
    const int ym = n.tly + (n.bry - n.tly + 1) / 2;
    int q = -1;
    uint32_t k = 0;
    if (gl < cnt) {
        k = P[n.beg + gl];
        q = kp_x(k) < xm ? (kp_y(k) < ym ? 0 : 2) : (kp_y(k) < ym ? 1 : 3);
    }
    unsigned m[4];
#pragma unroll
    for (int qq = 0; qq < 4; qq++) m[qq] = (unsigned)(__ballot(q == qq) >> sh) & 0xffffu;
    const int c0 = __popc(m[0]), c1 = __popc(m[1]), c2 = __popc(m[2]), c3 = __popc(m[3]);
    const int o[4] = {n.beg, n.beg + c0, n.beg + c0 + c1, n.beg + c0 + c1 + c2};
    if (SCATTER && q >= 0) T[o[q] + __popc(m[q] & lt16)] = k;
    return make_int4(c0, c1, c2, c3);
}

// quadtree_kernel's block size.  qt_block_split is written for exactly QT_THREADS threads (QT_WAVES
// wavefronts): its child counts are summed from QT_WAVES per-wave partials and its scatter tiles are
// 4 x QT_THREADS points with (u, child, wave) ballot counts.  Round 5's 64-thread experiment
// (ORBX_QT_SMALL=64) broke exactly this: with one wavefront the totals read three stale wave slots,
// the child offsets went wild and T was written out of bounds (the illegal access in
// test_fast_candidates_dense_cells[noise], whose dense root nodes take this split).  The kernel now
// checks its block size on entry and sets FAULT_BLOCK_SIZE instead of running (quadtree_kernel).
constexpr int QT_THREADS = 256, QT_WAVES = QT_THREADS / 64;
static_assert(QT_WAVES == 4, "qt_block_split's scratch layout (sc[16 u + 4 child + wave]) holds 4 wavefronts");
// All threads of the QT_THREADS block split one large node: child counts by a block reduction,
// then the stable scatter in tiles of 4 QT_THREADS points, point u*QT_THREADS + tid of a tile in
// thread tid, its position from the per-(u, child, wave) ballot counts of the tile.  sc: 64 ints of
// LDS scratch.  Every thread must call it; the counts are block-uniform.
// Phase-1 nodes above this size are split by the whole block (round 5: 2048 -> 512, quadtree
// -3 % on pan frames, +0.7 % textured: a level's first pass has a few root nodes of 500-2000
// points, and a wavefront per node left the other wavefronts idle)
#ifndef QT_BIG_DEF
#define QT_BIG_DEF 512
#endif
constexpr int QT_BIG = QT_BIG_DEF;
__device__ int4 qt_block_split(const QtNode& n, const uint32_t* __restrict__ P, uint32_t* __restrict__ T, int* sc) {
    const int tid = threadIdx.x, w = tid >> 6, lane = lane_id();
    const int xm = n.tlx + (n.brx - n.tlx + 1) / 2;
    const int ym = n.tly + (n.bry - n.tly + 1) / 2;
    auto quad = [&](uint32_t k) { return kp_x(k) < xm ? (kp_y(k) < ym ? 0 : 2) : (kp_y(k) < ym ? 1 : 3); };
    int c[4] = {0, 0, 0, 0};
#ifndef QT_BS_CNT
#define QT_BS_CNT 4
#endif
    for (int b = 0; b < n.cnt; b += QT_THREADS * QT_BS_CNT) {   // (the counts: QT_BS_CNT points per thread per round)
        uint32_t k[QT_BS_CNT];
#pragma unroll
        for (int u = 0; u < QT_BS_CNT; u++) {
            const int j = b + QT_THREADS * u + tid;
            k[u] = j < n.cnt ? P[n.beg + j] : 0u;
        }
#pragma unroll
        for (int u = 0; u < QT_BS_CNT; u++) {
            const int q = b + QT_THREADS * u + tid < n.cnt ? quad(k[u]) : -1;
#pragma unroll
            for (int qq = 0; qq < 4; qq++) c[qq] += q == qq;
        }
    }
#pragma unroll
    for (int qq = 0; qq < 4; qq++) {
        const int v = wave_sum_i32(c[qq]);
        if (lane == 0) sc[4 * w + qq] = v;
    }
    __syncthreads();
    int tot[4], o[4];
#pragma unroll
    for (int qq = 0; qq < 4; qq++) tot[qq] = sc[qq] + sc[4 + qq] + sc[8 + qq] + sc[12 + qq];   // QT_WAVES = 4 partials
    o[0] = n.beg;
    o[1] = o[0] + tot[0];
    o[2] = o[1] + tot[1];
    o[3] = o[2] + tot[2];
    __syncthreads();
    for (int b = 0; b < n.cnt; b += 4 * QT_THREADS) {
        uint32_t k[4];
        int q[4];
        unsigned long long m[4];
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const int j = b + QT_THREADS * u + tid;
            k[u] = j < n.cnt ? P[n.beg + j] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            q[u] = b + QT_THREADS * u + tid < n.cnt ? quad(k[u]) : -1;
            m[u] = 0;
#pragma unroll
            for (int qq = 0; qq < 4; qq++) {
                const unsigned long long bm = __ballot(q[u] == qq);
                if (q[u] == qq) m[u] = bm;
                if (lane == 0) sc[16 * u + 4 * qq + w] = popc64(bm);   // (u, child, wave)
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < 4; u++) {
            if (q[u] < 0) continue;
            const int* cq = sc + 4 * q[u];
            int off = o[q[u]];
            for (int uu = 0; uu < u; uu++) off += cq[16 * uu] + cq[16 * uu + 1] + cq[16 * uu + 2] + cq[16 * uu + 3];
            for (int ww = 0; ww < w; ww++) off += cq[16 * u + ww];
            T[off + rank64(m[u])] = k[u];
        }
#pragma unroll
        for (int qq = 0; qq < 4; qq++)
#pragma unroll
            for (int u = 0; u < 4; u++)
                o[qq] += sc[16 * u + 4 * qq] + sc[16 * u + 4 * qq + 1] + sc[16 * u + 4 * qq + 2] + sc[16 * u + 4 * qq + 3];
        __syncthreads();
    }
    return make_int4(tot[0], tot[1], tot[2], tot[3]);
}

// Child counts of one node by a single thread (phase 2 only needs the counts of every divisible
// node to find where to stop; only the processed prefix is then split for real); 8 loads in flight.
__device__ __forceinline__ int4 qt_thread_count(const QtNode& n, const uint32_t* __restrict__ P) {
    const int xm = n.tlx + (n.brx - n.tlx + 1) / 2;
    const int ym = n.tly + (n.bry - n.tly + 1) / 2;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    for (int j0 = 0; j0 < n.cnt; j0 += 8) {
        uint32_t kk[8];
#pragma unroll
        for (int u = 0; u < 8; u++) kk[u] = j0 + u < n.cnt ? P[n.beg + j0 + u] : 0u;
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t k = kk[u];
            const bool in = j0 + u < n.cnt;
            const bool r = kp_x(k) >= xm, d = kp_y(k) >= ym;
            c0 += in && !r && !d;
            c1 += in && r && !d;
            c2 += in && !r && d;
            c3 += in && r && d;
        }
    }
    return make_int4(c0, c1, c2, c3);
}

__device__ __forceinline__ int ne4(int4 c) { return (c.x > 0) + (c.y > 0) + (c.z > 0) + (c.w > 0); }
__device__ __forceinline__ int dv4(int4 c) { return (c.x > 1) + (c.y > 1) + (c.z > 1) + (c.w > 1); }
__device__ __forceinline__ int c4(int4 c, int i) { return i == 0 ? c.x : i == 1 ? c.y : i == 2 ? c.z : c.w; }

// Appends item `j`'s children into the new list (group position `gpos`, children in push_front
// order c3..c0) and its divisible children into `divs` at `dpos` (child order c0..c3).
__device__ __forceinline__ void qt_emit_children(const QtNode& parent, int4 cc, int gpos, int dpos, QtNode* nb,
                                                 QtItem* divs, int NC) {
    int pos = gpos;
    for (int c = 3; c >= 0; c--) {
        const int n = c4(cc, c);
        if (n <= 0) continue;
        QtNode ch;
        qt_child_geom(parent, c, ch);
        int off = 0;
        for (int q = 0; q < c; q++) off += c4(cc, q);
        ch.beg = parent.beg + off;
        ch.cnt = n;
        if (pos < NC) nb[pos] = ch;
        pos++;
    }
    // positions: child c sits at gpos + #{nonempty c' > c}
    int d = dpos;
    for (int c = 0; c < 4; c++) {
        const int n = c4(cc, c);
        if (n <= 1) continue;
        int above = 0;
        for (int q = c + 1; q < 4; q++) above += c4(cc, q) > 0;
        if (d < NC) divs[d] = QtItem{n, gpos + above};
        d++;
    }
}

#ifndef QT_STAMP_LEVEL
#define QT_STAMP_LEVEL 0   // the level whose frame-0 workgroup records the phase stamps (ORB_QT_STAMPS)
#endif
#ifdef ORB_QT_STAMPS
__device__ unsigned long long g_qt_stamps[64];
__device__ unsigned long long g_qt_wg[4096 * 2];   // per (frame, level) WG: start, end
#define QT_STAMP(k)                                                                                \
    do {                                                                                           \
        if (blockIdx.x == 0 && lev0 + (int)blockIdx.y == QT_STAMP_LEVEL && threadIdx.x == 0 && (k) < 64)\
            g_qt_stamps[(k)] = __builtin_amdgcn_s_memtime();                                       \
    } while (0)
#ifndef QT_SUB_ITER
#define QT_SUB_ITER 5   // the phase-1 pass whose sub-phases are stamped (56-59)
#endif
#define QT_SUBSTAMP(k)                                                                             \
    do {                                                                                           \
        if (iter_no == QT_SUB_ITER + 1) QT_STAMP(k);                                               \
    } while (0)
#else
#define QT_SUBSTAMP(k) \
    do {               \
    } while (0)
#define QT_STAMP(k) \
    do {            \
    } while (0)
#endif


// std::sort(a, a+n, size-descending) as qt_sort_parallel_form() (qt_sort.h): each Hoare partition
// computed from ballot-compacted stopper lists by one wavefront.  Segments of one recursion round are disjoint
// and a partition (or the depth-0 heap sort) only moves items inside its own segment, so the
// rounds run one after another and a round's segments in parallel, one wavefront each; the
// result is identical to the sequential order.  All threads of the block must call it.
// Scratch: Ls, Rs, seg_lo, seg_len (n ints each), tmp (n items), lists (6 * list_cap ints),
// s_cnt (2 shared ints).  list_cap >= n / 17 + 1.
template <bool WV>
__device__ void qt_sort_block(QtItem* a, int n, int* Ls, int* Rs, int* seg_lo, int* seg_len, QtItem* tmp,
                              int* lists, int list_cap, int* s_cnt) {
    const int lane = lane_id(), w = WV ? 0 : (int)(threadIdx.x >> 6), nw = WV ? 1 : (int)(blockDim.x >> 6);
    const int gtid = WV ? lane : (int)threadIdx.x, gbd = WV ? 64 : (int)blockDim.x;
    if (n <= 0) return;
    int* cur = lists;
    int* nxt = lists + 3 * list_cap;
    if (gtid == 0) {
        s_cnt[0] = 0;
        s_cnt[1] = 0;
        if (n > 16) {
            cur[0] = 0; cur[1] = n; cur[2] = 2 * qt_lg(n);
            s_cnt[0] = 1;
        }
    }
    if (n <= 16)
        for (int i = gtid; i < n; i += gbd) { seg_lo[i] = 0; seg_len[i] = n; }
    qt_sync<WV>();
    while (true) {
        const int nc = s_cnt[0];
        if (nc == 0) break;
        for (int si = w; si < nc; si += nw) {
            const int lo = cur[3 * si], hi = cur[3 * si + 1];
            int depth = cur[3 * si + 2];
            if (depth == 0) {
                if (lane == 0) qt_heap_sort(a + lo, a + hi);
                for (int i = lo + lane; i < hi; i += 64) { seg_lo[i] = lo; seg_len[i] = -1; }
                wave_lds_sync();
                continue;
            }
            --depth;
            const int mid = lo + (hi - lo) / 2;
            if (lane == 0) qt_median_to_first(a + lo, a + lo + 1, a + mid, a + hi - 1);
            wave_lds_sync();
            const int pv = a[lo].size;
            int nl = 0, nr = 0;
            for (int base = lo + 1; base < hi; base += 64) {
                const int i = base + lane;
                const bool f = i < hi && a[i].size <= pv;
                const unsigned long long m = __ballot(f);
                if (f) Ls[lo + nl + rank64(m)] = i;
                nl += popc64(m);
            }
            for (int base = hi - 1; base >= lo; base -= 64) {
                const int j = base - lane;
                const bool f = j >= lo && a[j].size >= pv;
                const unsigned long long m = __ballot(f);
                if (f) Rs[lo + nr + rank64(m)] = j;
                nr += popc64(m);
            }
            wave_lds_sync();
            const int mn = min(nl, nr);
            int K = 0;
            for (int kb = 0; kb < mn; kb += 64) {
                const int k = kb + lane;
                const unsigned long long m = __ballot(k < mn && Ls[lo + k] < Rs[lo + k]);
                K += popc64(m);
                if (m != ~0ull) break;   // the predicate holds on a prefix of k
            }
            for (int k = lane; k < K; k += 64) {
                const int li = Ls[lo + k], ri = Rs[lo + k];
                const QtItem x = a[li], y = a[ri];
                a[li] = y;
                a[ri] = x;
            }
            wave_lds_sync();
            int cut;
            if (K == 0) cut = Ls[lo];
            else {
                const int c1 = K < nl ? Ls[lo + K] : hi;
                const int c2 = Rs[lo + K - 1];
                cut = c1 < c2 ? c1 : c2;
            }
            // children: > 16 go to the next round, the rest are final segments now
            const int clo[2] = {lo, cut}, chi[2] = {cut, hi};
#pragma unroll
            for (int c = 0; c < 2; c++) {
                if (chi[c] - clo[c] > 16) {
                    if (lane == 0) {
                        const int idx = atomicAdd(&s_cnt[1], 1);
                        nxt[3 * idx] = clo[c]; nxt[3 * idx + 1] = chi[c]; nxt[3 * idx + 2] = depth;
                    }
                } else {
                    for (int i = clo[c] + lane; i < chi[c]; i += 64) { seg_lo[i] = clo[c]; seg_len[i] = chi[c] - clo[c]; }
                }
            }
            wave_lds_sync();
        }
        qt_sync<WV>();
        if (gtid == 0) {
            s_cnt[0] = s_cnt[1];
            s_cnt[1] = 0;
        }
        int* t = cur; cur = nxt; nxt = t;
        qt_sync<WV>();
    }
    // final insertion pass == stable sort inside each final segment
    for (int i = gtid; i < n; i += gbd) {
        const QtItem v = a[i];
        if (seg_len[i] < 0) { tmp[i] = v; continue; }
        const int lo = seg_lo[i], hi = lo + seg_len[i];
        int r = 0;
        for (int j = lo; j < hi; j++) {
            const int sj = a[j].size;
            r += (sj > v.size) || (sj == v.size && j < i);
        }
        tmp[lo + r] = v;
    }
    qt_sync<WV>();
    for (int i = gtid; i < n; i += gbd) a[i] = tmp[i];
    qt_sync<WV>();
}

#ifndef QT_WAVES_DEF
#define QT_WAVES_DEF 4   // wavefronts per SIMD = workgroups per CU (4 wavefronts each)
#endif
// per node: na, nb (QtNode), cc (int4), divs, prev (QtItem), ia, ib (int) -- the host sizes the LDS with it
constexpr int QT_NODE_BYTES = 2 * (int)sizeof(QtNode) + (int)sizeof(int4) + 2 * (int)sizeof(QtItem) + 2 * (int)sizeof(int);
template <bool WV>
__global__ __launch_bounds__(QT_THREADS, QT_WAVES_DEF) void quadtree_kernel(Geom g, const int* __restrict__ cell_cnt,
                                                       const uint32_t* __restrict__ slots, const CellDev* cells,
                                                       uint32_t* __restrict__ Pbuf, uint32_t* __restrict__ Tbuf,
                                                       uint32_t* __restrict__ sel, int* __restrict__ sel_cnt, int NC,
                                                       int PTC, uint32_t* fault, int lev0, int nlev) {
    extern __shared__ __attribute__((aligned(16))) char smem_all[];
    // WV: wavefront q of the workgroup runs level lev0 + 4 blockIdx.y + q on its own LDS slice and its
    // own copy of the shared scalars; otherwise the workgroup runs level lev0 + blockIdx.y
    const int wslot = WV ? (int)(threadIdx.x >> 6) : 0;
    char* smem = smem_all + (WV ? (size_t)wslot * ((size_t)NC * QT_NODE_BYTES + (size_t)PTC * 8) : 0);
    QtNode* na = reinterpret_cast<QtNode*>(smem);
    QtNode* nb = na + NC;
    int4* cc = reinterpret_cast<int4*>(nb + NC);
    QtItem* divs = reinterpret_cast<QtItem*>(cc + NC);
    QtItem* prev = divs + NC;
    int* ia = reinterpret_cast<int*>(prev + NC);    // per-node scratch (flags / positions)
    int* ib = ia + NC;
    uint32_t* lds_P = reinterpret_cast<uint32_t*>(ib + NC);   // candidate arrays when they fit
    uint32_t* lds_T = lds_P + PTC;
    constexpr int NSC = WV ? QT_WAVES : 1;
    __shared__ int tmp_a[NSC][16];
    __shared__ int s_sc[NSC][8];
    __shared__ int s_sortcnt_a[NSC][2];
    __shared__ int s_split[64];
    __shared__ int rc_a[NSC][MAX_ROOTS];
    int* tmp = tmp_a[wslot];
    int& s_n = s_sc[wslot][0];
    int& s_ndiv = s_sc[wslot][1];
    int& s_state = s_sc[wslot][2];
    int& s_proc = s_sc[wslot][3];
    int& s_fail = s_sc[wslot][4];
    int& s_anybig = s_sc[wslot][5];
    int* s_sortcnt = s_sortcnt_a[wslot];
    int* rc = rc_a[wslot];

    const int f = blockIdx.x, l = WV ? lev0 + 4 * (int)blockIdx.y + wslot : lev0 + (int)blockIdx.y;
    if (blockDim.x != QT_THREADS) {   // block-uniform: a launch this kernel is not written for fails loudly
        if (threadIdx.x == 0) {
            atomicOr(fault, FAULT_BLOCK_SIZE);
            // describe then sees empty levels, never stale selections (WV: all four of the group)
            for (int q = 0; q < (WV ? 4 : 1); q++) {
                const int lq = WV ? lev0 + 4 * (int)blockIdx.y + q : l;
                if (!WV || lq < lev0 + nlev) sel_cnt[f * g.nlevels + lq] = 0;
            }
        }
        return;
    }
    if (WV && l >= lev0 + nlev) return;   // (wave-uniform; no workgroup barrier in this form)
    int* scnt = sel_cnt + f * g.nlevels + l;
    const LevelDev& L = g.lv[l];
    const int qtid = WV ? lane_id() : (int)threadIdx.x;   // thread index within the tree's group
    constexpr int QBD = WV ? 64 : QT_THREADS;               // the group's size
    const int w = WV ? 0 : (int)(threadIdx.x >> 6), nw = WV ? 1 : QT_WAVES;
    if (L.rw <= 0 || L.rh <= 0 || L.ncells == 0) {
        if (qtid == 0) *scnt = 0;
        return;
    }
    uint32_t* P = Pbuf + (long long)f * g.cand_frame + L.cand_base;
    uint32_t* T = Tbuf + (long long)f * g.cand_frame + L.cand_base;
    uint32_t* gP = P;
    const int* ccell = cell_cnt + (long long)f * g.ncells_total + L.cell_base;
    const uint32_t* fslots = slots + (long long)f * g.slot_frame;

    QT_STAMP(0);
    int p2_round = 0;
    (void)p2_round;
#ifdef ORB_QT_STAMPS
    const unsigned long long qt_t0 = __builtin_amdgcn_s_memtime();
#endif
    // ---- gather candidates in cell raster order (DetectFAST push_back order).  Pass 1: total count;
    //      the arrays live in LDS when they fit.  Pass 2: one lane per cell copies its points.
    // Root id of a keypoint (:562-569): (int)(((float)x - roi.x) / hx) in double; monotone in x.
    const int R = L.nroots;
    auto root_x = [&](int x) -> int {
        const float dx = (float)x - (float)L.rx;   // keypoint.pt.x - roi.x (float)
        return (int)((double)dx / L.hx);
    };
    if (qtid < MAX_ROOTS) rc[qtid] = 0;
    if (qtid == 0) s_fail = 0;
    int n_total = 0, carry = 0;
    bool parted = false;   // the gather below writes the root-partitioned order itself (round 5)
    if (L.ncells <= 4 * QBD && R <= 4) {
        // thread t owns cells cpt t .. cpt t + cpt - 1 (raster order): their counts and slot offsets are loaded
        // together and the points go straight to their root's segment.  A cell whose zone lies inside
        // one root (all but the cells on a root boundary) sends all its points there, a boundary cell
        // splits them by x; one block scan per root (R <= 4) of the threads' counts places the threads'
        // runs, so each segment keeps the gather order: the stable partition of :547-579 without the
        // round trip through T.  Every thread's first 8 points per cell are loaded in one batch.
        // Cells per thread: as few as the grid allows (a small level's 100-500 cells over 1-2 per
        // thread instead of 4), so a thread's chain of dependent slot loads is shorter (round 5);
        // thread order is still cell order.
        const int cpt = (L.ncells + QBD - 1) / QBD;   // 1..4
        const int i0 = cpt * qtid;
        int cv[4], cs[4], rl[4], rh[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = i0 + k;
            cv[k] = 0; cs[k] = 0; rl[k] = 0; rh[k] = 0;
            if (k < cpt && i < L.ncells) {
                const CellDev cd = cells[L.cell_base + i];
                cv[k] = ccell[i] & CELL_CNT_MASK;
                cs[k] = cd.slot;
                const int zx = (cd.x0y0 & 0xffff) + 3;            // the zone's first column
                rl[k] = root_x(zx);
                rh[k] = root_x(zx + (cd.zwzh & 0xffff) - 1);     // and its last
            }
        }
        bool bad = false;
#pragma unroll
        for (int k = 0; k < 4; k++) bad |= cv[k] > 0 && (rl[k] < 0 || rh[k] >= R);
        if (bad) atomicOr(fault, FAULT_QT_ROOT);
        int cnt[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (rl[k] == rh[k]) {
#pragma unroll
                for (int rt = 0; rt < 4; rt++) cnt[rt] += rl[k] == rt ? cv[k] : 0;
            } else {   // a boundary cell (rare): its points' roots
                for (int q = 0; q < cv[k]; q++) {
                    const int rt = root_x(kp_x(fslots[cs[k] + q]));
#pragma unroll
                    for (int u = 0; u < 4; u++) cnt[u] += rt == u;
                }
            }
        }
        int run[4];
        int base = 0;
#pragma unroll
        for (int rt = 0; rt < 4; rt++) {
            if (rt >= R) { run[rt] = 0; continue; }   // block-uniform
            int tot;
            run[rt] = base + grp_excl_scan<WV>(cnt[rt], tmp, &tot);
            if (qtid == 0) rc[rt] = tot;
            base += tot;
        }
        n_total = base;
        if (n_total <= PTC) { P = lds_P; T = lds_T; }
        uint32_t r[4][8];
#pragma unroll
        for (int k = 0; k < 4; k++)
#pragma unroll
            for (int q = 0; q < 8; q++) r[k][q] = q < cv[k] ? fslots[cs[k] + q] : 0u;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (rl[k] == rh[k]) {
                int o = run[0];
#pragma unroll
                for (int rt = 1; rt < 4; rt++) o = rl[k] == rt ? run[rt] : o;
#pragma unroll
                for (int q = 0; q < 8; q++)
                    if (q < cv[k]) P[o + q] = r[k][q];
                for (int q0 = 8; q0 < cv[k]; q0 += 8) {   // > 8 points in a cell: batches of 8 loads
                    uint32_t r2[8];
#pragma unroll
                    for (int q = 0; q < 8; q++) r2[q] = q0 + q < cv[k] ? fslots[cs[k] + q0 + q] : 0u;
#pragma unroll
                    for (int q = 0; q < 8; q++)
                        if (q0 + q < cv[k]) P[o + q0 + q] = r2[q];
                }
#pragma unroll
                for (int rt = 0; rt < 4; rt++) run[rt] += rl[k] == rt ? cv[k] : 0;
            } else {
                for (int q = 0; q < cv[k]; q++) {
                    const uint32_t kk = fslots[cs[k] + q];
                    const int rt = root_x(kp_x(kk));
                    int o = run[0];
#pragma unroll
                    for (int u = 1; u < 4; u++) o = rt == u ? run[u] : o;
                    P[o] = kk;
#pragma unroll
                    for (int u = 0; u < 4; u++) run[u] += rt == u;
                }
            }
        }
        carry = n_total;
        parted = true;
    } else if (L.ncells <= 4 * QBD) {
        // (more than 4 roots: an aspect ratio above 4.5) the gather in raster order, partitioned below
        const int i0 = 4 * qtid;
        int cv[4], cs[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int i = i0 + k;
            cv[k] = i < L.ncells ? ccell[i] & CELL_CNT_MASK : 0;
            cs[k] = i < L.ncells ? cells[L.cell_base + i].slot : 0;
        }
        const int sum = cv[0] + cv[1] + cv[2] + cv[3];
        const int ex = grp_excl_scan<WV>(sum, tmp, &n_total);
        if (n_total <= PTC) { P = lds_P; T = lds_T; }
        int o = ex;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            for (int q0 = 0; q0 < cv[k]; q0 += 8) {
                uint32_t r2[8];
#pragma unroll
                for (int q = 0; q < 8; q++) r2[q] = q0 + q < cv[k] ? fslots[cs[k] + q0 + q] : 0u;
#pragma unroll
                for (int q = 0; q < 8; q++)
                    if (q0 + q < cv[k]) P[o + q0 + q] = r2[q];
            }
            o += cv[k];
        }
        carry = n_total;
    } else {
        {
            int part = 0;
            for (int i = qtid; i < L.ncells; i += QBD) part += ccell[i] & CELL_CNT_MASK;
            part = wave_sum_i32(part);
            if (lane_id() == 0) tmp[8 + w] = part;
            qt_sync<WV>();
            for (int q = 0; q < nw; q++) n_total += tmp[8 + q];
            qt_sync<WV>();
        }
        if (n_total <= PTC) { P = lds_P; T = lds_T; }
        for (int b = 0; b < L.ncells; b += QBD) {
            const int i = b + qtid;
            const int v = i < L.ncells ? ccell[i] & CELL_CNT_MASK : 0;
            int tot;
            const int ex = grp_excl_scan<WV>(v, tmp, &tot);
            if (v > 0) {
                const uint32_t* __restrict__ src = fslots + cells[L.cell_base + i].slot;
                uint32_t* dst = P + carry + ex;
                for (int j0 = 0; j0 < v; j0 += 8) {
                    uint32_t r[8];
#pragma unroll
                    for (int q = 0; q < 8; q++) r[q] = j0 + q < v ? src[j0 + q] : 0;
#pragma unroll
                    for (int q = 0; q < 8; q++)
                        if (j0 + q < v) dst[j0 + q] = r[q];
                }
            }
            carry += tot;
        }
    }
    qt_sync<WV>();
    const int n_src = carry;
    if (WV && !parted) {   // the host sends only levels the partitioned gather takes (<= 256 cells, <= 4 roots)
        if (qtid == 0) {
            atomicOr(fault, FAULT_BLOCK_SIZE);
            *scnt = 0;
        }
        return;
    }
    QT_STAMP(1);
    if (n_src == 0) {
        if (qtid == 0) *scnt = 0;
        return;
    }
    qt_sync<WV>();

    // ---- root nodes (:547-579): stable partition by root id (the large-grid gather's order; the
    //      small-grid gather above wrote the partitioned order itself)
    if (!parted) {   // block-uniform
    auto root_of = [&](uint32_t k) -> int { return root_x(kp_x(k)); };
    // every wave partitions a contiguous quarter (root ids kept in registers between the passes);
    // quarter q's base offset per root = that root's count over quarters < q -> stable overall
    __shared__ int s_rcnt[4][MAX_ROOTS];
    constexpr int QT_RPL = 32;   // points per lane held in registers (fallback loop past that)
    const int qlen = (n_src + nw - 1) / nw;
    const int q0 = min(n_src, w * qlen), q1 = min(n_src, q0 + qlen);
    int rid[QT_RPL];
    {
        int counts[MAX_ROOTS];
        for (int r = 0; r < R; r++) counts[r] = 0;
#pragma unroll
        for (int t = 0; t < QT_RPL; t++) {
            if (q0 + 64 * t >= q1) { rid[t] = -1; continue; }   // wave-uniform: past this quarter
            const int j = q0 + 64 * t + lane_id();
            int r = -1;
            if (j < q1) {
                r = root_of(P[j]);
                if (r < 0 || r >= R) atomicOr(fault, FAULT_QT_ROOT);
            }
            rid[t] = r;
            for (int q = 0; q < R; q++) counts[q] += popc64(__ballot(r == q));
        }
        for (int b = q0 + 64 * QT_RPL; b < q1; b += 256) {   // quarters longer than 64*QT_RPL points
            uint32_t kk[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = b + 64 * u + lane_id();
                kk[u] = j < q1 ? P[j] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = b + 64 * u + lane_id();
                const int r = j < q1 ? root_of(kk[u]) : -1;
                for (int q = 0; q < R; q++) counts[q] += popc64(__ballot(r == q));
            }
        }
        if (lane_id() == 0)
            for (int q = 0; q < R; q++) s_rcnt[w][q] = counts[q];
    }
    qt_sync<WV>();
    {
        int o[MAX_ROOTS];
        int acc = 0;
        for (int q = 0; q < R; q++) {
            int before = 0, tot = 0;
            for (int v = 0; v < nw; v++) {
                tot += s_rcnt[v][q];
                if (v < w) before += s_rcnt[v][q];
            }
            o[q] = acc + before;
            acc += tot;
            if (qtid == 0) rc[q] = tot;
        }
#pragma unroll
        for (int t = 0; t < QT_RPL; t++) {
            if (q0 + 64 * t >= q1) continue;   // wave-uniform
            const int j = q0 + 64 * t + lane_id();
            const uint32_t k = j < q1 ? P[j] : 0;
            const int r = rid[t];
            for (int q = 0; q < R; q++) {
                const unsigned long long m = __ballot(r == q);
                if (r == q) T[o[q] + rank64(m)] = k;
                o[q] += popc64(m);
            }
        }
        for (int b = q0 + 64 * QT_RPL; b < q1; b += 256) {
            uint32_t kk[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = b + 64 * u + lane_id();
                kk[u] = j < q1 ? P[j] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int j = b + 64 * u + lane_id();
                const uint32_t k = kk[u];
                const int r = j < q1 ? root_of(k) : -1;
                for (int q = 0; q < R; q++) {
                    const unsigned long long m = __ballot(r == q);
                    if (r == q) T[o[q] + rank64(m)] = k;
                    o[q] += popc64(m);
                }
            }
        }
    }
    qt_sync<WV>();
    {   // the partitioned copy becomes P (every thread swaps the same pointers)
        uint32_t* t = P;
        P = T;
        T = t;
    }
    }   // !parted
    if (qtid == 0) {
        int n = 0, acc = 0;
        for (int q = 0; q < R; q++) {
            if (rc[q] > 0) {
                QtNode r;
                r.tlx = (short)(int)(L.rx + L.hx * q);
                r.tly = (short)L.ry;
                r.brx = (short)(int)(L.rx + L.hx * (q + 1));
                r.bry = (short)(L.ry + L.rh);
                r.beg = acc;
                r.cnt = rc[q];
                na[n++] = r;
            }
            acc += rc[q];
        }
        s_n = n;
        s_state = 0;   // 0 = phase 1, 1 = phase 2, 2 = finished
        s_ndiv = 0;
        s_anybig = 0;
    }
    qt_sync<WV>();

    const int nfeat = L.quota;
    QT_STAMP(2);
    int iter_no = 0;
    (void)iter_no;
    (void)gP;
    // ---- main loop
    while (true) {
        const int n = s_n;
        const int state = s_state;
        QT_STAMP(3 + 2 * iter_no);
        if (qtid == 0 && blockIdx.x == 0 && l == QT_STAMP_LEVEL) {
#ifdef ORB_QT_STAMPS
            if (4 + 2 * iter_no < 60) g_qt_stamps[4 + 2 * iter_no] = ((unsigned long long)state << 32) | (unsigned)n;
#endif
        }
        iter_no++;
        if (state == 2) break;
        if (state == 0) {
            // Phase 1 pass (:588-630): split every divisible node in list order.
            // D positions via compaction
            int kdiv = 0, nnd = 0;   // (s_anybig was cleared before the last barrier)
            for (int b = 0; b < n; b += QBD) {
                const int i = b + qtid;
                const int dvf = (i < n && na[i].cnt > 1) ? 1 : 0;
                if (!WV && i < n && na[i].cnt > QT_BIG) s_anybig = 1;   // (WV: one wavefront per tree, no block split)
                int tot;
                const int ex = grp_excl_scan<WV>(dvf, tmp, &tot);
                if (i < n) {
                    if (dvf) ia[kdiv + ex] = i;               // D: divisible, processing order
                    else ib[i] = nnd + (i - b - ex);          // rank among non-divisible
                }
                nnd += min(QBD, n - b) - tot;
                kdiv += tot;
            }
            qt_sync<WV>();
            QT_SUBSTAMP(56);
            // nodes of <= 16 points: four per wavefront (16-lane groups); larger: one wavefront each
            for (int b = 4 * w; b < kdiv; b += 4 * nw) {   // wave-uniform trip count
                const int j = b + (lane_id() >> 4);
                QtNode nd{};
                int cnt = 0;
                if (j < kdiv) {
                    nd = na[ia[j]];
                    cnt = nd.cnt <= 16 ? nd.cnt : 0;
                }
                const int4 c = qt_group16_split(nd, cnt, P, T);
                if (cnt > 0 && (lane_id() & 15) == 0) cc[j] = c;
            }
            for (int j = w; j < kdiv; j += nw) {
                const int cn = na[ia[j]].cnt;
                if (cn <= 16 || (!WV && cn > QT_BIG)) continue;   // wave-uniform
                const int4 c = qt_wave_split(na[ia[j]], P, T);
                if (lane_id() == 0) cc[j] = c;
            }
            if (!WV && s_anybig) {   // block-uniform (set before the scans' barriers)
                for (int j = 0; j < kdiv; j++) {
                    if (na[ia[j]].cnt <= QT_BIG) continue;   // block-uniform
                    const int4 c = qt_block_split(na[ia[j]], P, T, s_split);
                    if (qtid == 0) cc[j] = c;
                }
            }
            qt_sync<WV>();
            QT_SUBSTAMP(57);
            // group positions: reverse processing order; divisibles: forward order.  The ne and dv counts
            // share one block scan (16-bit halves: a chunk's totals are <= 4 blockDim); with one chunk
            // (kdiv <= blockDim, every small level) the scan's total is the grand total the reverse
            // order needs, so the separate total pass and its two barriers are skipped (round 5)
            int ne_carry = 0, dv_carry = 0, ne_total = 0;
            if (kdiv > QBD) {   // block-uniform
                int part = 0;
                for (int j = qtid; j < kdiv; j += QBD) part += ne4(cc[j]);
                part = wave_sum_i32(part);
                if (lane_id() == 0) tmp[8 + w] = part;
                qt_sync<WV>();
                for (int q = 0; q < nw; q++) ne_total += tmp[8 + q];
                qt_sync<WV>();
            }
            for (int b = 0; b < kdiv; b += QBD) {
                const int j = b + qtid;
                const int4 c = j < kdiv ? cc[j] : make_int4(0, 0, 0, 0);
                int tt;
                const int ex = grp_excl_scan<WV>(ne4(c) | (dv4(c) << 16), tmp, &tt);
                const int t1 = tt & 0xffff, t2 = tt >> 16, ex_ne = ex & 0xffff, ex_dv = ex >> 16;
                if (kdiv <= QBD) ne_total = t1;
                if (j < kdiv) {
                    const int incl = ne_carry + ex_ne + ne4(c);
                    const int gpos = ne_total - incl;   // sum of ne over items after j
                    qt_emit_children(na[ia[j]], c, gpos, dv_carry + ex_dv, nb, divs, NC);
                }
                ne_carry += t1;
                dv_carry += t2;
            }
            const int n_new = ne_total + nnd;
            QT_SUBSTAMP(55);   // (thread 0: its emit done)
            for (int i = qtid; i < n; i += QBD)
                if (na[i].cnt <= 1 && ne_total + ib[i] < NC) nb[ne_total + ib[i]] = na[i];
            // commit: the single points of the non-divisible nodes join the split nodes' points in
            // T, which becomes P (every thread swaps the same pointers)
            for (int i = qtid; i < n; i += QBD)
                if (na[i].cnt == 1) T[na[i].beg] = P[na[i].beg];
            {
                uint32_t* t = P;
                P = T;
                T = t;
            }
            qt_sync<WV>();
            QT_SUBSTAMP(58);
            if (qtid == 0) {
                if (n_new > NC) { s_fail = 1; atomicOr(fault, FAULT_QT_NODES); }
                s_n = min(n_new, NC);
                s_ndiv = dv_carry;
                s_anybig = 0;
                if (n_new >= nfeat || n_new == n || s_fail) s_state = 2;
                else if (n_new + 3 * dv_carry > nfeat) s_state = 1;
            }
            qt_sync<WV>();
            QT_SUBSTAMP(59);
            QtNode* t = na; na = nb; nb = t;
        } else {
            // Phase 2 round (:632-672): split the previous round's divisible nodes, largest
            // first (std::sort, emulated), stopping as soon as the list reaches nfeat.
            const int m = s_ndiv;
            for (int j = qtid; j < m; j += QBD) prev[j] = divs[j];
            qt_sync<WV>();
            QT_STAMP(40 + 4 * min(p2_round, 5));
            {
                int* seg = reinterpret_cast<int*>(cc);   // cc (4 NC ints) is free until the splits below
                qt_sort_block<WV>(prev, m, ia, ib, seg, seg + NC, divs, seg + 2 * NC, NC / 3, s_sortcnt);
            }
            QT_STAMP(41 + 4 * min(p2_round, 5));
            for (int j = qtid; j < m; j += QBD) cc[j] = qt_thread_count(na[prev[j].node], P);
            for (int i = qtid; i < n; i += QBD) ia[i] = 0;   // erased flags
            if (qtid == 0) s_proc = m;
            qt_sync<WV>();
            // first sorted item whose split brings the list to nfeat (:666-667), by prefix sums
            {
                int carry2 = 0;
                for (int b = 0; b < m; b += QBD) {
                    const int j = b + qtid;
                    const int d = j < m ? ne4(cc[j]) - 1 : 0;
                    int tot;
                    const int ex = grp_excl_scan<WV>(d, tmp, &tot);
                    if (j < m && n + carry2 + ex + d >= nfeat) atomicMin(&s_proc, j + 1);
                    carry2 += tot;
                }
            }
            qt_sync<WV>();
            const int proc = s_proc;
            QT_STAMP(42 + 4 * min(p2_round, 5));
            for (int j = qtid; j < proc; j += QBD) ia[prev[j].node] = 1;
            // split the processed prefix only: small nodes one thread each, large ones one wave each
            for (int b = 4 * w; b < proc; b += 4 * nw) {   // <= 16 points: 16-lane groups
                const int j = b + (lane_id() >> 4);
                QtNode nd{};
                int cnt = 0;
                if (j < proc) {
                    nd = na[prev[j].node];
                    cnt = nd.cnt <= 16 ? nd.cnt : 0;
                }
                (void)qt_group16_split(nd, cnt, P, T);
            }
            for (int j = w; j < proc; j += nw)
                if (na[prev[j].node].cnt > 16) (void)qt_wave_split(na[prev[j].node], P, T);
            qt_sync<WV>();
            int ne_total = 0;   // (one packed scan; the total pass only for more than one chunk, as phase 1)
            if (proc > QBD) {   // block-uniform
                int part = 0;
                for (int j = qtid; j < proc; j += QBD) part += ne4(cc[j]);
                part = wave_sum_i32(part);
                if (lane_id() == 0) tmp[8 + w] = part;
                qt_sync<WV>();
                for (int q = 0; q < nw; q++) ne_total += tmp[8 + q];
                qt_sync<WV>();
            }
            int ne_carry = 0, dv_carry = 0;
            for (int b = 0; b < proc; b += QBD) {
                const int j = b + qtid;
                const int4 c = j < proc ? cc[j] : make_int4(0, 0, 0, 0);
                int tt;
                const int ex = grp_excl_scan<WV>(ne4(c) | (dv4(c) << 16), tmp, &tt);
                const int t1 = tt & 0xffff, t2 = tt >> 16, ex_ne = ex & 0xffff, ex_dv = ex >> 16;
                if (proc <= QBD) ne_total = t1;
                if (j < proc) {
                    const int gpos = ne_total - (ne_carry + ex_ne + ne4(c));
                    qt_emit_children(na[prev[j].node], c, gpos, dv_carry + ex_dv, nb, divs, NC);
                }
                ne_carry += t1;
                dv_carry += t2;
            }
            // survivors keep their order after the new groups
            int surv = 0;
            for (int b = 0; b < n; b += QBD) {
                const int i = b + qtid;
                const int keep = (i < n && !ia[i]) ? 1 : 0;
                int tot;
                const int ex = grp_excl_scan<WV>(keep, tmp, &tot);
                if (keep && ne_total + surv + ex < NC) nb[ne_total + surv + ex] = na[i];
                surv += tot;
            }
            for (int j = w; j < proc; j += nw) {
                const QtNode& p = na[prev[j].node];
                for (int q = lane_id(); q < p.cnt; q += 64) P[p.beg + q] = T[p.beg + q];
            }
            qt_sync<WV>();
            if (qtid == 0) {
                const int n_new = ne_total + surv;
                if (n_new > NC) { s_fail = 1; atomicOr(fault, FAULT_QT_NODES); }
                s_n = min(n_new, NC);
                s_ndiv = dv_carry;
                if (n_new >= nfeat || n_new == n || s_fail) s_state = 2;
            }
            qt_sync<WV>();
            QT_STAMP(43 + 4 * min(p2_round, 5));
            p2_round++;
            QtNode* t = na; na = nb; nb = t;
        }
    }

    // ---- retain the best point per node (:677-692): strict '>' => first maximum wins.  One lane
    //      per node (nodes are small at this point).
    const int n = s_n;
    uint32_t* out = sel + (long long)f * g.out_frame + L.out_base;
    if (n > L.out_cap && qtid == 0) atomicOr(fault, FAULT_OUT_CAP);
    for (int i = qtid; i < n && i < L.out_cap; i += QBD) {
        const QtNode nd = na[i];
        int bs = -1;
        uint32_t best = 0;
        for (int j0 = 0; j0 < nd.cnt; j0 += 4) {
            uint32_t r[4];
#pragma unroll
            for (int q = 0; q < 4; q++) r[q] = j0 + q < nd.cnt ? P[nd.beg + j0 + q] : 0;
#pragma unroll
            for (int q = 0; q < 4; q++)
                if (j0 + q < nd.cnt && kp_s(r[q]) > bs) { bs = kp_s(r[q]); best = r[q]; }
        }
        out[i] = best;
    }
    if (qtid == 0) *scnt = min(n, L.out_cap);
    QT_STAMP(63);
#ifdef ORB_QT_STAMPS
    if (qtid == 0 && f * g.nlevels + l < 4096) {
        g_qt_wg[2 * (f * g.nlevels + l)] = qt_t0;
        g_qt_wg[2 * (f * g.nlevels + l) + 1] = __builtin_amdgcn_s_memtime();
    }
#endif
}

__global__ __launch_bounds__(256) void qt_sort_test_kernel(QtItem* items, int n, int* scratch) {
    __shared__ int s_cnt[2];
    qt_sort_block<false>(items, n, scratch, scratch + n, scratch + 2 * n, scratch + 3 * n,
                  reinterpret_cast<QtItem*>(scratch + 4 * n), scratch + 6 * n, n / 3 + 2, s_cnt);
}

}  // namespace orbamd
