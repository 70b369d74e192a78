// ORBmatcher::SearchForInitialization (included by orbp.hip after orbp_grid.h and orbp_host.h).
//
// Reference: src/ORBmatcher.cc:614-694, batched over pairs (F1, F2).
// The reference walks the octave-0 features of F1 in idx1 order against a state over F2
// (matchedDistance, matches21): a candidate idx2 is skipped when the distance it is held at is <=
// its own, and an accepted query takes idx2 from its earlier holder.  Three stages:
//   pj_grid_kernel   F2's FeaturesGrid (orbp_grid.h; mp_begin = q_begin gives each query its pair)
//   pi_score_kernel  a 16-lane group per query: the octave-0 candidates of its window in
//                    GetFeaturesInArea's scan order with their Hamming distances, up to PI_CAP
//   pi_walk_kernel   one wavefront per pair: the queries in order, lanes over a query's candidates
//                    against the state in LDS (matchedDistance u16, matches21 / matches12 i16),
//                    best = min (dist, scan position), second = the second-smallest distance of the
//                    candidates not skipped; windows with more than PI_CAP candidates are rescanned
//                    from the grid.  Then CheckOrientation over every push (stale ones included),
//                    the output and the prevMatched update.
#pragma once

namespace orbamd {

using orbamd_host::PI_CAP;
constexpr int PI_TH_LOW = 50;    // ORBmatcher.cc:42
constexpr int PI_INF = 0xffff;   // matchedDistance = INT_MAX on entry (:618)

struct PiExtra {
    const int32_t* q_begin;
    const int32_t* q_oct;
    const uint8_t* q_desc;
    const float* q_angle;
    const float* kp_angle;
    float* prev;
    float r, nnratio;
    int check_ori, total_q;
    int32_t* cnt;        // total_q: candidates in the query's window (0: not searched / none)
    uint32_t* cand;      // total_q x PI_CAP: (dist << 13 | idx2) in scan order
    int32_t* matches12;  // total_q
};

struct PiWin {
    PjWindow win;   // any: the query searches at all
    int lvl;
    bool chk;
    float u, v, r;
};

// GetFeaturesInArea(u, v, windowSize, level1, level1) (Frame.cc:102-145) of query j (octave <= 0).
__device__ __forceinline__ PiWin pi_window(const PjArgs& a, const PiExtra& e, int f, int j) {
    PiWin w;
    w.lvl = e.q_oct[j];
    w.chk = w.lvl >= 0;   // checkLevels = minLevel > 0 || maxLevel >= 0
    w.u = e.prev[2 * (size_t)j];
    w.v = e.prev[2 * (size_t)j + 1];
    w.r = e.r;
    w.win = pj_window(pj_bounds(a.bounds + 4 * (size_t)f), w.u, w.v, w.r);
    if (!(w.lvl <= 0)) w.win.any = false;   // :628-630: level1 > 0 continue
    return w;
}

// the level / area gates of keypoint idx of frame f (false: not a candidate)
__device__ __forceinline__ bool pi_gate(const PjArgs& a, const PiWin& w, int k0, int idx) {
    const int k = k0 + idx;
    if (w.chk && a.kp_oct[k] != w.lvl) return false;
    return pj_in_box(a.kp_xy[2 * (size_t)k], a.kp_xy[2 * (size_t)k + 1], w.u, w.v, w.r);
}

__global__ __launch_bounds__(256) void pi_score_kernel(PjArgs a, PiExtra e) {
    const int j = blockIdx.x * 16 + (threadIdx.x >> 4), lane = threadIdx.x & 15;
    if (j >= e.total_q) return;   // whole 16-lane groups
    const int f = a.mp_frame[j];
    const int k0 = a.kp_begin[f], n2 = a.kp_begin[f + 1] - k0;
    int cnt = 0;
    if (n2 <= PJ_MAXKP) {
        const PiWin w = pi_window(a, e, f, j);
        if (w.win.any) {
            const uint8_t* d1 = e.q_desc + 32 * (size_t)j;
            const int32_t* cs = a.grid_start + (size_t)f * (PJ_CELLS + 1);
            const int gsh = threadIdx.x & 48;   // this group's bit offset in the wave's ballot
            // Written out, not through pj_scan_window: every lane of the group has to reach the ballot of
            // each 16-position step, also the lanes past the end of the column (p >= p1).
            for (int cx = w.win.mincx; cx <= w.win.maxcx; cx++) {
                const int p0 = cs[cx * PJ_ROWS + w.win.mincy], p1 = cs[cx * PJ_ROWS + w.win.maxcy + 1];
                for (int b = p0; b < p1; b += 16) {
                    const int p = b + lane;
                    int idx = -1;
                    if (p < p1) {
                        idx = a.grid_idx[k0 + p];
                        if (!pi_gate(a, w, k0, idx)) idx = -1;
                    }
                    const unsigned long long bm = __ballot(idx >= 0);
                    const uint32_t gm = (uint32_t)(bm >> gsh) & 0xffffu;
                    if (idx >= 0) {
                        const int pos = cnt + __popc(gm & ((1u << lane) - 1u));
                        if (pos < PI_CAP) {
                            const int dist = pj_hamming(d1, a.kp_desc + 32 * (size_t)(k0 + idx));
                            e.cand[(size_t)j * PI_CAP + pos] = ((uint32_t)dist << PJ_IDX_BITS) | (uint32_t)idx;
                        }
                    }
                    cnt += __popc(gm);
                }
            }
        }
    }
    if (lane == 0) e.cnt[j] = cnt;
}

__device__ __forceinline__ unsigned long long pi_wave_min64(unsigned long long v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        const unsigned lo = (unsigned)__shfl_xor((int)(unsigned)v, m, 64), hi = (unsigned)__shfl_xor((int)(v >> 32), m, 64);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(64) void pi_walk_kernel(PjArgs a, PiExtra e) {
    __shared__ uint16_t mdist[PJ_MAXKP];
    __shared__ int16_t m21[PJ_MAXKP];
    __shared__ int16_t m12[PJ_MAXKP];
    __shared__ int hist[32];
    __shared__ uint32_t keep_s;
    const int f = blockIdx.x, lane = threadIdx.x;
    const int k0 = a.kp_begin[f], n2 = a.kp_begin[f + 1] - k0;
    const int q0 = e.q_begin[f], n1 = e.q_begin[f + 1] - q0;
    if (n1 > PJ_MAXKP || n2 > PJ_MAXKP) {
        for (int i = lane; i < n1; i += 64) e.matches12[q0 + i] = -1;
        if (lane == 0) a.n_matches[f] = -1;
        return;
    }
    for (int i = lane; i < n2; i += 64) { mdist[i] = PI_INF; m21[i] = -1; }
    for (int i = lane; i < n1; i += 64) m12[i] = -1;
    if (lane < 32) hist[lane] = 0;
    __syncthreads();
    const int32_t* cs = a.grid_start + (size_t)f * (PJ_CELLS + 1);
    int nm = 0;
    for (int c = 0; c < n1; c += 64) {
        const int cnt_l = c + lane < n1 ? e.cnt[q0 + c + lane] : 0;
        unsigned long long todo = __ballot(cnt_l > 0);
        while (todo) {
            const int t = __builtin_ctzll(todo);
            todo &= todo - 1;
            const int qi = c + t, j = q0 + qi;
            const int cnt = __shfl(cnt_l, t, 64);
            unsigned long long bkey = ~0ull;   // (dist << 32) | (scan position << 13) | idx2
            int d1 = PI_INF, d2 = PI_INF;      // the lane's two smallest distances not skipped
            auto consider = [&](int dist, int idx2, int pos) {
                if ((int)mdist[idx2] <= dist) return;   // matchedDistance[idx2] <= dist (:650-651)
                const unsigned long long key = ((unsigned long long)dist << 32) | ((unsigned)pos << PJ_IDX_BITS) | (unsigned)idx2;
                bkey = key < bkey ? key : bkey;
                if (dist < d1) { d2 = d1; d1 = dist; } else if (dist < d2) d2 = dist;
            };
            if (cnt <= PI_CAP) {
                for (int k = lane; k < cnt; k += 64) {
                    const uint32_t key = e.cand[(size_t)j * PI_CAP + k];
                    consider((int)(key >> PJ_IDX_BITS), (int)(key & PJ_IDX_MASK), k);
                }
            } else {   // a window with more than PI_CAP candidates: rescan it from the grid
                const PiWin w = pi_window(a, e, f, j);
                const uint8_t* d1p = e.q_desc + 32 * (size_t)j;
                pj_scan_window<64>(w.win, cs, a.grid_idx, k0, lane, [&](int p, int idx) {
                    if (pi_gate(a, w, k0, idx)) consider(pj_hamming(d1p, a.kp_desc + 32 * (size_t)(k0 + idx)), idx, p);
                });
            }
            bkey = pi_wave_min64(bkey);
#pragma unroll
            for (int m = 32; m > 0; m >>= 1) {   // merge the lanes' two smallest: second order statistic
                const int o1 = __shfl_xor(d1, m, 64), o2 = __shfl_xor(d2, m, 64);
                d2 = min(max(d1, o1), min(d2, o2));
                d1 = min(d1, o1);
            }
            if (bkey == ~0ull) continue;
            const int best = (int)(bkey >> 32), b = (int)(bkey & PJ_IDX_MASK);
            // bestDist < secondBestDist * fNNRatio_ in float, INT_MAX when there is no second (:665)
            const float second = d2 >= PI_INF ? 2147483648.0f : (float)d2;
            if (best <= PI_TH_LOW && (float)best < second * e.nnratio) {
                if (lane == 0) {
                    const int old = m21[b];
                    if (old >= 0) { m12[old] = -1; nm--; }   // :667-671
                    m12[qi] = (int16_t)b;
                    m21[b] = (int16_t)qi;
                    mdist[b] = (uint16_t)best;
                    nm++;
                    if (e.check_ori) hist[pjm_bin(e.kp_angle[k0 + b], e.q_angle[j])]++;
                }
                __builtin_amdgcn_wave_barrier();
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            }
        }
    }
    __syncthreads();
    if (e.check_ori) {   // CheckOrientation(frame2.keypointsUn, frame1.keypointsUn, matchIds, matches12)
        if (lane == 0) keep_s = pjm_keep_bins(hist, &nm);   // nm = matchIds.size() - reduction
        __syncthreads();
        const uint32_t k = keep_s;
        for (int i = lane; i < n1; i += 64) {
            const int m = m12[i];
            if (m >= 0 && !((k >> pjm_bin(e.kp_angle[k0 + m], e.q_angle[q0 + i])) & 1u)) m12[i] = -1;
        }
        __syncthreads();
    }
    for (int i = lane; i < n1; i += 64) {   // output and the prevMatched update (:686-688)
        const int m = m12[i];
        e.matches12[q0 + i] = m;
        if (m >= 0) {
            e.prev[2 * (size_t)(q0 + i)] = a.kp_xy[2 * (size_t)(k0 + m)];
            e.prev[2 * (size_t)(q0 + i) + 1] = a.kp_xy[2 * (size_t)(k0 + m) + 1];
        }
    }
    if (lane == 0) a.n_matches[f] = nm;
}

static int launch_init(PjArgs& a, PiExtra& e, hipStream_t st) {
    int rc;
    if ((rc = launch_grid(a, st))) return rc;
    if (e.total_q > 0) {
        hipLaunchKernelGGL(pi_score_kernel, dim3((e.total_q + 15) / 16), dim3(256), 0, st, a, e);
        ORB_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(pi_walk_kernel, dim3(a.n_frames), dim3(64), 0, st, a, e);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

// Argument checks and the fields shared by both entries.
static int pi_common(const orbm_init_batch* b, int32_t* matches12, int32_t* n_matches, PjArgs& a, PiExtra& e) {
    ORB_CHECK_ARG(b, "null argument");
    int rc;
    if ((rc = pj_check_sizes(b->n_pairs, b->total_kp, b->total_q))) return rc;
    ORB_CHECK_ARG(b->window >= 0, "negative windowSize");
    std::memset(&a, 0, sizeof(a));
    std::memset(&e, 0, sizeof(e));
    a.n_frames = b->n_pairs;
    a.n_levels = 8;
    a.total_mp = b->total_q;
    e.r = (float)b->window;   // static_cast<float>(windowSize) (:622)
    e.nnratio = b->nnratio;
    e.check_ori = b->check_orientation ? 1 : 0;
    e.total_q = b->total_q;
    if (b->n_pairs == 0) return ORB_OK;
    ORB_CHECK_ARG(b->kp_begin && b->q_begin && b->bounds && b->prev_matched && matches12 && n_matches, "null array");
    ORB_CHECK_ARG(b->total_kp == 0 || (b->kp_xy && b->kp_octave && b->kp_desc), "null F2 keypoint array");
    ORB_CHECK_ARG(b->total_q == 0 || (b->q_octave && b->q_desc), "null F1 keypoint array");
    ORB_CHECK_ARG(!b->check_orientation || ((b->total_kp == 0 || b->kp_angle) && (b->total_q == 0 || b->q_angle)),
                  "CheckOrientation needs kp_angle / q_angle");
    a.kp_begin = b->kp_begin; a.kp_xy = b->kp_xy; a.kp_oct = b->kp_octave; a.kp_desc = b->kp_desc;
    a.bounds = b->bounds; a.mp_begin = b->q_begin; a.n_matches = n_matches;
    e.q_begin = b->q_begin; e.q_oct = b->q_octave; e.q_desc = b->q_desc; e.q_angle = b->q_angle;
    e.kp_angle = b->kp_angle; e.prev = b->prev_matched; e.matches12 = matches12;
    return ORB_OK;
}

}  // namespace orbamd
