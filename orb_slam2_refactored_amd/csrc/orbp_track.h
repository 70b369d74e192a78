// ORBmatcher::SearchByProjection(Frame&, const std::vector<MapPoint*>&, th) (included by orbp.hip after
// orbp_grid.h and orbp_host.h).
//
// Reference: src/ORBmatcher.cc:315-382 (the search) and :53 (RadiusByViewingCos).
//
// The reference loop is sequential in one respect only: a keypoint that an earlier map point has
// claimed (frame.mappoints[idx] with Observations() > 0, :339) is skipped by the later ones.  So
// the work splits into two data-parallel stages and one thin sequential one:
//   pj_grid_kernel   (orbp_grid.h) the FeaturesGrid of every frame
//   pj_score_kernel  one 16-lane group per map point: window cells, level / area / entry-claim /
//                    stereo gates, Hamming distance, and the K smallest keys (dist << 13 | scan
//                    position) = the first K of the candidates stably sorted by distance, plus
//                    the candidate count.
//   pj_walk_kernel   one wavefront per frame walks the map points in order with a claim bitmap
//                    in LDS: best / second best = the first two unclaimed of the K (the
//                    reference's strict-< scan keeps exactly the first two of that stable order);
//                    when fewer than two of the K are unclaimed and more candidates exist, the
//                    wavefront rescans that map point's window against the bitmap.  Then the
//                    TH_HIGH / same-level ratio test and the claim.
#pragma once

namespace orbamd {

struct PjPoint {   // one map point's search window (ORBmatcher.cc:322-333)
    PjWindow win;
    int lvl;
    float u, v, uR, radius;
};

__device__ __forceinline__ PjPoint pj_point(const PjArgs& a, int f, int mj) {
    PjPoint w;
    w.lvl = a.mp_level[mj];
    const float vcos = a.mp_vcos[mj];
    const float r = (double)vcos > 0.998 ? 2.5f : 4.f;   // RadiusByViewingCos (:53), double compare
    w.radius = a.th * r * a.scale[w.lvl];
    w.u = a.mp_proj[3 * (size_t)mj];
    w.v = a.mp_proj[3 * (size_t)mj + 1];
    w.uR = a.mp_proj[3 * (size_t)mj + 2];
    w.win = pj_window(pj_bounds(a.bounds + 4 * (size_t)f), w.u, w.v, w.radius);
    return w;
}

// Calls fn(key, idx, level) for each candidate of this lane that passes every gate; key =
// dist << 13 | sorted position (increasing along GetFeaturesInArea's scan order).
template <bool DYN, int W = 64, class Fn>
__device__ __forceinline__ void pj_scan(const PjArgs& a, int f, int mj, const PjPoint& w, const uint32_t* bits,
                                        int lane, Fn&& fn) {
    const int k0 = a.kp_begin[f];
    const uint8_t* d1 = a.mp_desc + 32 * (size_t)mj;
    pj_scan_window<W>(w.win, a.grid_start + (size_t)f * (PJ_CELLS + 1), a.grid_idx, k0, lane, [&](int p, int idx) {
        const int k = k0 + idx;
        const int level = a.kp_oct[k];
        if (level < w.lvl - 1 || level > w.lvl) return;   // checkLevels (maxLevel >= 0)
        if (!pj_in_box(a.kp_xy[2 * (size_t)k], a.kp_xy[2 * (size_t)k + 1], w.u, w.v, w.radius)) return;
        if (a.kp_claimed && a.kp_claimed[k]) return;
        if (DYN && ((bits[idx >> 5] >> (idx & 31)) & 1u)) return;
        const float ur = a.kp_ur[k];
        if (ur > 0 && fabsf(w.uR - ur) > w.radius) return;
        const int dist = pj_hamming(d1, a.kp_desc + 32 * (size_t)k);
        fn(((uint32_t)dist << PJ_IDX_BITS) | (uint32_t)p, idx, level);
    });
}

template <int K>
__device__ __forceinline__ void pj_insert(uint32_t (&t)[K], uint32_t key) {
#pragma unroll
    for (int r = 0; r < K; r++) {
        const uint32_t lo = min(t[r], key), hi = max(t[r], key);
        t[r] = lo;
        key = hi;
    }
}

// Pops the wave's K smallest keys (one lane owns each key: positions are unique).
template <int K, int W = 64>
__device__ __forceinline__ void pj_wave_topk(uint32_t (&t)[K], uint32_t (&out)[K]) {
#pragma unroll
    for (int r = 0; r < K; r++) {
        const uint32_t m = pj_wave_min<W>(t[0]);
        out[r] = m;
        if (t[0] == m && m != PJ_NONE) {
#pragma unroll
            for (int q = 0; q + 1 < K; q++) t[q] = t[q + 1];
            t[K - 1] = PJ_NONE;
        }
    }
}

// ---------------------------------------------------------------- per map point: top-K candidates
// A 16-lane group per map point (4 per wavefront; the windows at the search radii hold tens of
// candidates), the frame from pj_grid_kernel's map-point -> frame table.
__global__ __launch_bounds__(256) void pj_score_kernel(PjArgs a) {
    const int lane = threadIdx.x & (PJ_GW - 1);
    const int mj = blockIdx.x * (256 / PJ_GW) + (threadIdx.x / PJ_GW);
    if (mj >= a.total_mp) return;   // group-uniform (every later reduction stays inside the group)
    const int f = a.mp_frame[mj];
    const int n = a.kp_begin[f + 1] - a.kp_begin[f];
    int cnt = 0;
    uint32_t out[PJ_K];
#pragma unroll
    for (int r = 0; r < PJ_K; r++) out[r] = PJ_NONE;
    const int lvl = a.mp_level[mj];
    if (n <= PJ_MAXKP && a.mp_valid[mj] && lvl >= 0 && lvl < a.n_levels) {
        const PjPoint w = pj_point(a, f, mj);
        uint32_t t[PJ_K];
#pragma unroll
        for (int r = 0; r < PJ_K; r++) t[r] = PJ_NONE;
        int c = 0;
        pj_scan<false, PJ_GW>(a, f, mj, w, nullptr, lane, [&](uint32_t key, int, int) {
            pj_insert(t, key);
            c++;
        });
        cnt = pj_wave_sum<PJ_GW>(c);
        pj_wave_topk<PJ_K, PJ_GW>(t, out);
    }
    if (lane == 0) a.mp_cnt[mj] = cnt;
    if (lane < PJ_K) {
        uint32_t key = out[0];
#pragma unroll
        for (int r = 1; r < PJ_K; r++) key = lane == r ? out[r] : key;
        uint32_t ent = 0;
        if (key != PJ_NONE) {
            const int k0 = a.kp_begin[f];
            const int idx = a.grid_idx[k0 + (int)(key & PJ_IDX_MASK)];
            ent = (uint32_t)idx | ((uint32_t)a.kp_oct[k0 + idx] << 24);
        }
        a.mp_top[(size_t)mj * PJ_K + lane] = make_uint2(key, ent);
    }
}

// ---------------------------------------------------------------- the ordered claim walk
// One wavefront per frame, 64 map points per chunk, one lane per map point.  A map point's outcome
// depends on the earlier ones only through the claim bitmap (keypoints whose map point has
// observations, :339), and only through the claim bits of its K kept candidates while two of them
// remain available (else the window is rescanned).  So every round decides all remaining lanes of
// the chunk at once against the current bitmap, marks each claimed keypoint with the lowest
// claiming lane (LDS atomicMin), and commits the lanes before the first one that either saw an
// available candidate claimed by an earlier lane of the round or needs a rescan.  Claims set bits
// as the reference's loop would, in lane order (a committed lane saw no earlier claim on its
// candidates); kp_match keeps the last map point to match a keypoint (:374) by atomicMax on the map
// point index, which grows with the walk.  The first undecided lane then runs next round, or — when
// it needs the rescan — alone on the wavefront as the sequential walk does.
constexpr int PJ_CHUNK = 64;

__global__ __launch_bounds__(64) void pj_walk_kernel(PjArgs a) {
    __shared__ uint32_t bits[PJ_MAXKP / 32];
    __shared__ int stamp[PJ_MAXKP];   // lowest claiming lane of the round (64: none)
    const int lane = threadIdx.x;
    const int f = blockIdx.x;
    const int k0 = a.kp_begin[f], n = a.kp_begin[f + 1] - k0;
    const int m0 = a.mp_begin[f], nm = a.mp_begin[f + 1] - m0;
    for (int i = lane; i < n; i += 64) a.kp_match[k0 + i] = -1;
    if (n > PJ_MAXKP) {
        if (lane == 0) a.n_matches[f] = -1;
        return;
    }
    for (int w = lane; w < (n + 31) / 32; w += 64) {
        uint32_t v = 0;
        if (a.kp_claimed)
            for (int b = 0; b < 32 && w * 32 + b < n; b++) v |= (uint32_t)(a.kp_claimed[k0 + w * 32 + b] != 0) << b;
        bits[w] = v;
    }
    for (int i = lane; i < n; i += 64) stamp[i] = 64;
    __syncthreads();
    auto bit = [&](int idx) { return (bits[idx >> 5] >> (idx & 31)) & 1u; };
    int nmatches = 0;
    for (int c = 0; c < nm; c += PJ_CHUNK) {
        const int m = min(PJ_CHUNK, nm - c);
        // this lane's map point: validity, candidate count, observations, K kept candidates
        int cnt = 0;
        bool has_obs = false;
        uint2 e[PJ_K];
#pragma unroll
        for (int k = 0; k < PJ_K; k++) e[k] = make_uint2(PJ_NONE, 0);
        if (lane < m) {
            const int mj = m0 + c + lane;
            const int lvl = a.mp_level[mj];
            const bool ok = a.mp_valid[mj] && lvl >= 0 && lvl < a.n_levels;
            cnt = ok ? a.mp_cnt[mj] : 0;
            has_obs = a.mp_has_obs[mj] != 0;
#pragma unroll
            for (int k = 0; k < PJ_K; k++) e[k] = a.mp_top[(size_t)mj * PJ_K + k];
        }
        int start = 0;
        while (start < m) {   // wavefront-uniform
            // decide every lane >= start against the current bitmap
            uint32_t avail = 0;
#pragma unroll
            for (int k = 0; k < PJ_K; k++)
                if (e[k].x != PJ_NONE && !bit((int)(e[k].y & 0xffffffu))) avail |= 1u << k;
            const bool mine = lane >= start && lane < m && cnt > 0;
            const bool rescan = mine && !(__popc(avail) >= 2 || cnt <= PJ_K);
            bool match = false;
            int bidx = -1;
            if (mine && !rescan && avail) {
                const int l0 = __ffs(avail) - 1;
                const uint32_t rest = avail & (avail - 1);
                uint32_t bkey = PJ_NONE, skey = PJ_NONE, be = 0, se = 0;
#pragma unroll
                for (int k = 0; k < PJ_K; k++)
                    if (k == l0) { bkey = e[k].x; be = e[k].y; }
                if (rest) {
                    const int l1 = __ffs(rest) - 1;
#pragma unroll
                    for (int k = 0; k < PJ_K; k++)
                        if (k == l1) { skey = e[k].x; se = e[k].y; }
                }
                const int bestDist = (int)(bkey >> PJ_IDX_BITS);
                const int secondDist = skey == PJ_NONE ? 256 : (int)(skey >> PJ_IDX_BITS);
                const int blev = (int)(be >> 24), slev = skey == PJ_NONE ? -1 : (int)(se >> 24);
                if (bestDist <= PJ_TH_HIGH && !(blev == slev && (float)bestDist > a.nnratio * (float)secondDist)) {   // :367-377
                    match = true;
                    bidx = (int)(be & 0xffffffu);
                }
            }
            const bool claims = match && has_obs;
            if (claims) atomicMin(&stamp[bidx], lane);
            __syncthreads();   // one wavefront: orders its LDS writes before the reads below
            bool conflict = rescan;
            if (mine && !rescan) {
#pragma unroll
                for (int k = 0; k < PJ_K; k++)
                    if (((avail >> k) & 1u) && stamp[(int)(e[k].y & 0xffffffu)] < lane) conflict = true;
            }
            const unsigned long long cb = __ballot(conflict);
            const int stop = cb ? __ffsll((long long)cb) - 1 : m;   // first undecided lane
            // commit [start, stop)
            const bool commit = lane >= start && lane < stop && match;
            if (commit) {
                atomicMax(a.kp_match + k0 + bidx, c + lane);
                if (claims) atomicOr(&bits[bidx >> 5], 1u << (bidx & 31));
            }
            nmatches += (int)__popcll(__ballot(commit));
            if (claims) stamp[bidx] = 64;
            __syncthreads();   // one wavefront: orders its LDS writes before the reads below
            if (stop == start) {
                // lane `start` needs the rescan: the window with the current bitmap, on the wavefront
                const int i = start;
                const int mj = m0 + c + i;
                const PjPoint w = pj_point(a, f, mj);
                uint32_t t[2] = {PJ_NONE, PJ_NONE};
                pj_scan<true>(a, f, mj, w, bits, lane, [&](uint32_t key, int, int) { pj_insert(t, key); });
                uint32_t o[2];
                pj_wave_topk(t, o);
                const uint32_t bkey = o[0], skey = o[1];
                int bi = -1, blev = -1, slev = -1;
                if (bkey != PJ_NONE) {
                    bi = a.grid_idx[k0 + (int)(bkey & PJ_IDX_MASK)];
                    blev = a.kp_oct[k0 + bi];
                }
                if (skey != PJ_NONE) slev = a.kp_oct[k0 + a.grid_idx[k0 + (int)(skey & PJ_IDX_MASK)]];
                const int bestDist = bkey == PJ_NONE ? 256 : (int)(bkey >> PJ_IDX_BITS);
                const int secondDist = skey == PJ_NONE ? 256 : (int)(skey >> PJ_IDX_BITS);
                const bool obs_i = __shfl(has_obs ? 1 : 0, i, 64) != 0;
                if (bestDist <= PJ_TH_HIGH && !(blev == slev && (float)bestDist > a.nnratio * (float)secondDist)) {
                    if (lane == 0) {
                        atomicMax(a.kp_match + k0 + bi, c + i);
                        if (obs_i) bits[bi >> 5] |= 1u << (bi & 31);
                    }
                    nmatches++;
                }
                __syncthreads();   // one wavefront: orders its LDS writes before the reads below
                start = i + 1;
            } else {
                start = stop;
            }
        }
    }
    if (lane == 0) a.n_matches[f] = nmatches;
}

static int launch_projection(PjArgs& a, hipStream_t st) {
    int rc;
    if ((rc = launch_grid(a, st))) return rc;
    if (a.total_mp > 0) {
        hipLaunchKernelGGL(pj_score_kernel, dim3((a.total_mp + 256 / PJ_GW - 1) / (256 / PJ_GW)), dim3(256), 0, st, a);
        ORB_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(pj_walk_kernel, dim3(a.n_frames), dim3(64), 0, st, a);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

// Argument checks and the fields shared by both entries (the arrays as the device entry reads them).
static int proj_common(const orbm_proj_batch* b, int32_t* kp_match, int32_t* n_matches, PjArgs& a) {
    ORB_CHECK_ARG(b, "null argument");
    int rc;
    if ((rc = pj_check_sizes(b->n_frames, b->total_kp, b->total_mp))) return rc;
    std::memset(&a, 0, sizeof(a));
    if ((rc = pj_set_pyramid(a, b->n_levels, b->scale_factors, b->th))) return rc;
    a.n_frames = b->n_frames;
    a.nnratio = b->nnratio;
    a.total_mp = b->total_mp;
    if (b->n_frames == 0) return ORB_OK;
    ORB_CHECK_ARG(b->kp_begin && b->mp_begin && b->bounds && kp_match && n_matches, "null array");
    ORB_CHECK_ARG(b->total_kp == 0 || (b->kp_xy && b->kp_octave && b->kp_uright && b->kp_desc), "null keypoint array");
    ORB_CHECK_ARG(b->total_mp == 0 || (b->mp_valid && b->mp_proj && b->mp_view_cos && b->mp_level && b->mp_desc &&
                                       b->mp_has_obs),
                  "null map point array");
    a.kp_begin = b->kp_begin; a.kp_xy = b->kp_xy; a.kp_oct = b->kp_octave; a.kp_ur = b->kp_uright;
    a.kp_desc = b->kp_desc; a.kp_claimed = b->kp_claimed; a.bounds = b->bounds;
    a.mp_begin = b->mp_begin; a.mp_valid = b->mp_valid; a.mp_proj = b->mp_proj; a.mp_vcos = b->mp_view_cos;
    a.mp_level = b->mp_level; a.mp_desc = b->mp_desc; a.mp_has_obs = b->mp_has_obs;
    a.kp_match = kp_match;
    a.n_matches = n_matches;
    return ORB_OK;
}

}  // namespace orbamd
