// orbtl.hip — Tracking's local map on gfx950: LocalMap::Update and SearchLocalPoints up to the matcher call, batched
// over frames (include/orbslam2_amd.h, "Tracking's local map").
//
// Reference: src/Tracking.cc:59-179 (UpdateLocalKeyFrames, UpdateLocalPoints), :554-642 (IsInFrustum,
// SearchLocalPoints).  The per-point arithmetic is csrc/tl_frustum.h's.
//
// The map is slot tables; the std::map of votes and the std::set of children are walked in ascending slot order
// (the reference: pointer order).  Passes of one call, stream-ordered, nothing read back:
//   tl_vote_kernel     one thread per (f, keypoint): bad points nulled, votes by integer atomics, the seen bytes,
//                      kp_claimed
//   tl_list_kernel     one wavefront per f: the first part by ballot over 64 slots a step, then the sequential walk
//                      with the lanes scanning a covisibility row or a child list
//   tl_first_kernel    one thread per (f, list position, keypoint): atomicMin of position * kf_cap + index into the
//                      (f, map point) first-occurrence table
//   tl_count_kernel    one workgroup per (f, list position): how many of its entries are first occurrences
//   tl_emit_kernel     one workgroup per (f, list position): its offset = the counts before it; an ordered
//                      compaction by ballot / popcount prefix (no atomics: the order is the reference's)
//   tl_frustum_kernel  one thread per (f, keypoint) for step 5 and per (f, local point) for IsInFrustum
//   tl_gather_kernel   two lanes per local point, 16 bytes each: the descriptors
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "tl_frustum.h"

namespace orbamd {

constexpr int TL_COVIS = ORBDB_COVIS;

struct TlWork {
    int32_t* votes;   // [F][K]
    uint8_t* mark;    // [F][K]
    uint32_t* first;  // [F][M]
    uint8_t* seen;    // [F][M]
    int32_t* cnt;     // [F][kf_list_cap]
};

__device__ __forceinline__ int tl_clamp(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(256) void tl_vote_kernel(orbtl_map m, orbtl_frames fr, orbtl_result o, TlWork w) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x == 0 && f == 0)
        for (int t = threadIdx.x; t <= fr.n_frames; t += 256) {
            o.kp_begin[t] = t * fr.kp_cap;
            o.mp_begin[t] = t * fr.mp_cap;
        }
    if (i >= fr.kp_cap) return;
    const size_t at = (size_t)f * fr.kp_cap + i;
    uint8_t claimed = 1;   // the padding is claimed: never matched
    if (i < tl_clamp(fr.frame_n[f], 0, fr.kp_cap)) {
        claimed = 0;
        const int p = fr.frame_mappoint[at];
        if (p >= 0 && p < m.n_mappoints) {
            if (m.mp_bad[p]) {
                fr.frame_mappoint[at] = -1;   // currFrame.mappoints[i] = nullptr (:86)
            } else {
                w.seen[(size_t)f * m.n_mappoints + p] = 1;
                const int e0 = m.mp_obs_off[p], e1 = m.mp_obs_off[p + 1];
                for (int e = e0; e0 >= 0 && e < e1; e++) {
                    const int k = m.mp_obs_kf[e];
                    if (k >= 0 && k < m.n_keyframes) atomicAdd(&w.votes[(size_t)f * m.n_keyframes + k], 1);
                }
                claimed = m.mp_nobs[p] > 0 ? 1 : 0;
            }
        } else if (p != -1) {
            fr.frame_mappoint[at] = -1;   // a slot outside the table is null
        }
    }
    o.kp_claimed[at] = claimed;
}

// One wavefront per frame.  `mark` is written and read by different lanes of this wavefront: every store is
// followed by __syncthreads() (one wavefront: a wait for the stores and a fence) before the next read.
__global__ __launch_bounds__(64) void tl_list_kernel(orbtl_map m, orbtl_frames fr, orbtl_result o, TlWork w) {
    const int f = blockIdx.x, lane = threadIdx.x, K = m.n_keyframes, cap = fr.kf_list_cap;
    const int32_t* votes = w.votes + (size_t)f * K;
    uint8_t* mark = w.mark + (size_t)f * K;
    int32_t* list = fr.local_kf + (size_t)f * cap;
    if (lane == 0) {
        o.status[f] = ORBTL_OK;
        o.n_to_match[f] = 0;
    }
    // ---- first part: the voted keyframes ascending, maxCount by a strict comparison (:100-116)
    int size = 0, best_c = 0, best_k = -1;
    bool any = false;
    for (int base = 0; base < K; base += 64) {
        const int k = base + lane;
        const int c = k < K ? votes[k] : 0;
        const bool take = c > 0 && !m.kf_bad[k];
        any |= c > 0;
        const unsigned long long b = __ballot(take);
        if (take) {
            const int pos = size + __popcll(b & ((1ull << lane) - 1));
            if (pos < cap) list[pos] = k;
            mark[k] = 1;
            if (c > best_c) { best_c = c; best_k = k; }   // ascending k per lane: the first of equal counts stays
        }
        size += __popcll(b);
    }
    if (!__ballot(any)) {   // keyframeCounter.empty(): return (:90); the list is the one that came in
        if (lane == 0) {
            o.reference_kf[f] = -1;
            fr.n_local_kf[f] = tl_clamp(fr.n_local_kf[f], 0, cap);
        }
        return;
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
        const int oc = __shfl_xor(best_c, s, 64), ok = __shfl_xor(best_k, s, 64);
        if (ok >= 0 && (oc > best_c || (oc == best_c && (best_k < 0 || ok < best_k)))) { best_c = oc; best_k = ok; }
    }
    __syncthreads();
    // ---- second part (:119-156): only the first part's elements are walked (end() is taken once)
    const int n1 = size;
    for (int e = 0; e < n1 && n1 <= cap; e++) {
        if (size > ORBTL_MAX_KEYFRAMES) break;
        const int k = list[e];
        {   // GetBestCovisibilityKeyFrames(10)
            const int nb = lane < TL_COVIS ? m.kf_covis[(size_t)k * TL_COVIS + lane] : -1;
            const bool ok = nb >= 0 && nb < K && !m.kf_bad[nb] && !mark[nb];
            const unsigned long long b = __ballot(ok);
            if (b) {
                const int first = __builtin_ctzll(b);
                if (lane == first) {
                    if (size < cap) list[size] = nb;
                    mark[nb] = 1;
                }
                size++;
                __syncthreads();
            }
        }
        {   // GetChildren()
            const int c0 = m.kf_child_off[k], c1 = m.kf_child_off[k + 1];
            for (int base = c0; c0 >= 0 && base < c1; base += 64) {
                const int ch = base + lane < c1 ? m.kf_child_idx[base + lane] : -1;
                const bool ok = ch >= 0 && ch < K && !m.kf_bad[ch] && !mark[ch];
                const unsigned long long b = __ballot(ok);
                if (b) {
                    const int first = __builtin_ctzll(b);
                    if (lane == first) {
                        if (size < cap) list[size] = ch;
                        mark[ch] = 1;
                    }
                    size++;
                    __syncthreads();
                    break;
                }
            }
        }
        const int par = m.kf_parent[k];   // no isBad() check (:145-154)
        if (par >= 0 && par < K && !mark[par]) {
            if (lane == 0) {
                if (size < cap) list[size] = par;
                mark[par] = 1;
            }
            size++;
            break;
        }
    }
    if (lane == 0) {
        o.reference_kf[f] = best_k;
        fr.n_local_kf[f] = min(size, cap);
        if (size > cap) {
            o.status[f] = ORBTL_KF_OVERFLOW;
            o.n_to_match[f] = -1;
        }
    }
}

// The entry (f, p, idx) of the listed keyframes' map points: the slot, or -1 when it is null, bad or outside.
__device__ __forceinline__ int tl_entry(const orbtl_map& m, int k, int idx) {
    if (k < 0 || k >= m.n_keyframes || idx >= tl_clamp(m.kf_n[k], 0, m.kf_cap)) return -1;
    const int p = m.kf_mappoint[(size_t)k * m.kf_cap + idx];
    return (p >= 0 && p < m.n_mappoints && !m.mp_bad[p]) ? p : -1;
}

__global__ __launch_bounds__(256) void tl_first_kernel(orbtl_map m, orbtl_frames fr, orbtl_result o, TlWork w) {
    const int f = blockIdx.z, p = blockIdx.y, idx = blockIdx.x * 256 + threadIdx.x;
    if (o.status[f] != ORBTL_OK || p >= fr.n_local_kf[f] || idx >= m.kf_cap) return;
    const int mp = tl_entry(m, fr.local_kf[(size_t)f * fr.kf_list_cap + p], idx);
    if (mp >= 0) atomicMin(&w.first[(size_t)f * m.n_mappoints + mp], (uint32_t)p * (uint32_t)m.kf_cap + (uint32_t)idx);
}

// Is (f, p, idx) the first occurrence of its map point?  Returns the slot or -1.
__device__ __forceinline__ int tl_is_first(const orbtl_map& m, const orbtl_frames& fr, const TlWork& w, int f, int p,
                                           int idx) {
    if (idx >= m.kf_cap) return -1;
    const int mp = tl_entry(m, fr.local_kf[(size_t)f * fr.kf_list_cap + p], idx);
    if (mp < 0) return -1;
    return w.first[(size_t)f * m.n_mappoints + mp] == (uint32_t)p * (uint32_t)m.kf_cap + (uint32_t)idx ? mp : -1;
}

__global__ __launch_bounds__(256) void tl_count_kernel(orbtl_map m, orbtl_frames fr, orbtl_result o, TlWork w) {
    __shared__ int s_c[4];
    const int f = blockIdx.y, p = blockIdx.x;
    int c = 0;
    if (o.status[f] == ORBTL_OK && p < fr.n_local_kf[f])
        for (int idx = threadIdx.x; idx < m.kf_cap; idx += 256) c += tl_is_first(m, fr, w, f, p, idx) >= 0 ? 1 : 0;
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) c += __shfl_xor(c, s, 64);
    if ((threadIdx.x & 63) == 0) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) w.cnt[(size_t)f * fr.kf_list_cap + p] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
}

__global__ __launch_bounds__(256) void tl_emit_kernel(orbtl_map m, orbtl_frames fr, orbtl_result o, TlWork w) {
    __shared__ int s_before, s_total, s_wave[4];
    const int f = blockIdx.y, p = blockIdx.x, cap = fr.kf_list_cap;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (o.status[f] != ORBTL_OK) {   // tl_list_kernel's; step 4's own overflow is stored by tl_overflow_kernel
        if (p == 0) {
            for (int j = threadIdx.x; j < fr.mp_cap; j += 256) o.local_mp[(size_t)f * fr.mp_cap + j] = -1;
            if (threadIdx.x == 0) o.n_local_mp[f] = 0;
        }
        return;
    }
    if (wave == 0) {   // the counts before this position, and the frame's total
        int before = 0, total = 0;
        for (int q = lane; q < cap; q += 64) {
            const int c = w.cnt[(size_t)f * cap + q];
            total += c;
            if (q < p) before += c;
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            before += __shfl_xor(before, s, 64);
            total += __shfl_xor(total, s, 64);
        }
        if (lane == 0) { s_before = before; s_total = total; }
    }
    __syncthreads();
    const int total = s_total;
    const bool over = total > fr.mp_cap;   // every workgroup of the frame finds the same total: none emits
    if (p == 0) {
        const int n = over ? 0 : total;
        for (int j = n + (int)threadIdx.x; j < fr.mp_cap; j += 256) o.local_mp[(size_t)f * fr.mp_cap + j] = -1;
        if (threadIdx.x == 0) o.n_local_mp[f] = n;
    }
    if (over || p >= fr.n_local_kf[f]) return;
    int pos = s_before;
    for (int base = 0; base < m.kf_cap; base += 256) {   // uniform trip count
        const int mp = tl_is_first(m, fr, w, f, p, base + (int)threadIdx.x);
        const unsigned long long b = __ballot(mp >= 0);
        if (lane == 0) s_wave[wave] = __popcll(b);
        __syncthreads();
        int off = pos;
        for (int t = 0; t < wave; t++) off += s_wave[t];
        const int step = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        if (mp >= 0) {
            const int j = off + __popcll(b & ((1ull << lane) - 1));
            if (j < fr.mp_cap) o.local_mp[(size_t)f * fr.mp_cap + j] = mp;   // j < total <= mp_cap
        }
        pos += step;
        __syncthreads();
    }
}

// The overflow status of step 4, after every tl_emit workgroup has read the status of steps 2-3.
__global__ __launch_bounds__(256) void tl_overflow_kernel(orbtl_frames fr, orbtl_result o, TlWork w) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= fr.n_frames || o.status[f] != ORBTL_OK) return;
    long long total = 0;
    for (int q = 0; q < fr.kf_list_cap; q++) total += w.cnt[(size_t)f * fr.kf_list_cap + q];
    if (total > fr.mp_cap) {
        o.status[f] = ORBTL_MP_OVERFLOW;
        o.n_to_match[f] = -1;
    }
}

__global__ __launch_bounds__(256) void tl_frustum_kernel(orbtl_map m, orbtl_frames fr, orbtl_result o, TlWork w) {
    const int f = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    const bool live = o.status[f] == ORBTL_OK;
    // step 5 (:610-625): the frame's own points are visible once per keypoint holding them
    if (live && t < fr.kp_cap && t < fr.frame_n[f]) {
        const int p = fr.frame_mappoint[(size_t)f * fr.kp_cap + t];
        if (p >= 0 && p < m.n_mappoints && !m.mp_bad[p]) atomicAdd(&m.mp_visible[p], 1);
    }
    // step 6 (:631-642)
    bool pass = false;
    if (t < fr.mp_cap) {
        const size_t at = (size_t)f * fr.mp_cap + t;
        TlPoint r{TL_DEPTH, 0.f, 0.f, 0.f, 0.f, 0, 0.0};
        uint8_t has_obs = 0;
        if (live && t < o.n_local_mp[f]) {
            const int p = o.local_mp[at];   // in [0, M) and not bad: tl_entry
            has_obs = m.mp_nobs[p] > 0 ? 1 : 0;
            if (!w.seen[(size_t)f * m.n_mappoints + p]) {   // lastFrameSeen != currFrame.id
                r = tl_frustum(fr.pose + 12 * (size_t)f, fr.camera + 5 * (size_t)f, fr.bounds + 4 * (size_t)f,
                               m.mp_xw + 3 * (size_t)p, m.mp_normal + 3 * (size_t)p, m.mp_max_min[2 * (size_t)p],
                               m.mp_max_min[2 * (size_t)p + 1], fr.min_view_cos, fr.log_scale_factor, fr.n_levels);
                pass = r.fail == TL_PASS;
                if (pass) atomicAdd(&m.mp_visible[p], 1);   // IncreaseVisible (:639)
            }
        }
        o.mp_valid[at] = pass ? 1 : 0;
        o.mp_proj[3 * at] = pass ? r.u : 0.f;
        o.mp_proj[3 * at + 1] = pass ? r.v : 0.f;
        o.mp_proj[3 * at + 2] = pass ? r.ur : 0.f;
        o.mp_view_cos[at] = pass ? r.view_cos : 0.f;
        o.mp_level[at] = pass ? r.level : 0;
        o.mp_has_obs[at] = has_obs;
    }
    const unsigned long long b = __ballot(pass);
    if (b && (threadIdx.x & 63) == 0) atomicAdd(&o.n_to_match[f], __popcll(b));
}

__global__ __launch_bounds__(256) void tl_gather_kernel(orbtl_map m, orbtl_frames fr, orbtl_result o) {
    const int f = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    const int j = t >> 1, half = t & 1;
    if (j >= fr.mp_cap) return;
    const size_t at = (size_t)f * fr.mp_cap + j;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (o.status[f] == ORBTL_OK && j < o.n_local_mp[f])
        v = reinterpret_cast<const uint4*>(m.mp_desc)[2 * (size_t)o.local_mp[at] + half];
    reinterpret_cast<uint4*>(o.mp_desc)[2 * at + half] = v;
}

}  // namespace orbamd

using namespace orbamd;

namespace {

thread_local Scratch g_tl;

constexpr long long TL_MAX_ENTRIES = 0x7fffffffLL;

int tl_check(const orbtl_map* m, const orbtl_frames* fr, const orbtl_result* o) {
    ORB_CHECK_ARG(m && fr && o, "null map, frames or result");
    ORB_CHECK_ARG(m->n_keyframes >= 0 && m->n_mappoints >= 0 && fr->n_frames >= 0, "negative sizes");
    ORB_CHECK_ARG(m->kf_cap >= 1 && fr->kp_cap >= 1, "kf_cap and kp_cap must be at least 1");
    ORB_CHECK_ARG(fr->kf_list_cap >= 1, "kf_list_cap must be at least 1");
    ORB_CHECK_ARG(fr->mp_cap >= 1, "mp_cap must be at least 1");
    ORB_CHECK_ARG(fr->n_levels >= 1 && fr->n_levels <= 32, "n_levels must be in [1, 32]");
    ORB_CHECK_ARG(std::isfinite(fr->log_scale_factor) && fr->log_scale_factor > 0.f, "log_scale_factor must be finite and > 0");
    const long long F = fr->n_frames, K = m->n_keyframes;
    ORB_CHECK_ARG((long long)fr->kf_list_cap * m->kf_cap < TL_MAX_ENTRIES, "kf_list_cap x kf_cap must be below 2^31");
    ORB_CHECK_ARG(K * m->kf_cap < TL_MAX_ENTRIES && F * fr->kp_cap < TL_MAX_ENTRIES && F * fr->mp_cap < TL_MAX_ENTRIES &&
                      F * std::max(K, 1LL) < TL_MAX_ENTRIES && F * fr->kf_list_cap < TL_MAX_ENTRIES && F < 65536 &&
                      fr->kf_list_cap < 65536,
                  "a table of 2^31 entries or more (or 65536 frames / list positions) in one call");
    if (F == 0) return ORB_OK;
    ORB_CHECK_ARG(m->kf_bad && m->kf_covis && m->kf_parent && m->kf_child_off && m->kf_child_idx && m->kf_n && m->kf_mappoint,
                  "null keyframe table");
    ORB_CHECK_ARG(m->mp_bad && m->mp_xw && m->mp_normal && m->mp_max_min && m->mp_desc && m->mp_nobs && m->mp_obs_off &&
                      m->mp_obs_kf && m->mp_visible,
                  "null map-point table");
    ORB_CHECK_ARG(fr->frame_n && fr->frame_mappoint && fr->pose && fr->camera && fr->bounds && fr->local_kf && fr->n_local_kf,
                  "null frame array");
    ORB_CHECK_ARG(o->reference_kf && o->local_mp && o->n_local_mp && o->n_to_match && o->status && o->kp_begin && o->mp_begin &&
                      o->kp_claimed && o->mp_valid && o->mp_proj && o->mp_view_cos && o->mp_level && o->mp_desc && o->mp_has_obs,
                  "null output array");
    ORB_CHECK_ARG(((uintptr_t)m->mp_desc | (uintptr_t)o->mp_desc) % 16 == 0, "mp_desc arrays must be 16-byte aligned");
    return ORB_OK;
}

// CSR offsets and the keyframe slots they index
int tl_check_csr(const int32_t* off, const int32_t* idx, int n, int range, const char* what) {
    int rc;
    if ((rc = check_csr(off, n, 0x7fffffff, what))) return rc;
    return check_range(idx, off[n], 0, range, (std::string(what) + ": keyframe slot outside [0, n_keyframes)").c_str());
}

int tl_check_slots(const int32_t* a, size_t n, int range, const char* msg) { return check_range(a, n, -1, range, msg); }

int tl_check_host(const orbtl_map* m, const orbtl_frames* fr) {
    const int K = m->n_keyframes, M = m->n_mappoints, F = fr->n_frames;
    int rc;
    if ((rc = tl_check_slots(m->kf_covis, (size_t)K * TL_COVIS, K, "kf_covis entry outside [-1, n_keyframes)"))) return rc;
    if ((rc = tl_check_slots(m->kf_parent, K, K, "kf_parent outside [-1, n_keyframes)"))) return rc;
    if ((rc = tl_check_csr(m->kf_child_off, m->kf_child_idx, K, K, "kf_child"))) return rc;
    for (int k = 0; k < K; k++) ORB_CHECK_ARG(m->kf_n[k] >= 0 && m->kf_n[k] <= m->kf_cap, "kf_n outside [0, kf_cap]");
    if ((rc = tl_check_slots(m->kf_mappoint, (size_t)K * m->kf_cap, M, "kf_mappoint entry outside [-1, n_mappoints)"))) return rc;
    if ((rc = tl_check_csr(m->mp_obs_off, m->mp_obs_kf, M, K, "mp_obs"))) return rc;
    for (int f = 0; f < F; f++) {
        ORB_CHECK_ARG(fr->frame_n[f] >= 0 && fr->frame_n[f] <= fr->kp_cap, "frame_n outside [0, kp_cap]");
        ORB_CHECK_ARG(fr->n_local_kf[f] >= 0 && fr->n_local_kf[f] <= fr->kf_list_cap, "n_local_kf outside [0, kf_list_cap]");
        for (int p = 0; p < fr->n_local_kf[f]; p++) {
            const int k = fr->local_kf[(size_t)f * fr->kf_list_cap + p];
            ORB_CHECK_ARG(k >= 0 && k < K, "local_kf entry outside [0, n_keyframes)");
        }
    }
    return tl_check_slots(fr->frame_mappoint, (size_t)F * fr->kp_cap, M, "frame_mappoint entry outside [-1, n_mappoints)");
}

}  // namespace

extern "C" int orbtl_track_local_map_device(const orbtl_map* map, const orbtl_frames* frames, const orbtl_result* out,
                                            void* stream) {
    int rc;
    if ((rc = tl_check(map, frames, out))) return rc;
    if (frames->n_frames == 0) return ORB_OK;
    if ((rc = g_tl.use_current_device())) return rc;
    hipStream_t st = (hipStream_t)stream;
    const orbtl_map& m = *map;
    const orbtl_frames& fr = *frames;
    const size_t F = fr.n_frames, K = m.n_keyframes, M = m.n_mappoints;
    TlWork w{};   // votes | mark | seen (zeroed together), first (all ones), cnt (written by tl_count_kernel)
    size_t zero_end = 0;
    auto carve = [&](char* base) {
        Carver c{base};
        c.take(w.votes, out->votes ? 0 : F * K); c.take(w.mark, F * K); c.take(w.seen, F * M);
        zero_end = c.off;
        c.take(w.first, F * M); c.take(w.cnt, F * fr.kf_list_cap);
        return c.off;
    };
    if ((rc = g_tl.ws.reserve(carve(nullptr)))) return rc;
    char* p = g_tl.ws.as<char>();
    carve(p);
    if (out->votes) w.votes = out->votes;
    ORB_HIP_TRY(hipMemsetAsync(p, 0, zero_end, st));
    if (out->votes) ORB_HIP_TRY(hipMemsetAsync(out->votes, 0, std::max<size_t>(F * K * 4, 1), st));
    ORB_HIP_TRY(hipMemsetAsync(w.first, 0xff, std::max<size_t>(F * M * 4, 1), st));
    const unsigned nF = (unsigned)F, cap = (unsigned)fr.kf_list_cap;
    const unsigned per_frame = (unsigned)std::max(fr.kp_cap, fr.mp_cap);
    hipLaunchKernelGGL(tl_vote_kernel, dim3((fr.kp_cap + 255) / 256, nF), dim3(256), 0, st, m, fr, *out, w);
    hipLaunchKernelGGL(tl_list_kernel, dim3(nF), dim3(64), 0, st, m, fr, *out, w);
    hipLaunchKernelGGL(tl_first_kernel, dim3((m.kf_cap + 255) / 256, cap, nF), dim3(256), 0, st, m, fr, *out, w);
    hipLaunchKernelGGL(tl_count_kernel, dim3(cap, nF), dim3(256), 0, st, m, fr, *out, w);
    hipLaunchKernelGGL(tl_emit_kernel, dim3(cap, nF), dim3(256), 0, st, m, fr, *out, w);
    hipLaunchKernelGGL(tl_overflow_kernel, dim3((nF + 255) / 256), dim3(256), 0, st, fr, *out, w);
    hipLaunchKernelGGL(tl_frustum_kernel, dim3((per_frame + 255) / 256, nF), dim3(256), 0, st, m, fr, *out, w);
    hipLaunchKernelGGL(tl_gather_kernel, dim3((2 * fr.mp_cap + 255) / 256, nF), dim3(256), 0, st, m, fr, *out);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbtl_track_local_map(const orbtl_map* map, const orbtl_frames* frames, const orbtl_result* out,
                                     int device) {
    int rc;
    if ((rc = tl_check(map, frames, out))) return rc;
    if (frames->n_frames == 0) return ORB_OK;
    if ((rc = tl_check_host(map, frames))) return rc;   // before any copy
    const size_t F = frames->n_frames, K = map->n_keyframes, M = map->n_mappoints, kc = map->kf_cap, pc = frames->kp_cap,
                 lc = frames->kf_list_cap, mc = frames->mp_cap;
    const size_t n_child = K ? map->kf_child_off[K] : 0, n_obs = M ? map->mp_obs_off[M] : 0;
    orbtl_map dm = *map;
    orbtl_frames df = *frames;
    orbtl_result dr = *out;
    Mirror io;
    io.add(dm.kf_bad, K, true, false); io.add(dm.kf_covis, K * TL_COVIS, true, false); io.add(dm.kf_parent, K, true, false);
    io.add(dm.kf_child_off, K + 1, true, false); io.add(dm.kf_child_idx, n_child, true, false); io.add(dm.kf_n, K, true, false);
    io.add(dm.kf_mappoint, K * kc, true, false); io.add(dm.mp_bad, M, true, false); io.add(dm.mp_xw, M * 3, true, false);
    io.add(dm.mp_normal, M * 3, true, false); io.add(dm.mp_max_min, M * 2, true, false); io.add(dm.mp_desc, M * 32, true, false);
    io.add(dm.mp_nobs, M, true, false); io.add(dm.mp_obs_off, M + 1, true, false); io.add(dm.mp_obs_kf, n_obs, true, false);
    io.add(dm.mp_visible, M, true, true);
    io.add(df.frame_n, F, true, false); io.add(df.frame_mappoint, F * pc, true, true); io.add(df.pose, F * 12, true, false);
    io.add(df.camera, F * 5, true, false); io.add(df.bounds, F * 4, true, false); io.add(df.local_kf, F * lc, true, true);
    io.add(df.n_local_kf, F, true, true);
    io.add(dr.reference_kf, F, false, true); io.add(dr.local_mp, F * mc, false, true); io.add(dr.n_local_mp, F, false, true);
    io.add(dr.n_to_match, F, false, true); io.add(dr.status, F, false, true); io.add(dr.kp_begin, F + 1, false, true);
    io.add(dr.mp_begin, F + 1, false, true); io.add(dr.kp_claimed, F * pc, false, true); io.add(dr.mp_valid, F * mc, false, true);
    io.add(dr.mp_proj, F * mc * 3, false, true); io.add(dr.mp_view_cos, F * mc, false, true); io.add(dr.mp_level, F * mc, false, true);
    io.add(dr.mp_desc, F * mc * 32, false, true); io.add(dr.mp_has_obs, F * mc, false, true); io.add(dr.votes, F * K, false, true);
    return run_host(g_tl, device, io, [&] { return orbtl_track_local_map_device(&dm, &df, &dr, nullptr); });
}
