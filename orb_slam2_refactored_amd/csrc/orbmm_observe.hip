// orbmm_observe.hip — observation edits on gfx950 (include/orbslam2_amd.h, "Observation edits"; the rules are
// csrc/mm_observe.h's).  The lane groups and the scan are csrc/mm_groups.h's, the per-thread buffers and the table checks
// orbmm.hip's entries share csrc/mm_host.h's.
//   mm_obs_new_kernel     one thread per entry of the new keyframe's row: IsInKeyFrame, else AddObservation on the
//                         point's row (the points of a row are distinct: a row has one writer)
//   mm_obs_lists_kernel   one workgroup: the two stable compactions (added, recent) and their counts
//   mm_obs_apply_kernel   one workgroup of four wavefronts walks the Fuse list: the lanes compact a chunk's hits into
//                         LDS, the hits are taken one after another on uniformly loaded values, Replace's union is spread
//                         over all lanes; a last scan turns the touched flags into the list
//   mm_grow_*_kernel      the CSR with slack: count per point, one 64-bit scan by one workgroup, fill
#include <algorithm>

#include "common.h"
#include "mm_groups.h"
#include "mm_host.h"
#include "mm_observe.h"

namespace orbamd {

__global__ __launch_bounds__(256) void mm_obs_new_kernel(MmObserve t, int cur, uint8_t* kind, int32_t* status) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= t.kf_cap) return;
    int32_t st = MM_OK;
    kind[i] = (uint8_t)obs_new_keyframe_entry(t, cur, i, st);
    status[i] = st;
}

// added / recent_out: kf_cap entries each, -1 padded; counts: their two lengths
__global__ __launch_bounds__(64 * MM_CULL_WAVES) void mm_obs_lists_kernel(MmObserve t, int cur, const uint8_t* kind, int32_t* added,
                                                                           int32_t* recent_out, int32_t* counts) {
    __shared__ int32_t s_red[MM_CULL_WAVES];
    const MmBlock b{(int)threadIdx.x, s_red};
    const bool live = cur >= 0 && cur < t.K;
    for (int list = 0; list < 2; list++) {
        int32_t* out = list == 0 ? added : recent_out;
        const int want = list == 0 ? OBS_ADDED : OBS_RECENT;
        int at = 0;
        for (int base = 0; base < t.kf_cap; base += b.width) {   // uniform trip count
            const int i = base + b.lane;
            const bool flag = live && i < t.kf_cap && kind[i] == want;
            int total;
            const int off = b.prefix(flag, total);
            if (flag) out[at + off] = t.kf_mappoint[(size_t)cur * t.kf_cap + i];
            at += total;
        }
        for (int i = at + b.lane; i < t.kf_cap; i += b.width) out[i] = -1;
        if (b.lane == 0) counts[list] = at;
    }
}

__global__ __launch_bounds__(64 * MM_CULL_WAVES) void mm_obs_apply_kernel(MmObserve t, MmApply a, int32_t* ws) {
    __shared__ int32_t s_red[MM_CULL_WAVES];
    __shared__ int32_t s_chunk[64 * MM_CULL_WAVES];
    const MmBlock b{(int)threadIdx.x, s_red};
    obs_fuse_apply(b, t, a, s_chunk, ws);
}

__global__ __launch_bounds__(256) void mm_grow_count_kernel(int M, int n_obs, const int32_t* off, const int32_t* kf, int slack,
                                                            const int32_t* extra, int n_out, int32_t* out_off) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= M) return;
    const int s = extra ? mm_clamp(extra[p], 0, n_out) : slack;
    out_off[p] = obs_grow_point(n_obs, off, kf, nullptr, p, 0, 0, 0, nullptr, nullptr) + s;   // <= n_obs + n_out
}

// Exclusive scan of out_off[0 .. M) in place by one workgroup of 256, summed in 64 bits; an offset past n_out is stored
// as n_out + 1 (nothing is written from there on).  *status: the total does not fit.
__global__ __launch_bounds__(256) void mm_grow_scan_kernel(int M, int n_out, int32_t* out_off, int32_t* status) {
    const long long total = mm_block_scan<long long>(out_off, M, out_off, 0, 0x7fffffff, 0, (long long)n_out + 1);
    if (threadIdx.x == 0) *status = total > n_out ? MM_OBS_OVERFLOW : MM_OK;
}

__global__ __launch_bounds__(256) void mm_grow_fill_kernel(int M, int n_obs, const int32_t* off, const int32_t* kf,
                                                           const int32_t* idx, int n_out, const int32_t* out_off,
                                                           int32_t* out_kf, int32_t* out_idx) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= M) return;
    const int at = out_off[p], room = out_off[p + 1] - at;   // the row: live entries, then the slack
    const int n = obs_grow_point(n_obs, off, kf, idx, p, 0, at, n_out, out_kf, out_idx);
    for (int j = n; j < room; j++)
        if ((long long)at + j < n_out) out_kf[at + j] = out_idx[at + j] = -1;
}

}  // namespace orbamd

using namespace orbamd;

namespace {

MmObserve mm_observe(const orbmm_observe& o) {
    return MmObserve{o.n_keyframes, o.n_mappoints, o.kf_cap, o.n_obs, o.kf_n, o.kf_mappoint, o.kf_uright, o.mp_bad, o.mp_nobs,
                     o.mp_found, o.mp_visible, o.mp_replaced, o.mp_obs_off, o.mp_obs_kf, o.mp_obs_idx};
}

int mm_observe_check(const orbmm_observe* o, bool replace) {
    ORB_CHECK_ARG(o, "null observation tables");
    ORB_CHECK_ARG(o->n_keyframes >= 0 && o->n_mappoints >= 0 && o->n_obs >= 0, "negative sizes");
    ORB_CHECK_ARG(o->kf_cap >= 1, "kf_cap must be at least 1");
    ORB_CHECK_ARG((long long)o->n_keyframes * o->kf_cap < MM_MAX_ENTRIES && 3LL * o->n_obs + o->n_mappoints < MM_MAX_ENTRIES,
                  "a table of 2^31 entries or more");
    ORB_CHECK_ARG(o->kf_n && o->kf_mappoint && o->kf_uright, "null keyframe table");
    ORB_CHECK_ARG(o->mp_bad && o->mp_nobs && o->mp_obs_off && o->mp_obs_kf && o->mp_obs_idx, "null map-point table");
    ORB_CHECK_ARG(!replace || (o->mp_found && o->mp_visible && o->mp_replaced), "null map-point table");
    return ORB_OK;
}

// The host entries' checks: the slack (-1) is accepted; what is live ascends.
int mm_observe_check_host(const orbmm_observe* o, bool replace) {
    const int K = o->n_keyframes, M = o->n_mappoints;
    int rc;
    if ((rc = check_csr(o->mp_obs_off, M, o->n_obs, "mp_obs"))) return rc;
    if ((rc = check_range(o->kf_n, K, 0, o->kf_cap + 1, "kf_n outside [0, kf_cap]"))) return rc;
    if ((rc = check_range(o->kf_mappoint, (size_t)K * o->kf_cap, -1, M, "kf_mappoint entry outside [-1, n_mappoints)"))) return rc;
    for (int p = 0; p < M; p++) {
        int last = -1;
        for (int e = o->mp_obs_off[p]; e < o->mp_obs_off[p + 1]; e++) {
            const int k = o->mp_obs_kf[e];
            if (k == -1) continue;
            ORB_CHECK_ARG(k >= 0 && k < K, "mp_obs_kf entry outside [-1, n_keyframes)");
            ORB_CHECK_ARG(o->mp_obs_idx[e] >= 0 && o->mp_obs_idx[e] < o->kf_cap, "mp_obs_idx entry outside [0, kf_cap)");
            ORB_CHECK_ARG(k != last, "a keyframe twice in a map point's observations");
            ORB_CHECK_ARG(k > last, "a map point's observations do not ascend in keyframe slot");
            last = k;
        }
    }
    if ((rc = mm_check_rows_distinct(K, M, o->kf_cap, o->kf_n, o->kf_mappoint))) return rc;
    if (replace && (rc = check_range(o->mp_replaced, M, -1, M, "mp_replaced outside [-1, n_mappoints)"))) return rc;
    return ORB_OK;
}

void mm_observe_add(Mirror& io, orbmm_observe& d, bool replace) {
    const size_t K = d.n_keyframes, M = d.n_mappoints, n_obs = d.n_obs;
    io.add(d.kf_n, K, true, false); io.add(d.kf_mappoint, K * d.kf_cap, true, true); io.add(d.kf_uright, K * d.kf_cap, true, false);
    io.add(d.mp_bad, M, true, replace); io.add(d.mp_nobs, M, true, true); io.add(d.mp_obs_off, M + 1, true, false);
    io.add(d.mp_obs_kf, n_obs, true, true); io.add(d.mp_obs_idx, n_obs, true, true);
    if (replace) {
        io.add(d.mp_found, M, true, true); io.add(d.mp_visible, M, true, true); io.add(d.mp_replaced, M, true, true);
    }
}

int mm_apply_check(const orbmm_observe* o, const orbmm_apply* a) {
    ORB_CHECK_ARG(a, "null apply list");
    ORB_CHECK_ARG(a->mode == ORBMM_APPLY_FUSE || a->mode == ORBMM_APPLY_FUSE_SIM3 || a->mode == ORBMM_APPLY_LOOP_MATCHED,
                  "unknown apply mode");
    ORB_CHECK_ARG(a->n_items >= 0 && a->n_entries >= 0, "negative sizes");
    ORB_CHECK_ARG(a->mp_begin && (a->n_items == 0 || (a->item_kf && a->n_fused)), "null item array");
    ORB_CHECK_ARG(a->n_entries == 0 || (a->point && a->best_idx), "null entry array");
    ORB_CHECK_ARG(a->mode != ORBMM_APPLY_FUSE_SIM3 || a->n_entries == 0 || a->replace_point, "null replace_point");
    ORB_CHECK_ARG(a->n_touched && a->progress && a->status && (o->n_mappoints == 0 || a->touched), "null output");
    return ORB_OK;
}

int mm_apply_check_host(const orbmm_observe* o, const orbmm_apply* a) {
    int rc;
    if ((rc = check_csr(a->mp_begin, a->n_items, a->n_entries, "mp_begin"))) return rc;
    if ((rc = check_range(a->item_kf, a->n_items, 0, o->n_keyframes, "item_kf outside [0, n_keyframes)"))) return rc;
    if ((rc = check_range(a->point, a->n_entries, -1, o->n_mappoints, "point outside [-1, n_mappoints)"))) return rc;
    if ((rc = check_range(a->best_idx, a->n_entries, -1, o->kf_cap, "best_idx outside [-1, kf_cap)"))) return rc;
    if (a->mode == ORBMM_APPLY_FUSE_SIM3 &&
        (rc = check_range(a->replace_point, a->n_entries, -1, o->n_mappoints, "replace_point outside [-1, n_mappoints)")))
        return rc;
    const int32_t* pr = a->progress;
    ORB_CHECK_ARG(pr[0] >= 0 && pr[0] <= a->n_items && pr[1] >= 0 && pr[1] <= (a->mode == ORBMM_APPLY_FUSE_SIM3 ? 1 : 0) && pr[2] >= 0 &&
                      pr[2] <= (pr[0] < a->n_items ? a->mp_begin[pr[0] + 1] - a->mp_begin[pr[0]] : 0),
                  "progress outside the list");
    if (pr[0] || pr[1] || pr[2]) {
        ORB_CHECK_ARG(*a->n_touched >= 0 && *a->n_touched <= o->n_mappoints, "n_touched outside [0, n_mappoints]");
        if ((rc = check_range(a->touched, *a->n_touched, 0, o->n_mappoints, "touched entry outside [0, n_mappoints)"))) return rc;
    }
    return ORB_OK;
}

int mm_grow_check(int32_t M, int32_t n_obs, const int32_t* off, const int32_t* kf, const int32_t* idx, int32_t slack,
                  int32_t n_obs_out, int32_t* out_off, int32_t* out_kf, int32_t* out_idx, int32_t* status) {
    ORB_CHECK_ARG(M >= 0 && n_obs >= 0 && n_obs_out >= 0 && slack >= 0, "negative sizes");
    ORB_CHECK_ARG((long long)n_obs + n_obs_out < MM_MAX_ENTRIES && (long long)n_obs + slack < MM_MAX_ENTRIES, "a table of 2^31 entries or more");
    ORB_CHECK_ARG(off && out_off && status && (n_obs == 0 || (kf && idx)) && (n_obs_out == 0 || (out_kf && out_idx)),
                  "null observation array");
    return ORB_OK;
}

}  // namespace

extern "C" int orbmm_add_keyframe_observations_device(const orbmm_observe* o, int32_t cur, int32_t* added, int32_t* recent_out,
                                                      int32_t* counts, int32_t* status, void* stream) {
    int rc;
    if ((rc = mm_observe_check(o, false))) return rc;
    ORB_CHECK_ARG(added && recent_out && counts && status, "null output");
    if ((rc = mm_use_current_device())) return rc;
    hipStream_t st = (hipStream_t)stream;
    if ((rc = g_mm.ws.reserve(std::max<size_t>(o->kf_cap, 256)))) return rc;
    uint8_t* kind = g_mm.ws.as<uint8_t>();
    const MmObserve t = mm_observe(*o);
    if (cur >= 0 && cur < t.K)
        hipLaunchKernelGGL(mm_obs_new_kernel, dim3((t.kf_cap + 255) / 256), dim3(256), 0, st, t, cur, kind, status);
    else
        ORB_HIP_TRY(hipMemsetAsync(status, 0, (size_t)t.kf_cap * 4, st));
    hipLaunchKernelGGL(mm_obs_lists_kernel, dim3(1), dim3(64 * MM_CULL_WAVES), 0, st, t, cur, kind, added, recent_out, counts);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbmm_fuse_apply_device(const orbmm_observe* o, const orbmm_apply* a, void* stream) {
    int rc;
    if ((rc = mm_observe_check(o, true))) return rc;
    if ((rc = mm_apply_check(o, a))) return rc;
    if ((rc = mm_use_current_device())) return rc;
    if ((rc = g_mm.ws.reserve(4 * std::max<size_t>(obs_scratch_entries(o->n_mappoints, o->n_obs), 64)))) return rc;
    const MmApply w{a->mode, a->n_items, a->n_entries, a->item_kf, a->mp_begin, a->point, a->best_idx, a->replace_point,
                    a->n_fused, a->touched, a->n_touched, a->progress, a->status};
    hipLaunchKernelGGL(mm_obs_apply_kernel, dim3(1), dim3(64 * MM_CULL_WAVES), 0, (hipStream_t)stream, mm_observe(*o), w,
                       g_mm.ws.as<int32_t>());
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbmm_grow_observations_device(int32_t n_mappoints, int32_t n_obs, const int32_t* mp_obs_off,
                                              const int32_t* mp_obs_kf, const int32_t* mp_obs_idx, int32_t slack,
                                              const int32_t* extra, int32_t n_obs_out, int32_t* out_off, int32_t* out_kf,
                                              int32_t* out_idx, int32_t* status, void* stream) {
    int rc;
    if ((rc = mm_grow_check(n_mappoints, n_obs, mp_obs_off, mp_obs_kf, mp_obs_idx, slack, n_obs_out, out_off, out_kf, out_idx, status)))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const int M = n_mappoints;
    const dim3 grid((M + 255) / 256);
    if (M)
        hipLaunchKernelGGL(mm_grow_count_kernel, grid, dim3(256), 0, st, M, n_obs, mp_obs_off, mp_obs_kf, slack, extra, n_obs_out,
                           out_off);
    hipLaunchKernelGGL(mm_grow_scan_kernel, dim3(1), dim3(256), 0, st, M, n_obs_out, out_off, status);
    if (M)
        hipLaunchKernelGGL(mm_grow_fill_kernel, grid, dim3(256), 0, st, M, n_obs, mp_obs_off, mp_obs_kf, mp_obs_idx, n_obs_out,
                           out_off, out_kf, out_idx);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbmm_add_keyframe_observations(const orbmm_observe* o, int32_t cur, int32_t* added, int32_t* recent_out,
                                               int32_t* counts, int32_t* status, int device) {
    int rc;
    if ((rc = mm_observe_check(o, false))) return rc;
    ORB_CHECK_ARG(added && recent_out && counts && status, "null output");
    if ((rc = mm_observe_check_host(o, false))) return rc;   // before any copy
    ORB_CHECK_ARG(cur >= 0 && cur < o->n_keyframes, "cur outside [0, n_keyframes)");
    orbmm_observe d = *o;
    d.mp_found = d.mp_visible = d.mp_replaced = nullptr;
    Mirror io;
    mm_observe_add(io, d, false);
    const size_t cap = o->kf_cap;
    io.add(added, cap, false, true); io.add(recent_out, cap, false, true); io.add(counts, 2, false, true); io.add(status, cap, false, true);
    return run_host(g_mm, device, io, [&] {
        return orbmm_add_keyframe_observations_device(&d, cur, added, recent_out, counts, status, nullptr);
    });
}

extern "C" int orbmm_fuse_apply(const orbmm_observe* o, const orbmm_apply* a, int device) {
    int rc;
    if ((rc = mm_observe_check(o, true))) return rc;
    if ((rc = mm_apply_check(o, a))) return rc;
    if ((rc = mm_observe_check_host(o, true))) return rc;   // before any copy
    if ((rc = mm_apply_check_host(o, a))) return rc;
    orbmm_observe d = *o;
    orbmm_apply w = *a;
    Mirror io;
    mm_observe_add(io, d, true);
    const size_t I = a->n_items, E = a->n_entries;
    io.add(w.item_kf, I, true, false); io.add(w.mp_begin, I + 1, true, false); io.add(w.point, E, true, false);
    io.add(w.best_idx, E, true, false); io.add(w.replace_point, E, true, true); io.add(w.n_fused, I, true, true);
    io.add(w.touched, (size_t)o->n_mappoints, true, true); io.add(w.n_touched, 1, true, true); io.add(w.progress, 4, true, true);
    io.add(w.status, 1, false, true);
    return run_host(g_mm, device, io, [&] { return orbmm_fuse_apply_device(&d, &w, nullptr); });
}

extern "C" int orbmm_grow_observations(int32_t n_mappoints, int32_t n_obs, const int32_t* mp_obs_off, const int32_t* mp_obs_kf,
                                       const int32_t* mp_obs_idx, int32_t slack, const int32_t* extra, int32_t n_obs_out,
                                       int32_t* out_off, int32_t* out_kf, int32_t* out_idx, int32_t* status, int device) {
    int rc;
    if ((rc = mm_grow_check(n_mappoints, n_obs, mp_obs_off, mp_obs_kf, mp_obs_idx, slack, n_obs_out, out_off, out_kf, out_idx, status)))
        return rc;
    if ((rc = check_csr(mp_obs_off, n_mappoints, n_obs, "mp_obs"))) return rc;   // before any copy
    if (extra && (rc = check_range(extra, n_mappoints, 0, 0x7fffffff, "extra must not be negative"))) return rc;
    const size_t M = n_mappoints;
    Mirror io;
    io.add(mp_obs_off, M + 1, true, false); io.add(mp_obs_kf, (size_t)n_obs, true, false); io.add(mp_obs_idx, (size_t)n_obs, true, false);
    io.add(extra, M, true, false);
    io.add(out_off, M + 1, false, true); io.add(out_kf, (size_t)n_obs_out, true, true); io.add(out_idx, (size_t)n_obs_out, true, true);
    io.add(status, 1, false, true);
    return run_host(g_mm, device, io, [&] {
        return orbmm_grow_observations_device(n_mappoints, n_obs, mp_obs_off, mp_obs_kf, mp_obs_idx, slack, extra, n_obs_out,
                                              out_off, out_kf, out_idx, status, nullptr);
    });
}
