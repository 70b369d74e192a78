// orbmk.hip — where the map grows, on gfx950: the KeyFrame constructor on a batch of frames and the MapPoint constructor
// with AddObservation / AddMapPoint / Map::AddMapPoint on a batch of lists, in place on the slot tables
// (include/orbslam2_amd.h, "Map creation"; the rules are csrc/mk_create.h's).  The lane groups and the scan are
// csrc/mm_groups.h's.
//   mk_insert_kernel   grid (ceil(kf_cap / 256), item): one thread per keypoint row of the keyframe; the item's first
//                      workgroup also writes the constructor state and the padded connection rows
//   mk_count_kernel    grid (chunk, item): the valid entries of 256 list positions
//   mk_decide_kernel   one workgroup: the 64-bit scan of the chunk counts, the rows of the slots the batch would take (a
//                      binary search of the offsets gives a slot's item), then status, needed, alloc and n_recent
//   mk_fill_kernel     grid (chunk, item): an entry's number is its chunk's offset plus its rank among the chunk's valid
//                      entries; one thread builds one point
// No atomics: a slot number depends on the lists alone, so two runs are byte-identical.
// Intended range: a keyframe's batch, tens of items and hundreds to a few thousand points.  mk_decide_kernel is one workgroup
// and serial in the batch: it scans n_items * chunks counts and walks every slot the batch would take; a batch near the
// permitted maximum (65535 items) stays correct but spends its time there.
#include <algorithm>
#include <set>
#include <utility>

#include "common.h"
#include "mk_create.h"
#include "mm_groups.h"

namespace orbamd {

static_assert(MK_CHUNK == 64 * MM_CULL_WAVES, "a chunk is one MmBlock");
static_assert(sizeof(MkKeypoint) == sizeof(orbx_keypoint) && sizeof(MkDesc) == 32, "the record layouts");

__global__ __launch_bounds__(256) void mk_insert_kernel(MkFrames fr, MkKeyframes t, MkItems a) {
    const int it = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    int f, k;
    if (!mk_item(fr, t, a, it, f, k)) return;
    if (i < t.kf_cap) mk_insert_keypoint(fr, t, f, k, i);
    if (blockIdx.x == 0)
        for (int q = threadIdx.x; q < MK_HEAD_ENTRIES + t.conn_cap; q += 256) mk_insert_head(fr, t, a, it, f, k, q);
}

__global__ __launch_bounds__(MK_CHUNK) void mk_count_kernel(MkMap t, MkLists l, int32_t* count) {
    __shared__ int32_t s_red[MM_CULL_WAVES];
    const MmBlock b{(int)threadIdx.x, s_red};
    const int i = blockIdx.y, j = blockIdx.x * MK_CHUNK + threadIdx.x;
    const int n = b.sum(j < mk_list_n(l, i) && mk_entry_valid(t, l, i, j) ? 1 : 0);
    if (b.lane == 0) count[(size_t)i * gridDim.x + blockIdx.x] = n;
}

// ws: base, recent base, the decision, a spare word, then the offsets of n_items * chunks counts (in place) and the total
__global__ __launch_bounds__(256) void mk_decide_kernel(MkMap t, MkLists l, MkOut o, int32_t* ws) {
    __shared__ int32_t s_red[MM_CULL_WAVES];
    const MmBlock b{(int)threadIdx.x, s_red};
    int32_t* off = ws + 4;
    const int nc = mk_chunks(l.list_cap), n = l.n_items * nc;
    const int base = mk_base(t, o), recent_base = mk_recent_base(o);
    const long long total = mm_block_scan<long long>(off, n, off, 0, MK_CHUNK, 0, (long long)t.M + 1);
    __syncthreads();   // the offsets are written, alloc and n_recent have been read
    int short_slot = 0x7fffffff;
    if (base + total <= t.M)   // no offset was capped
        for (int r = threadIdx.x; r < total; r += 256) {
            int lo = 0, hi = n - 1;   // the chunk of entry r: the first c with off[c + 1] > r
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (off[mid + 1] > r) hi = mid;
                else lo = mid + 1;
            }
            if (!mk_row_fits(t, base + r, mk_need(l, lo / nc))) {
                short_slot = base + r;
                break;
            }
        }
    short_slot = b.min(short_slot);
    if (threadIdx.x == 0) {
        ws[0] = base;
        ws[1] = recent_base;
        ws[2] = mk_decide(t, o, base, recent_base, total, short_slot == 0x7fffffff ? -1 : short_slot);
    }
}

__global__ __launch_bounds__(MK_CHUNK) void mk_fill_kernel(MkMap t, MkLists l, MkOut o, const int32_t* ws) {
    __shared__ int32_t s_red[MM_CULL_WAVES];
    const MmBlock b{(int)threadIdx.x, s_red};
    const int32_t* off = ws + 4;
    const int i = blockIdx.y, c = blockIdx.x, j = c * MK_CHUNK + threadIdx.x;
    const bool ok = ws[2] == MK_OK;
    const bool valid = ok && j < mk_list_n(l, i) && mk_entry_valid(t, l, i, j);
    int total;
    const int r = off[(size_t)i * gridDim.x + c] + b.prefix(valid, total);
    const long long p = (long long)ws[0] + r, recent_at = (long long)ws[1] + r;
    // (what the decision guarantees, tested again: the lists are the caller's memory)
    if (valid && p < t.M && mk_row_fits(t, (int)p, mk_need(l, i)) && (!o.recent || recent_at < o.recent_cap))
        mk_create_point(t, l, o, i, j, (int)p, (int)recent_at);
    else if (j < l.list_cap && o.created)
        o.created[(size_t)i * l.list_cap + j] = -1;
    if (c == 0 && threadIdx.x == 0 && o.n_created)
        o.n_created[i] = ok ? off[((size_t)i + 1) * gridDim.x] - off[(size_t)i * gridDim.x] : 0;
}

}  // namespace orbamd

using namespace orbamd;

namespace {

thread_local Scratch g_mk;

constexpr long long MK_MAX_ENTRIES = 0x7fffffffLL;

bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

MkFrames mk_frames(const orbmk_frames& f) {
    return MkFrames{f.n_frames, f.kp_cap, f.frame_n, f.frame_mappoint, reinterpret_cast<const MkKeypoint*>(f.kp_un), f.kp_octave,
                    f.kp_uright, f.kp_depth, reinterpret_cast<const MkDesc*>(f.kp_desc), f.pose, f.camera};
}

MkKeyframes mk_keyframes(const orbmk_keyframes& k) {
    return MkKeyframes{k.n_keyframes, k.kf_cap, k.conn_cap, k.kf_id, k.kf_n, k.kf_mappoint, reinterpret_cast<MkKeypoint*>(k.kf_keypoint),
                       k.kf_kp_octave, k.kf_uright, k.kf_depth, reinterpret_cast<MkDesc*>(k.kf_desc), k.kf_pose, k.kf_camera, k.kf_bad,
                       k.kf_not_erase, k.kf_to_be_erased, k.kf_parent, k.kf_first_connection, k.conn_slot, k.conn_weight, k.n_conn,
                       k.ord_slot, k.ord_weight, k.n_ord, k.kf_covis};
}

int mk_insert_check(const orbmk_frames* f, const orbmk_keyframes* k, int32_t n_items, const int32_t* item_frame, const int32_t* item_kf,
                    const int32_t* item_id, const float* item_baseline) {
    ORB_CHECK_ARG(f && k, "null frames or keyframe tables");
    ORB_CHECK_ARG(f->n_frames >= 0 && k->n_keyframes >= 0 && n_items >= 0, "negative sizes");
    ORB_CHECK_ARG(n_items < 65536, "65536 items or more in one call");
    ORB_CHECK_ARG(f->kp_cap >= 1 && k->kf_cap >= 1, "kp_cap and kf_cap must be at least 1");
    ORB_CHECK_ARG(f->kp_cap <= k->kf_cap, "kp_cap must not exceed kf_cap");
    const bool rows = k->conn_slot || k->conn_weight || k->ord_slot || k->ord_weight;
    ORB_CHECK_ARG(k->conn_cap >= (rows ? 1 : 0), "conn_cap must be at least 1");
    ORB_CHECK_ARG((long long)k->n_keyframes * k->kf_cap < MK_MAX_ENTRIES / 8 && (long long)f->n_frames * f->kp_cap < MK_MAX_ENTRIES / 8 &&
                      (long long)k->n_keyframes * std::max(k->conn_cap, 1) < MK_MAX_ENTRIES,
                  "a table of 2^31 entries or more");
    ORB_CHECK_ARG(n_items == 0 || (item_frame && item_kf), "null item array");
    ORB_CHECK_ARG(f->frame_n || n_items == 0, "null frame_n");
    ORB_CHECK_ARG(!k->kf_id || item_id || n_items == 0, "kf_id without item ids");
    ORB_CHECK_ARG(!k->kf_camera || ((item_baseline && f->camera) || n_items == 0), "kf_camera without camera or item baselines");
    ORB_CHECK_ARG((!k->kf_mappoint || f->frame_mappoint) && (!k->kf_keypoint || f->kp_un) && (!k->kf_kp_octave || f->kp_octave) &&
                      (!k->kf_uright || f->kp_uright) && (!k->kf_depth || f->kp_depth) && (!k->kf_desc || f->kp_desc) &&
                      (!k->kf_pose || f->pose),
                  "a keyframe table without its frame array");
    ORB_CHECK_ARG((uintptr_t)k->kf_keypoint % 4 == 0 && (uintptr_t)f->kp_un % 4 == 0, "keypoint records are not aligned");
    return ORB_OK;
}

MkMap mk_map(const orbmk_map& m) {
    return MkMap{m.n_keyframes, m.n_mappoints, m.kf_cap, m.n_obs, m.kf_id, m.kf_n, m.kf_mappoint, m.kf_uright, m.kf_bad,
                 reinterpret_cast<const MkDesc*>(m.kf_desc), m.mp_bad, m.mp_xw, m.mp_normal, m.mp_max_min, m.mp_nobs, m.mp_found,
                 m.mp_visible, m.mp_replaced, m.mp_first_kf_id, m.mp_ref_kf, reinterpret_cast<MkDesc*>(m.mp_desc), m.mp_obs_off,
                 m.mp_obs_kf, m.mp_obs_idx};
}

MkLists mk_lists(const orbmk_lists& l) {
    return MkLists{l.n_items, l.list_cap, l.values_by_keypoint, l.kf1, l.kf2, l.n_list, l.idx1, l.idx2, l.xw, l.normal, l.max_distance,
                   l.min_distance, l.n_frames, l.kp_cap, l.item_frame, l.frame_mappoint};
}

MkOut mk_out(const orbmk_created& o) {
    return MkOut{o.alloc, o.status, o.needed, o.created, o.n_created, o.recent, o.n_recent, o.recent_cap};
}

int mk_create_check(const orbmk_map* m, const orbmk_lists* l, const orbmk_created* o) {
    ORB_CHECK_ARG(m && l && o, "null map, lists or outputs");
    ORB_CHECK_ARG(m->n_keyframes >= 0 && m->n_mappoints >= 0 && m->n_obs >= 0 && l->n_items >= 0, "negative sizes");
    ORB_CHECK_ARG(l->n_items < 65536, "65536 items or more in one call");
    ORB_CHECK_ARG(m->kf_cap >= 1, "kf_cap must be at least 1");
    ORB_CHECK_ARG(l->list_cap >= 1, "list_cap must be at least 1");
    ORB_CHECK_ARG(l->values_by_keypoint == 0 || l->values_by_keypoint == 1, "values_by_keypoint must be 0 or 1");
    ORB_CHECK_ARG((long long)m->n_keyframes * m->kf_cap < MK_MAX_ENTRIES / 8 && 3LL * m->n_mappoints < MK_MAX_ENTRIES &&
                      m->n_obs < MK_MAX_ENTRIES && 3LL * l->n_items * l->list_cap < MK_MAX_ENTRIES,
                  "a table of 2^31 entries or more");
    ORB_CHECK_ARG(m->kf_id && m->kf_n && m->kf_mappoint && m->kf_uright, "null keyframe table");
    ORB_CHECK_ARG(m->mp_bad && m->mp_xw && m->mp_nobs && m->mp_found && m->mp_visible && m->mp_replaced && m->mp_first_kf_id &&
                      m->mp_ref_kf && m->mp_obs_off && m->mp_obs_kf && m->mp_obs_idx,
                  "null map-point table");
    ORB_CHECK_ARG(!m->kf_desc == !m->mp_desc, "kf_desc and mp_desc go together");
    ORB_CHECK_ARG(l->n_items == 0 || (l->kf1 && l->n_list && l->idx1 && l->xw), "null list array");
    ORB_CHECK_ARG(!l->kf2 || l->idx2 || l->n_items == 0, "kf2 without idx2");
    ORB_CHECK_ARG(!l->frame_mappoint || (l->item_frame && l->n_frames >= 0 && l->kp_cap >= 1 &&
                                         (long long)l->n_frames * l->kp_cap < MK_MAX_ENTRIES),
                  "frame_mappoint without item_frame, n_frames or kp_cap");
    ORB_CHECK_ARG(o->alloc && o->status && o->needed, "null output");
    ORB_CHECK_ARG(!o->recent || (o->n_recent && o->recent_cap >= 0), "recent without n_recent or recent_cap");
    return ORB_OK;
}

}  // namespace

extern "C" int orbmk_insert_keyframes_device(const orbmk_frames* fr, const orbmk_keyframes* kf, int32_t n_items,
                                             const int32_t* item_frame, const int32_t* item_kf, const int32_t* item_id,
                                             const float* item_baseline, void* stream) {
    int rc;
    if ((rc = mk_insert_check(fr, kf, n_items, item_frame, item_kf, item_id, item_baseline))) return rc;
    ORB_CHECK_ARG(aligned16(kf->kf_desc) && (!kf->kf_desc || aligned16(fr->kp_desc)), "descriptors must be 16-byte aligned");
    if (n_items == 0) return ORB_OK;
    hipLaunchKernelGGL(mk_insert_kernel, dim3((kf->kf_cap + 255) / 256, n_items), dim3(256), 0, (hipStream_t)stream, mk_frames(*fr),
                       mk_keyframes(*kf), MkItems{n_items, item_frame, item_kf, item_id, item_baseline});
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbmk_create_points_device(const orbmk_map* map, const orbmk_lists* lists, const orbmk_created* out, void* stream) {
    int rc;
    if ((rc = mk_create_check(map, lists, out))) return rc;
    ORB_CHECK_ARG(aligned16(map->kf_desc) && aligned16(map->mp_desc), "descriptors must be 16-byte aligned");
    if ((rc = g_mk.use_current_device())) return rc;
    const int nc = mk_chunks(lists->list_cap);
    if ((rc = g_mk.ws.reserve(4 * ((size_t)lists->n_items * nc + 5)))) return rc;
    int32_t* ws = g_mk.ws.as<int32_t>();
    hipStream_t st = (hipStream_t)stream;
    const MkMap t = mk_map(*map);
    const MkLists l = mk_lists(*lists);
    const MkOut o = mk_out(*out);
    const dim3 grid(nc, std::max(l.n_items, 1));
    if (l.n_items) hipLaunchKernelGGL(mk_count_kernel, grid, dim3(MK_CHUNK), 0, st, t, l, ws + 4);
    hipLaunchKernelGGL(mk_decide_kernel, dim3(1), dim3(256), 0, st, t, l, o, ws);
    if (l.n_items) hipLaunchKernelGGL(mk_fill_kernel, grid, dim3(MK_CHUNK), 0, st, t, l, o, ws);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbmk_insert_keyframes(const orbmk_frames* fr, const orbmk_keyframes* kf, int32_t n_items, const int32_t* item_frame,
                                      const int32_t* item_kf, const int32_t* item_id, const float* item_baseline, int device) {
    int rc;
    if ((rc = mk_insert_check(fr, kf, n_items, item_frame, item_kf, item_id, item_baseline))) return rc;
    if (n_items == 0) return ORB_OK;
    if ((rc = check_range(item_frame, n_items, 0, fr->n_frames, "item_frame outside [0, n_frames)"))) return rc;   // before any copy
    if ((rc = check_range(item_kf, n_items, 0, kf->n_keyframes, "item_kf outside [0, n_keyframes)"))) return rc;
    if ((rc = check_range(fr->frame_n, fr->n_frames, 0, fr->kp_cap + 1, "frame_n outside [0, kp_cap]"))) return rc;
    std::set<int32_t> seen;
    for (int i = 0; i < n_items; i++) ORB_CHECK_ARG(seen.insert(item_kf[i]).second, "a keyframe slot twice in the items");
    orbmk_frames f = *fr;
    orbmk_keyframes k = *kf;
    const size_t F = f.n_frames, pc = f.kp_cap, K = k.n_keyframes, kc = k.kf_cap, cc = k.conn_cap, I = n_items;
    Mirror io;
    io.add(item_frame, I, true, false); io.add(item_kf, I, true, false); io.add(item_id, I, true, false);
    io.add(item_baseline, I, true, false);
    io.add(f.frame_n, F, true, false); io.add(f.frame_mappoint, F * pc, true, false); io.add(f.kp_un, F * pc, true, false);
    io.add(f.kp_octave, F * pc, true, false); io.add(f.kp_uright, F * pc, true, false); io.add(f.kp_depth, F * pc, true, false);
    io.add(f.kp_desc, F * pc * 32, true, false); io.add(f.pose, F * 12, true, false); io.add(f.camera, F * 5, true, false);
    // (every row goes up, so that what is not written comes back as the caller left it)
    io.add(k.kf_id, K, true, true); io.add(k.kf_n, K, true, true); io.add(k.kf_mappoint, K * kc, true, true);
    io.add(k.kf_keypoint, K * kc, true, true); io.add(k.kf_kp_octave, K * kc, true, true); io.add(k.kf_uright, K * kc, true, true);
    io.add(k.kf_depth, K * kc, true, true); io.add(k.kf_desc, K * kc * 32, true, true); io.add(k.kf_pose, K * 12, true, true);
    io.add(k.kf_camera, K * 6, true, true); io.add(k.kf_bad, K, true, true); io.add(k.kf_not_erase, K, true, true);
    io.add(k.kf_to_be_erased, K, true, true); io.add(k.kf_parent, K, true, true); io.add(k.kf_first_connection, K, true, true);
    io.add(k.conn_slot, K * cc, true, true); io.add(k.conn_weight, K * cc, true, true); io.add(k.n_conn, K, true, true);
    io.add(k.ord_slot, K * cc, true, true); io.add(k.ord_weight, K * cc, true, true); io.add(k.n_ord, K, true, true);
    io.add(k.kf_covis, K * MK_COVIS, true, true);
    return run_host(g_mk, device, io, [&] {
        return orbmk_insert_keyframes_device(&f, &k, n_items, item_frame, item_kf, item_id, item_baseline, nullptr);
    });
}

extern "C" int orbmk_create_points(const orbmk_map* map, const orbmk_lists* lists, const orbmk_created* out, int device) {
    int rc;
    if ((rc = mk_create_check(map, lists, out))) return rc;
    const int K = map->n_keyframes, M = map->n_mappoints, I = lists->n_items, lc = lists->list_cap;
    if ((rc = check_csr(map->mp_obs_off, M, map->n_obs, "mp_obs"))) return rc;   // before any copy
    if ((rc = check_range(map->kf_n, K, 0, map->kf_cap + 1, "kf_n outside [0, kf_cap]"))) return rc;
    if ((rc = check_range(lists->kf1, I, 0, K, "kf1 outside [0, n_keyframes)"))) return rc;
    if (lists->kf2 && (rc = check_range(lists->kf2, I, -1, K, "kf2 outside [-1, n_keyframes)"))) return rc;
    if ((rc = check_range(lists->n_list, I, 0, lc + 1, "n_list outside [0, list_cap]"))) return rc;
    if (lists->frame_mappoint && (rc = check_range(lists->item_frame, I, -1, lists->n_frames, "item_frame outside [-1, n_frames)")))
        return rc;
    ORB_CHECK_ARG(out->alloc[0] >= 0 && out->alloc[0] <= M, "alloc outside [0, n_mappoints]");
    ORB_CHECK_ARG(!out->recent || (out->n_recent[0] >= 0 && out->n_recent[0] <= out->recent_cap), "n_recent outside [0, recent_cap]");
    const MkMap t = mk_map(*map);
    const MkLists l = mk_lists(*lists);
    std::set<std::pair<int32_t, int32_t>> seen;
    for (int i = 0; i < I; i++) {
        const size_t row = (size_t)i * lc;
        if ((rc = check_range(l.idx1 + row, l.n_list[i], -1, t.kf_cap, "idx1 outside [-1, kf_cap)"))) return rc;
        if (l.kf2 && l.kf2[i] >= 0 && (rc = check_range(l.idx2 + row, l.n_list[i], -1, t.kf_cap, "idx2 outside [-1, kf_cap)"))) return rc;
        for (int j = 0; j < l.n_list[i]; j++) {
            if (!mk_entry_valid(t, l, i, j)) continue;
            ORB_CHECK_ARG(seen.insert({l.kf1[i], l.idx1[row + j]}).second, "a keypoint of a keyframe twice in the lists");
            if (mk_second(t, l, i) >= 0)
                ORB_CHECK_ARG(seen.insert({l.kf2[i], l.idx2[row + j]}).second, "a keypoint of a keyframe twice in the lists");
        }
    }
    orbmk_map m = *map;
    orbmk_lists d = *lists;
    orbmk_created o = *out;
    const size_t Kc = (size_t)K * m.kf_cap, Ms = M, n_obs = m.n_obs, E = (size_t)I * lc, Fk = (size_t)std::max(d.n_frames, 0) * std::max(d.kp_cap, 0);
    Mirror io;
    io.add(m.kf_id, (size_t)K, true, false); io.add(m.kf_n, (size_t)K, true, false); io.add(m.kf_mappoint, Kc, true, true);
    io.add(m.kf_uright, Kc, true, false); io.add(m.kf_bad, (size_t)K, true, false); io.add(m.kf_desc, Kc * 32, true, false);
    io.add(m.mp_bad, Ms, true, true); io.add(m.mp_xw, Ms * 3, true, true); io.add(m.mp_normal, Ms * 3, true, true);
    io.add(m.mp_max_min, Ms * 2, true, true); io.add(m.mp_nobs, Ms, true, true); io.add(m.mp_found, Ms, true, true);
    io.add(m.mp_visible, Ms, true, true); io.add(m.mp_replaced, Ms, true, true); io.add(m.mp_first_kf_id, Ms, true, true);
    io.add(m.mp_ref_kf, Ms, true, true); io.add(m.mp_desc, Ms * 32, true, true); io.add(m.mp_obs_off, Ms + 1, true, false);
    io.add(m.mp_obs_kf, n_obs, true, true); io.add(m.mp_obs_idx, n_obs, true, true);
    io.add(d.kf1, (size_t)I, true, false); io.add(d.kf2, (size_t)I, true, false); io.add(d.n_list, (size_t)I, true, false);
    io.add(d.idx1, E, true, false); io.add(d.idx2, E, true, false); io.add(d.xw, E * 3, true, false); io.add(d.normal, E * 3, true, false);
    io.add(d.max_distance, E, true, false); io.add(d.min_distance, E, true, false); io.add(d.item_frame, (size_t)I, true, false);
    if (d.frame_mappoint) io.add(d.frame_mappoint, Fk, true, true);
    io.add(o.alloc, 1, true, true); io.add(o.status, 1, false, true); io.add(o.needed, 2, false, true);
    io.add(o.created, E, false, true); io.add(o.n_created, (size_t)I, false, true);
    io.add(o.recent, (size_t)std::max(o.recent_cap, 0), true, true); io.add(o.n_recent, 1, true, true);
    return run_host(g_mk, device, io, [&] { return orbmk_create_points_device(&m, &d, &o, nullptr); });
}
