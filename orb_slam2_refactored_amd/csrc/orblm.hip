// orblm.hip — LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:380-578) on gfx950, batched over (keyframe 1,
// keyframe 2) pairs on the extractor's slots.
//
//   lm_prepare_kernel      one workgroup per pair: both keyframes' constants (Tcw, Rwc, Ow, camera; lm_newpoint.h),
//                          the baseline, F12, the epipole; for a monocular pair the depths of keyframe 2's MapPoints
//                          into LDS and the element (n - 1) / 2 of their sorted order by rank counting (the lane whose
//                          depth has exactly that many (depth, slot) pairs below it: an exact selection, equal values
//                          tie by slot); the skip flag.  F12 / ep2 in the layout the search reads.
//   lm_triangulate_kernel  one workgroup per pair, lanes over idx1 in tiles of 256: the pair's constants staged in LDS,
//                          one match per lane (the fp64 Jacobi of init_hyp.h on the 4 x 4 A^T A), the created ones
//                          numbered by ballot + mbcnt inside a wavefront and the four wave counts through LDS, so the
//                          compacted list is in ascending idx1 without an atomic; a created point sets its two
//                          MapPoint flags with byte stores.
// orblm_create_new_map_points_device enqueues prepare once and then, round by round, the search
// (orbm_search_for_triangulation_batch_device, unchanged) and the triangulation with writable flags: stream order
// carries keyframe 1's flags from neighbour to neighbour.
#include <algorithm>
#include <cstring>
#include <limits>
#include <vector>

#include "common.h"
#include "lm_newpoint.h"

namespace orbamd {

constexpr int LM_BLOCK = 256;
static_assert(LM_MAX_LEVELS == ORBM_TRI_MAX_LEVELS, "");
static_assert(LM_CREATED == ORBLM_CREATED && LM_NO_MATCH == ORBLM_NO_MATCH && LM_PAIR_SKIPPED == ORBLM_PAIR_SKIPPED &&
                  LM_LOW_PARALLAX == ORBLM_LOW_PARALLAX && LM_W_ZERO == ORBLM_W_ZERO && LM_BEHIND1 == ORBLM_BEHIND1 &&
                  LM_BEHIND2 == ORBLM_BEHIND2 && LM_REPROJ1 == ORBLM_REPROJ1 && LM_REPROJ2 == ORBLM_REPROJ2 &&
                  LM_DIST_ZERO == ORBLM_DIST_ZERO && LM_SCALE == ORBLM_SCALE && LM_BRANCH_STEREO2 == ORBLM_BRANCH_STEREO2,
              "the public enum is the header's");

struct LmArgs {
    int n_pairs, cap1, cap2, n_frames1, n_frames2, monocular;
    const orbx_keypoint *kps1, *kps2;
    const int32_t *counts1, *counts2;
    const float *ur1, *z1, *ur2, *z2;
    const uint8_t* mp2;
    const float* xw2;
    const float *pose1, *pose2, *cam1, *cam2;
    const int32_t *frame1, *frame2;
    orblm_pairs pr;
    const int32_t* match12;
    orblm_points o;
};

__global__ __launch_bounds__(LM_BLOCK) void lm_prepare_kernel(LmArgs a) {
    __shared__ float depth[ORBLM_MAX_KP];
    __shared__ float s_median;
    const int tid = threadIdx.x, p = blockIdx.x;
    const int f1 = a.frame1 ? a.frame1[p] : p, f2 = a.frame2 ? a.frame2[p] : p;
    float* consts = a.pr.consts + 64 * (size_t)p;
    if (f1 < 0 || f1 >= a.n_frames1 || f2 < 0 || f2 >= a.n_frames2) {   // no pair
        if (tid < 64) consts[tid] = 0.f;
        if (tid < 9) a.pr.F12[9 * (size_t)p + tid] = 0.f;
        if (tid < 2) a.pr.ep2[2 * (size_t)p + tid] = 0.f;
        if (tid == 0) {
            a.pr.baseline[p] = 0.f; a.pr.median[p] = 0.f; a.pr.skip[p] = 2;
            a.pr.frame1[p] = 0; a.pr.frame2[p] = 0;
        }
        return;
    }
    LmFrame k1, k2;
    lm_frame(a.pose1 + 12 * (size_t)f1, a.cam1 + 6 * (size_t)f1, k1);
    lm_frame(a.pose2 + 12 * (size_t)f2, a.cam2 + 6 * (size_t)f2, k2);
    float F12[9], ep2[2], baseline;
    lm_pair(k1, k2, F12, ep2, baseline);
    int n = 0;
    float median = 0.f;
    if (a.monocular) {
        const int n2 = min(max(a.counts2[f2], 0), min(a.cap2, ORBLM_MAX_KP));
        const size_t base = (size_t)f2 * a.cap2;
        if (tid == 0) s_median = 0.f;
        for (int j0 = 0; j0 < n2; j0 += LM_BLOCK) {   // block-uniform bounds
            const int j = j0 + tid;
            bool has = false;
            if (j < n2) {
                has = a.mp2[base + j] != 0;
                depth[j] = has ? lm_depth(k2, a.xw2 + 3 * (base + j)) : std::numeric_limits<float>::quiet_NaN();
            }
            n += __syncthreads_count(has);
        }
        __syncthreads();
        if (n > 0) {
            const int target = (n - 1) / 2;
            for (int c = tid; c < n2; c += LM_BLOCK) {
                const float mine = depth[c];
                if (mine != mine) continue;
                int rank = 0;
                for (int o = 0; o < n2; o++) {
                    const float v = depth[o];
                    rank += (v < mine || (v == mine && o < c)) ? 1 : 0;
                }
                if (rank == target) s_median = mine;   // one lane at most, but for NaN depths
            }
            __syncthreads();
            median = s_median;
        }
    }
    const bool skip = lm_skip(a.monocular != 0, baseline, k2, n, median);
    if (tid == 0) {
        const float* s1 = reinterpret_cast<const float*>(&k1);
        const float* s2 = reinterpret_cast<const float*>(&k2);
        for (int i = 0; i < 32; i++) { consts[i] = s1[i]; consts[32 + i] = s2[i]; }
        for (int i = 0; i < 9; i++) a.pr.F12[9 * (size_t)p + i] = F12[i];
        a.pr.ep2[2 * (size_t)p] = ep2[0];
        a.pr.ep2[2 * (size_t)p + 1] = ep2[1];
        a.pr.baseline[p] = baseline; a.pr.median[p] = median; a.pr.skip[p] = skip ? 1 : 0;
        a.pr.frame1[p] = f1; a.pr.frame2[p] = f2;
    }
}

__global__ __launch_bounds__(LM_BLOCK) void lm_triangulate_kernel(LmArgs a, LmTables t) {
    __shared__ float s_consts[64];
    __shared__ int s_wave[LM_BLOCK / 64];
    const int tid = threadIdx.x, p = blockIdx.x;
    const int skip = a.pr.skip[p];
    if (skip == 2) {   // block-uniform
        if (tid == 0) a.o.n_created[p] = 0;
        return;
    }
    const int f1 = a.pr.frame1[p], f2 = a.pr.frame2[p];
    if (f1 < 0 || f1 >= a.n_frames1 || f2 < 0 || f2 >= a.n_frames2) {   // never, after prepare
        if (tid == 0) a.o.n_created[p] = 0;
        return;
    }
    if (tid < 64) s_consts[tid] = a.pr.consts[64 * (size_t)p + tid];
    __syncthreads();
    const LmFrame& k1 = *reinterpret_cast<const LmFrame*>(s_consts);
    const LmFrame& k2 = *reinterpret_cast<const LmFrame*>(s_consts + 32);
    const int n1 = min(max(a.counts1[f1], 0), a.cap1), n2 = min(max(a.counts2[f2], 0), a.cap2);
    const size_t b1 = (size_t)f1 * a.cap1, b2 = (size_t)f2 * a.cap2, bo = (size_t)p * a.cap1;
    const int lane = tid & 63, wave = tid >> 6;
    int total = 0;
    for (int i0 = 0; i0 < n1; i0 += LM_BLOCK) {   // block-uniform bounds
        const int i = i0 + tid;
        bool created = false;
        int m = -1;
        if (i < n1) {
            m = a.match12[bo + i];
            LmPoint r;
            r.status = LM_NO_MATCH; r.branch = LM_BRANCH_NONE;
            r.xw[0] = r.xw[1] = r.xw[2] = 0.f;
            r.normal[0] = r.normal[1] = r.normal[2] = 0.f;
            r.min_distance = 0.f; r.max_distance = 0.f;
            if (m >= 0 && m < n2) {
                if (skip) {
                    r.status = LM_PAIR_SKIPPED;
                } else {
                    const orbx_keypoint q1 = a.kps1[b1 + i], q2 = a.kps2[b2 + m];
                    const float ur1 = a.ur1 ? a.ur1[b1 + i] : -1.f, ur2 = a.ur2 ? a.ur2[b2 + m] : -1.f;
                    const float Z1 = a.z1 ? a.z1[b1 + i] : -1.f, Z2 = a.z2 ? a.z2[b2 + m] : -1.f;
                    lm_match(k1, k2, t, q1.x, q1.y, ur1, Z1, q1.octave, q2.x, q2.y, ur2, Z2, q2.octave, r);
                }
            }
            created = r.status == LM_CREATED;
            a.o.status[bo + i] = r.status;
            a.o.branch[bo + i] = r.branch;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                a.o.xw[3 * (bo + i) + k] = r.xw[k];
                a.o.normal[3 * (bo + i) + k] = r.normal[k];
            }
            a.o.min_distance[bo + i] = r.min_distance;
            a.o.max_distance[bo + i] = r.max_distance;
        }
        const uint64_t bal = __ballot(created);
        const int before = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
        __syncthreads();   // s_wave of the previous tile has been read
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int off = total;
#pragma unroll
        for (int w = 0; w < LM_BLOCK / 64; w++) {
            off += w < wave ? s_wave[w] : 0;
            total += s_wave[w];
        }
        if (created) {   // off + before < n1 <= cap1
            a.o.new_idx1[bo + off + before] = i;
            a.o.new_idx2[bo + off + before] = m;
            if (a.o.has_mappoint1) a.o.has_mappoint1[b1 + i] = 1;
            if (a.o.has_mappoint2) a.o.has_mappoint2[b2 + m] = 1;
        }
    }
    for (int k = total + tid; k < a.cap1; k += LM_BLOCK) {
        a.o.new_idx1[bo + k] = -1;
        a.o.new_idx2[bo + k] = -1;
    }
    if (tid == 0) a.o.n_created[p] = total;
}

thread_local Scratch g_lm;

}  // namespace orbamd

using namespace orbamd;

// The checks every entry shares; n = pairs in the per-pair arrays.
static int lm_common(const orblm_batch* b, const orblm_pairs* pr, long long n, LmArgs& a) {
    ORB_CHECK_ARG(b && pr, "null argument");
    ORB_CHECK_ARG(b->n_pairs >= 0 && b->cap1 > 0 && b->cap2 > 0 && b->n_frames1 >= 0 && b->n_frames2 >= 0,
                  "bad pair count / capacities / keyframe counts");
    ORB_CHECK_ARG(b->n_levels > 0 && b->n_levels <= ORBM_TRI_MAX_LEVELS, "n_levels must be 1..ORBM_TRI_MAX_LEVELS");
    ORB_CHECK_ARG(b->scale_factors1 && b->sigma2_1 && b->scale_factors2 && b->sigma2_2, "null pyramid tables");
    ORB_CHECK_ARG(n * b->cap1 < (1ll << 31) && n <= 65535, "too many pairs");
    ORB_CHECK_ARG(pr->F12 && pr->ep2 && pr->baseline && pr->median && pr->skip && pr->frame1 && pr->frame2 && pr->consts,
                  "null pair array");
    std::memset(&a, 0, sizeof(a));
    if (n == 0) return ORB_OK;
    ORB_CHECK_ARG(b->kps1 && b->counts1 && b->kps2 && b->counts2 && b->pose1 && b->pose2 && b->camera1 && b->camera2,
                  "null keyframe arrays");
    ORB_CHECK_ARG((b->uright1 == nullptr) == (b->depth1 == nullptr) && (b->uright2 == nullptr) == (b->depth2 == nullptr),
                  "uright and depth go together");
    if (b->monocular) {
        ORB_CHECK_ARG(b->has_mappoint2 && b->mp_xw2, "a monocular batch needs has_mappoint2 and mp_xw2");
        ORB_CHECK_ARG(b->cap2 <= ORBLM_MAX_KP, "cap2 exceeds ORBLM_MAX_KP");
    }
    a.n_pairs = (int)n; a.cap1 = b->cap1; a.cap2 = b->cap2; a.n_frames1 = b->n_frames1; a.n_frames2 = b->n_frames2;
    a.monocular = b->monocular ? 1 : 0;
    a.kps1 = b->kps1; a.kps2 = b->kps2; a.counts1 = b->counts1; a.counts2 = b->counts2;
    a.ur1 = b->uright1; a.z1 = b->depth1; a.ur2 = b->uright2; a.z2 = b->depth2;
    a.mp2 = b->has_mappoint2; a.xw2 = b->mp_xw2;
    a.pose1 = b->pose1; a.pose2 = b->pose2; a.cam1 = b->camera1; a.cam2 = b->camera2;
    a.frame1 = b->frame1; a.frame2 = b->frame2;
    a.pr = *pr;
    return ORB_OK;
}

static int lm_points_check(const orblm_points* o) {
    ORB_CHECK_ARG(o, "null argument");
    ORB_CHECK_ARG(o->status && o->branch && o->xw && o->normal && o->min_distance && o->max_distance && o->new_idx1 &&
                      o->new_idx2 && o->n_created,
                  "null output array");
    return ORB_OK;
}

static LmTables lm_tables(const orblm_batch* b) {
    LmTables t{};
    for (int l = 0; l < b->n_levels; l++) {
        t.scale1[l] = b->scale_factors1[l]; t.sigma1[l] = b->sigma2_1[l];
        t.scale2[l] = b->scale_factors2[l]; t.sigma2[l] = b->sigma2_2[l];
    }
    t.n_levels = b->n_levels;
    t.ratio_factor = 1.5f * b->scale_factor;
    return t;
}

static int lm_prepare(const orblm_batch* b, const orblm_pairs* pr, long long n, hipStream_t st) {
    LmArgs a;
    int rc;
    if ((rc = lm_common(b, pr, n, a))) return rc;
    if (n == 0) return ORB_OK;
    hipLaunchKernelGGL(lm_prepare_kernel, dim3((unsigned)n), dim3(LM_BLOCK), 0, st, a);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

// pairs [first, first + count) of arrays holding n pairs
static int lm_triangulate(const orblm_batch* b, const orblm_pairs* pr, const int32_t* match12, const orblm_points* o,
                          long long n, long long first, long long count, hipStream_t st) {
    LmArgs a;
    int rc;
    if ((rc = lm_common(b, pr, n, a))) return rc;
    if ((rc = lm_points_check(o))) return rc;
    if (count == 0) return ORB_OK;
    ORB_CHECK_ARG(match12, "null match12");
    const size_t c1 = (size_t)first * b->cap1;
    a.pr.skip += first; a.pr.frame1 += first; a.pr.frame2 += first; a.pr.consts += 64 * first;
    a.match12 = match12 + c1;
    a.o = *o;
    a.o.status += c1; a.o.branch += c1; a.o.xw += 3 * c1; a.o.normal += 3 * c1; a.o.min_distance += c1; a.o.max_distance += c1;
    a.o.new_idx1 += c1; a.o.new_idx2 += c1; a.o.n_created += first;
    hipLaunchKernelGGL(lm_triangulate_kernel, dim3((unsigned)count), dim3(LM_BLOCK), 0, st, a, lm_tables(b));
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orblm_prepare_pairs_device(const orblm_batch* b, const orblm_pairs* pairs, void* stream) {
    return lm_prepare(b, pairs, b ? b->n_pairs : 0, (hipStream_t)stream);
}

extern "C" int orblm_triangulate_device(const orblm_batch* b, const orblm_pairs* pairs, const int32_t* d_match12,
                                        const orblm_points* out, void* stream) {
    const long long n = b ? b->n_pairs : 0;
    return lm_triangulate(b, pairs, d_match12, out, n, 0, n, (hipStream_t)stream);
}

static int lm_loop_check(const orblm_batch* b, const orbm_tri_batch* s, int32_t n_rounds, const orblm_points* o,
                         const int32_t* match12, const int32_t* nmatches) {
    ORB_CHECK_ARG(b && s && o, "null argument");
    ORB_CHECK_ARG(n_rounds >= 0, "negative n_rounds");
    ORB_CHECK_ARG(match12 && nmatches, "null match12 / nmatches");
    ORB_CHECK_ARG(o->has_mappoint1 && o->has_mappoint2, "the neighbour loop needs writable has_mappoint1 / has_mappoint2");
    ORB_CHECK_ARG(s->desc1 && s->desc2, "null descriptors");
    ORB_CHECK_ARG(b->frame1 && b->frame2, "the neighbour loop needs a plan (frame1 / frame2)");
    return ORB_OK;
}

extern "C" int orblm_create_new_map_points_device(const orblm_batch* b, const orbm_tri_batch* search, int32_t n_rounds,
                                                  const orblm_pairs* pairs, const orblm_points* out, int32_t* d_match12,
                                                  int32_t* d_nmatches, void* stream) {
    int rc;
    if ((rc = lm_loop_check(b, search, n_rounds, out, d_match12, d_nmatches))) return rc;
    const long long P = b->n_pairs, n = P * n_rounds;
    const hipStream_t st = (hipStream_t)stream;
    LmArgs a;
    if ((rc = lm_common(b, pairs, n, a))) return rc;   // every check before the first launch
    if ((rc = lm_points_check(out))) return rc;
    if (n == 0) return ORB_OK;
    if ((rc = lm_prepare(b, pairs, n, st))) return rc;
    orbm_tri_batch s = *search;
    s.n_pairs = (int32_t)P; s.cap1 = b->cap1; s.cap2 = b->cap2;
    s.kps1 = b->kps1; s.counts1 = b->counts1; s.uright1 = b->uright1; s.has_mappoint1 = out->has_mappoint1;
    s.kps2 = b->kps2; s.counts2 = b->counts2; s.uright2 = b->uright2; s.has_mappoint2 = out->has_mappoint2;
    s.n_levels = b->n_levels; s.scale_factors2 = b->scale_factors2; s.sigma2 = b->sigma2_2;
    for (long long r = 0; r < n_rounds; r++) {
        const long long first = r * P;
        s.frame1 = pairs->frame1 + first; s.frame2 = pairs->frame2 + first;
        s.F12 = pairs->F12 + 9 * first; s.ep2 = pairs->ep2 + 2 * first;
        if ((rc = orbm_search_for_triangulation_batch_device(&s, d_match12 + first * b->cap1, d_nmatches + first, stream))) return rc;
        if ((rc = lm_triangulate(b, pairs, d_match12, out, n, first, P, st))) return rc;
    }
    return ORB_OK;
}

// ---- host forms ------------------------------------------------------------------------------------------------

// What the host forms validate before anything is copied; n = pairs.
static int lm_host_check(const orblm_batch* b, long long n) {
    for (int f = 0; f < b->n_frames1; f++) ORB_CHECK_ARG(b->counts1[f] >= 0 && b->counts1[f] <= b->cap1, "counts1 outside [0, cap1]");
    for (int f = 0; f < b->n_frames2; f++) ORB_CHECK_ARG(b->counts2[f] >= 0 && b->counts2[f] <= b->cap2, "counts2 outside [0, cap2]");
    for (long long p = 0; p < n; p++) {
        const int f1 = b->frame1 ? b->frame1[p] : (int)p, f2 = b->frame2 ? b->frame2[p] : (int)p;
        ORB_CHECK_ARG(f1 < b->n_frames1 && f2 < b->n_frames2, "a pair names a keyframe that is not there");
        ORB_CHECK_ARG((f1 < 0) == (f2 < 0), "a pair with one keyframe only");
    }
    for (int f = 0; f < b->n_frames1; f++)
        for (int i = 0; i < b->counts1[f]; i++) {
            const int o = b->kps1[(size_t)f * b->cap1 + i].octave;
            ORB_CHECK_ARG(o >= 0 && o < b->n_levels, "an octave of keyframe set 1 is outside the pyramid");
        }
    for (int f = 0; f < b->n_frames2; f++)
        for (int i = 0; i < b->counts2[f]; i++) {
            const int o = b->kps2[(size_t)f * b->cap2 + i].octave;
            ORB_CHECK_ARG(o >= 0 && o < b->n_levels, "an octave of keyframe set 2 is outside the pyramid");
        }
    return ORB_OK;
}

static void lm_mirror_batch(Mirror& m, orblm_batch& d, long long n) {
    const size_t s1 = (size_t)d.n_frames1 * d.cap1, s2 = (size_t)d.n_frames2 * d.cap2;
    m.add(d.kps1, s1, true, false); m.add(d.counts1, d.n_frames1, true, false);
    m.add(d.uright1, s1, true, false); m.add(d.depth1, s1, true, false);
    m.add(d.kps2, s2, true, false); m.add(d.counts2, d.n_frames2, true, false);
    m.add(d.uright2, s2, true, false); m.add(d.depth2, s2, true, false);
    m.add(d.has_mappoint2, s2, true, false); m.add(d.mp_xw2, 3 * s2, true, false);
    m.add(d.pose1, 12 * (size_t)d.n_frames1, true, false); m.add(d.pose2, 12 * (size_t)d.n_frames2, true, false);
    m.add(d.camera1, 6 * (size_t)d.n_frames1, true, false); m.add(d.camera2, 6 * (size_t)d.n_frames2, true, false);
    m.add(d.frame1, n, true, false); m.add(d.frame2, n, true, false);
}

static void lm_mirror_pairs(Mirror& m, orblm_pairs& q, long long n, bool in) {
    m.add(q.F12, 9 * n, in, !in); m.add(q.ep2, 2 * n, in, !in); m.add(q.baseline, n, in, !in); m.add(q.median, n, in, !in);
    m.add(q.skip, n, in, !in); m.add(q.frame1, n, in, !in); m.add(q.frame2, n, in, !in); m.add(q.consts, 64 * n, in, !in);
}

static void lm_mirror_points(Mirror& m, orblm_points& o, const orblm_batch& b, long long n) {
    const size_t c = (size_t)n * b.cap1;
    m.add(o.status, c, true, true); m.add(o.branch, c, true, true); m.add(o.xw, 3 * c, true, true); m.add(o.normal, 3 * c, true, true);
    m.add(o.min_distance, c, true, true); m.add(o.max_distance, c, true, true);
    m.add(o.new_idx1, c, true, true); m.add(o.new_idx2, c, true, true); m.add(o.n_created, n, true, true);
}

extern "C" int orblm_prepare_pairs(const orblm_batch* b, const orblm_pairs* pairs, int device) {
    LmArgs a;
    int rc;
    const long long n = b ? b->n_pairs : 0;
    if ((rc = lm_common(b, pairs, n, a))) return rc;
    if (n == 0) return ORB_OK;
    if ((rc = lm_host_check(b, n))) return rc;
    orblm_batch d = *b;
    orblm_pairs q = *pairs;
    Mirror m;
    lm_mirror_batch(m, d, n);
    lm_mirror_pairs(m, q, n, false);
    return run_host(g_lm, device, m, [&] { return orblm_prepare_pairs_device(&d, &q, nullptr); });
}

extern "C" int orblm_triangulate(const orblm_batch* b, const orblm_pairs* pairs, const int32_t* match12,
                                 const orblm_points* out, int device) {
    LmArgs a;
    int rc;
    const long long n = b ? b->n_pairs : 0;
    if ((rc = lm_common(b, pairs, n, a))) return rc;
    if ((rc = lm_points_check(out))) return rc;
    if (n == 0) return ORB_OK;
    ORB_CHECK_ARG(match12, "null match12");
    if ((rc = lm_host_check(b, n))) return rc;
    for (long long p = 0; p < n; p++) {
        ORB_CHECK_ARG(pairs->skip[p] >= 0 && pairs->skip[p] <= 2, "skip must be 0, 1 or 2");
        ORB_CHECK_ARG(pairs->frame1[p] >= 0 && pairs->frame1[p] < b->n_frames1 && pairs->frame2[p] >= 0 &&
                          pairs->frame2[p] < b->n_frames2, "pairs name a keyframe that is not there");
    }
    orblm_batch d = *b;
    orblm_pairs q = *pairs;
    orblm_points o = *out;
    const int32_t* dm = match12;
    Mirror m;
    lm_mirror_batch(m, d, n);
    lm_mirror_pairs(m, q, n, true);
    lm_mirror_points(m, o, d, n);
    m.add(dm, (size_t)n * b->cap1, true, false);
    m.add(o.has_mappoint1, (size_t)b->n_frames1 * b->cap1, true, true);
    m.add(o.has_mappoint2, (size_t)b->n_frames2 * b->cap2, true, true, true);   // may be has_mappoint1
    return run_host(g_lm, device, m, [&] { return orblm_triangulate_device(&d, &q, dm, &o, nullptr); });
}

extern "C" int orblm_create_new_map_points(const orblm_batch* b, const orbm_tri_batch* search, int32_t n_rounds,
                                           const orblm_pairs* pairs, const orblm_points* out, int32_t* match12,
                                           int32_t* nmatches, int device) {
    LmArgs a;
    int rc;
    if ((rc = lm_loop_check(b, search, n_rounds, out, match12, nmatches))) return rc;
    const long long P = b->n_pairs, n = P * n_rounds;
    if ((rc = lm_common(b, pairs, n, a))) return rc;
    if ((rc = lm_points_check(out))) return rc;
    if (n == 0) return ORB_OK;
    ORB_CHECK_ARG(!search->fv_node1 && !search->fv_off1 && !search->fv_idx1 && !search->fv_n_nodes1 && !search->fv_node2 &&
                      !search->fv_off2 && !search->fv_idx2 && !search->fv_n_nodes2,
                  "the host form searches without FeatureVectors");
    if ((rc = lm_host_check(b, n))) return rc;
    // the plan's precondition: within a round no keyframe's flags have two writers
    const bool same = (const void*)out->has_mappoint1 == (const void*)out->has_mappoint2;
    std::vector<uint8_t> seen1(b->n_frames1), seen2(b->n_frames2);
    for (int r = 0; r < n_rounds; r++) {
        std::fill(seen1.begin(), seen1.end(), 0);
        std::fill(seen2.begin(), seen2.end(), 0);
        for (long long j = 0; j < P; j++) {
            const int f1 = b->frame1[r * P + j], f2 = b->frame2[r * P + j];
            if (f1 < 0) continue;
            ORB_CHECK_ARG(!seen1[f1] && !seen2[f2], "a round names a keyframe twice");
            seen1[f1] = 1;
            seen2[f2] = 1;
        }
        if (same)
            for (int f = 0; f < std::min(b->n_frames1, b->n_frames2); f++)
                ORB_CHECK_ARG(!(seen1[f] && seen2[f]), "a round names a keyframe as keyframe 1 and as keyframe 2");
    }
    orblm_batch d = *b;
    orbm_tri_batch s = *search;
    orblm_pairs q = *pairs;
    orblm_points o = *out;
    int32_t *dm = match12, *dn = nmatches;
    Mirror m;
    lm_mirror_batch(m, d, n);
    lm_mirror_pairs(m, q, n, false);
    lm_mirror_points(m, o, d, n);
    m.add(s.desc1, (size_t)b->n_frames1 * b->cap1 * 32, true, false);
    m.add(s.desc2, (size_t)b->n_frames2 * b->cap2 * 32, true, false);
    m.add(dm, (size_t)n * b->cap1, true, true);
    m.add(dn, n, true, true);
    m.add(o.has_mappoint1, (size_t)b->n_frames1 * b->cap1, true, true);
    m.add(o.has_mappoint2, (size_t)b->n_frames2 * b->cap2, true, true, true);   // one array when they are the same
    return run_host(g_lm, device, m, [&] { return orblm_create_new_map_points_device(&d, &s, n_rounds, &q, &o, dm, dn, nullptr); });
}
