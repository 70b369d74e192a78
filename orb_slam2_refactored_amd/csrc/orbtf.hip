// orbtf.hip — Tracking's per-frame state on gfx950: frame.mappoints, frame.outlier and the pose between the searches,
// the local map and PoseOptimization, batched over frames (include/orbslam2_amd.h, "Tracking's per-frame state").
//
// Reference: src/Tracking.cc:187-282 (DiscardOutliers, TrackWithMotionModel, TrackReferenceKeyFrame), :490-511, :664-680,
// :685-786, :808-814, :980-997, :1259-1313; src/Optimizer.cc:355-415; src/ORBmatcher.cc:1283-1313; src/KeyFrame.cc:198-220.
// The per-element arithmetic is csrc/tf_frame.h's.
//
// Kernels and what bounds them (cap = kp_cap <= 8192, n = frame_n clamped to [0, cap]):
//   tf_apply_kernel        one thread per (f, i < n): a gather through kp_match
//   tf_edge_count_kernel   one workgroup per f: the keypoints with a map point; pose and camera widened
//   tf_edge_emit_kernel    one workgroup per f: its offset = the counts before it, an ordered compaction by ballot /
//                          popcount prefix (the order is the reference's: no atomics)
//   tf_finish_kernel       one workgroup per f: scatter of the edge flags, the narrowed pose, then the ordered pass
//   tf_motion_kernel       one thread per (f, i < max(cur cap, last cap)); every thread forms the 12-float pose product
//   tf_end_kernel          one workgroup per f: one pass over the keypoints, one over the reference keyframe's row
//   tf_drop_kernel         one thread per (f, i < n)
//   tf_stereo_kernel       one workgroup of 1024 per f: the depth words in LDS (4 * cap bytes + cap flag bytes), two
//                          counting passes of n reads per thread (rank, then position among the created)
#include <algorithm>

#include "common.h"
#include "tf_frame.h"

namespace orbamd {

__device__ __forceinline__ int tf_n(const orbtf_frames& fr, int f) { return min(max(fr.frame_n[f], 0), fr.kp_cap); }

// sum over a workgroup of 256 (s: 4 ints); every thread gets it
__device__ __forceinline__ int tf_block_sum(int c, int* s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    return (s[0] + s[1]) + (s[2] + s[3]);
}

// The position of a taken element among those taken by the workgroup of 256 in this step, and the step's total.
__device__ __forceinline__ int tf_block_rank(bool take, int* s_wave, int& total) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long b = __ballot(take);
    __syncthreads();
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int off = 0;
    for (int t = 0; t < wave; t++) off += s_wave[t];
    total = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
    return off + __popcll(b & ((1ull << lane) - 1));
}

__global__ __launch_bounds__(256) void tf_apply_kernel(orbtf_frames fr, int mode, const int32_t* kp_match, const int32_t* src,
                                                       int n_rows, int src_cap, const int32_t* src_row, int M) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= tf_n(fr, f)) return;
    const size_t at = (size_t)f * fr.kp_cap + i;
    const int row = src_row ? src_row[f] : f, m = kp_match[at];
    if (!tf_slot_ok(row, n_rows) || !tf_slot_ok(m, src_cap)) {
        if (mode == ORBTF_REPLACE) fr.frame_mappoint[at] = -1;
        return;
    }
    const int p = src[(size_t)row * src_cap + m];
    fr.frame_mappoint[at] = tf_slot_ok(p, M) ? p : -1;
}

__global__ __launch_bounds__(256) void tf_edge_count_kernel(orbtf_frames fr, int M, orbtf_edges o, int32_t* cnt) {
    __shared__ int s[4];
    const int f = blockIdx.x, n = tf_n(fr, f), t = threadIdx.x;
    int c = 0;
    for (int i = t; i < n; i += 256) c += tf_slot_ok(fr.frame_mappoint[(size_t)f * fr.kp_cap + i], M) ? 1 : 0;
    c = tf_block_sum(c, s);
    if (t == 0) cnt[f] = c;
    if (t < 9) o.pose_R[9 * (size_t)f + t] = (double)fr.pose[12 * (size_t)f + t];
    if (t < 3) o.pose_t[3 * (size_t)f + t] = (double)fr.pose[12 * (size_t)f + 9 + t];
    if (t < 5) o.cam[5 * (size_t)f + t] = (double)fr.camera[5 * (size_t)f + t];
}

__global__ __launch_bounds__(256) void tf_edge_emit_kernel(orbtf_frames fr, orbtf_map m, const float* inv_sigma2, int n_levels,
                                                           orbtf_edges o, const int32_t* cnt) {
    __shared__ int s_before, s_wave[4];
    const int f = blockIdx.x, n = tf_n(fr, f), F = fr.n_frames;
    if (threadIdx.x < 64) {   // the counts before this frame, and the batch's total
        int before = 0, total = 0;
        for (int q = threadIdx.x; q < F; q += 64) {
            const int c = cnt[q];
            total += c;
            if (q < f) before += c;
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) {
            before += __shfl_xor(before, s, 64);
            total += __shfl_xor(total, s, 64);
        }
        if (threadIdx.x == 0) {
            s_before = before;
            o.edge_begin[f] = before;
            if (f == F - 1) o.edge_begin[F] = total;
        }
    }
    __syncthreads();
    int pos = s_before;
    const size_t rows = (size_t)F * fr.kp_cap;
    for (int base = 0; base < n; base += 256) {   // uniform trip count
        const int i = base + (int)threadIdx.x;
        const size_t at = (size_t)f * fr.kp_cap + i;
        const int p = i < n ? fr.frame_mappoint[at] : -1;
        const bool ok = tf_slot_ok(p, m.n_mappoints);
        int step;
        const size_t e = (size_t)pos + tf_block_rank(ok, s_wave, step);
        if (ok && e < rows) {   // e < the batch's total <= rows
            fr.frame_outlier[at] = 0;   // :371
            const int oct = min(max(fr.kp_octave[at], 0), n_levels - 1);
#pragma unroll
            for (int k = 0; k < 3; k++) o.xw[3 * e + k] = (double)m.mp_xw[3 * (size_t)p + k];
            o.obs[3 * e] = (double)fr.kp_xy[2 * at];
            o.obs[3 * e + 1] = (double)fr.kp_xy[2 * at + 1];
            o.obs[3 * e + 2] = (double)fr.kp_uright[at];
            o.inv_sigma2[e] = (double)inv_sigma2[oct];
            o.edge_kp[e] = i;
        }
        pos += step;
    }
}

__global__ __launch_bounds__(256) void tf_finish_kernel(orbtf_frames fr, orbtf_map m, int mode, orbtf_edges ed, orbba_pose_result res,
                                                        int localization, int stereo, int32_t* n_inliers, int32_t* discarded,
                                                        int32_t* n_discarded) {
    __shared__ int s[4], s_wave[4];
    const int f = blockIdx.x, n = tf_n(fr, f), t = threadIdx.x;
    const long long rows = (long long)fr.n_frames * fr.kp_cap;
    const long long e0 = min(max((long long)ed.edge_begin[f], 0LL), rows), e1 = min(max((long long)ed.edge_begin[f + 1], e0), rows);
    if (e1 - e0 >= 3) {   // :413-415
        for (long long e = e0 + t; e < e1; e += 256) {
            const int k = ed.edge_kp[e];
            if (tf_slot_ok(k, n)) fr.frame_outlier[(size_t)f * fr.kp_cap + k] = res.outlier[e] ? 1 : 0;
        }
        if (t < 9) fr.pose[12 * (size_t)f + t] = (float)res.pose_R[9 * (size_t)f + t];   // FromSE3Quat: one rounding
        if (t < 3) fr.pose[12 * (size_t)f + 9 + t] = (float)res.pose_t[3 * (size_t)f + t];
    }
    __syncthreads();   // the flags are read back by other threads of this workgroup
    int c = 0, n_disc = 0;
    for (int base = 0; base < n; base += 256) {   // uniform trip count
        const int i = base + t;
        const size_t at = (size_t)f * fr.kp_cap + i;
        const int p = i < n ? fr.frame_mappoint[at] : -1;
        const bool ok = tf_slot_ok(p, m.n_mappoints);
        const bool out = ok && fr.frame_outlier[at];
        if (mode == ORBTF_DISCARD) {
            int step;
            const int j = n_disc + tf_block_rank(out, s_wave, step);
            if (out) {
                fr.frame_mappoint[at] = -1;
                fr.frame_outlier[at] = 0;
                discarded[(size_t)f * fr.kp_cap + j] = p;   // j < n
            } else if (ok && m.mp_nobs[p] > 0) {
                c++;
            }
            n_disc += step;
        } else if (ok) {
            if (!out) {
                atomicAdd(&m.mp_found[p], 1);   // IncreaseFound
                if (localization || m.mp_nobs[p] > 0) c++;
            } else if (stereo) {
                fr.frame_mappoint[at] = -1;
            }
        }
    }
    c = tf_block_sum(c, s);
    if (t == 0) {
        n_inliers[f] = c;
        if (mode == ORBTF_DISCARD) n_discarded[f] = n_disc;
    }
}

__global__ __launch_bounds__(256) void tf_motion_kernel(orbtf_frames cur, orbtf_frames last, orbtf_map m, const float* velocity,
                                                        const float* baseline, int monocular, orbtf_motion o) {
    const int f = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
    const float* L = last.pose + 12 * (size_t)f;
    float Cp[12];
    tf_pose_product(velocity + 12 * (size_t)f, L, Cp);   // currFrame.SetPose(CameraPose(velocity) * lastFrame.pose)
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 12; k++) cur.pose[12 * (size_t)f + k] = Cp[k];
        o.motion[f] = tf_motion(L, Cp, baseline[f], monocular != 0);
    }
    if (blockIdx.x == 0 && f == 0)
        for (int q = threadIdx.x; q <= cur.n_frames; q += 256) {
            o.kp_begin[q] = q * cur.kp_cap;
            o.mp_begin[q] = q * last.kp_cap;
        }
    if (t < cur.kp_cap) {
        const size_t at = (size_t)f * cur.kp_cap + t;
        const bool live = t < tf_n(cur, f);
        if (live) cur.frame_mappoint[at] = -1;   // std::fill (:232)
        o.kp_claimed[at] = live ? 0 : 1;         // the padding is never matched
    }
    if (t >= last.kp_cap) return;
    const size_t at = (size_t)f * last.kp_cap + t;
    TfProj r{0, 0.f, 0.f, 0.f};
    int oct = 0;
    float ang = 0.f;
    uint8_t has_obs = 0;
    uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
    if (t < tf_n(last, f)) {
        int p = last.frame_mappoint[at];
        if (tf_slot_ok(p, m.n_mappoints)) {
            const int rp = m.mp_replaced[p];   // GetReplaced(): one step (:808-814)
            if (tf_slot_ok(rp, m.n_mappoints)) last.frame_mappoint[at] = p = rp;
        }
        oct = last.kp_octave[at];
        ang = last.kp_angle[at];
        if (tf_slot_ok(p, m.n_mappoints)) {
            has_obs = m.mp_nobs[p] > 0 ? 1 : 0;
            d0 = reinterpret_cast<const uint4*>(m.mp_desc)[2 * (size_t)p];
            d1 = reinterpret_cast<const uint4*>(m.mp_desc)[2 * (size_t)p + 1];
            if (!last.frame_outlier[at]) r = tf_project(Cp, cur.camera + 5 * (size_t)f, cur.bounds + 4 * (size_t)f, m.mp_xw + 3 * (size_t)p);
        }
    }
    o.mp_valid[at] = (uint8_t)r.valid;
    o.mp_proj[3 * at] = r.u;
    o.mp_proj[3 * at + 1] = r.v;
    o.mp_proj[3 * at + 2] = r.ur;
    o.mp_octave[at] = oct;
    o.mp_angle[at] = ang;
    o.mp_has_obs[at] = has_obs;
    reinterpret_cast<uint4*>(o.mp_desc)[2 * at] = d0;
    reinterpret_cast<uint4*>(o.mp_desc)[2 * at + 1] = d1;
}

__global__ __launch_bounds__(256) void tf_end_kernel(orbtf_frames fr, orbtf_map m, float th_depth, const int32_t* reference_kf,
                                                     const int32_t* min_obs, int32_t* n_observations, int32_t* counts) {
    __shared__ int s[4];
    const int f = blockIdx.x, n = tf_n(fr, f), t = threadIdx.x;
    int c0 = 0, c1 = 0, c2 = 0;
    for (int i = t; i < fr.kp_cap; i += 256) {
        const size_t at = (size_t)f * fr.kp_cap + i;
        if (i >= n) {
            n_observations[at] = -1;
            continue;
        }
        const int p = fr.frame_mappoint[at];
        bool ok = tf_slot_ok(p, m.n_mappoints), out = fr.frame_outlier[at] != 0;
        const int nobs = ok ? m.mp_nobs[p] : 0;
        n_observations[at] = ok && !out ? nobs : -1;   // :1259-1264, before the clean
        if (ok && nobs < 1) {                          // :1273-1281
            fr.frame_outlier[at] = 0;
            fr.frame_mappoint[at] = -1;
            ok = out = false;
        }
        if (fr.kp_depth) {   // :502-510
            const uint32_t z = tf_bits(fr.kp_depth[at]);
            if (tf_depth_valid(z) && tf_depth_near(z, th_depth)) (ok && !out ? c0 : c1)++;
        }
    }
    const int k = reference_kf[f], mo = min_obs[f];
    if (tf_slot_ok(k, m.n_keyframes)) {   // KeyFrame::TrackedMapPoints
        const int nk = min(max(m.kf_n[k], 0), m.kf_cap);
        for (int i = t; i < nk; i += 256) {
            const int p = m.kf_mappoint[(size_t)k * m.kf_cap + i];
            if (tf_slot_ok(p, m.n_mappoints) && !m.mp_bad[p] && (mo <= 0 || m.mp_nobs[p] >= mo)) c2++;
        }
    }
    c0 = tf_block_sum(c0, s);
    c1 = tf_block_sum(c1, s);
    c2 = tf_block_sum(c2, s);
    if (t == 0) {
        counts[3 * (size_t)f] = c0;
        counts[3 * (size_t)f + 1] = c1;
        counts[3 * (size_t)f + 2] = c2;
    }
}

__global__ __launch_bounds__(256) void tf_drop_kernel(orbtf_frames fr) {
    const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= tf_n(fr, f)) return;
    const size_t at = (size_t)f * fr.kp_cap + i;
    if (fr.frame_outlier[at]) fr.frame_mappoint[at] = -1;
}

constexpr int TF_ST_THREADS = 1024;
constexpr int TF_ST_OWN = ORBM_PROJ_MAX_KP / TF_ST_THREADS;   // keypoints a thread owns: i = t + k * 1024

// sum over the workgroup of 1024 (s: 16 ints)
__device__ __forceinline__ int tf_sum1024(int c, int* s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = c;
    __syncthreads();
    int total = 0;
#pragma unroll
    for (int w = 0; w < TF_ST_THREADS / 64; w++) total += s[w];
    return total;
}

// Dynamic LDS: the depth words of cap4 = kp_cap rounded up to 4 keypoints, then cap4 flag bytes.
__global__ __launch_bounds__(TF_ST_THREADS) void tf_stereo_kernel(orbtf_frames fr, orbtf_map m, int mode, float th_depth,
                                                                  orbtf_created o) {
    extern __shared__ uint4 s_dyn[];
    __shared__ int s[TF_ST_THREADS / 64];
    const int f = blockIdx.x, n = tf_n(fr, f), t = threadIdx.x;
    const int cap4 = (fr.kp_cap + 3) & ~3, n4 = (n + 3) & ~3;
    uint32_t* s_w = reinterpret_cast<uint32_t*>(s_dyn);
    uint8_t* s_flag = reinterpret_cast<uint8_t*>(s_w + cap4);
    const bool by_index = mode == ORBTF_INIT;
    uint32_t w[TF_ST_OWN], zb[TF_ST_OWN];
    int rank[TF_ST_OWN];
    int n_valid = 0, n_close = 0;
#pragma unroll
    for (int k = 0; k < TF_ST_OWN; k++) {
        const int i = t + k * TF_ST_THREADS;
        zb[k] = i < n ? tf_bits(fr.kp_depth[(size_t)f * fr.kp_cap + i]) : 0u;
        w[k] = tf_depth_word(zb[k], by_index);
        rank[k] = 0;
        if (i < n4) s_w[i] = w[k];
        if (w[k] != TF_WORD_NONE) {
            n_valid++;
            if (!tf_depth_far(zb[k], th_depth)) n_close++;
        }
    }
    n_valid = tf_sum1024(n_valid, s);
    n_close = tf_sum1024(n_close, s);   // (its barriers also publish s_w)
    for (int j = 0; j < n4; j += 4) {   // rank = the pairs before this one
        const uint4 q = *reinterpret_cast<const uint4*>(s_w + j);
#pragma unroll
        for (int k = 0; k < TF_ST_OWN; k++) {
            if (k * TF_ST_THREADS >= n) break;   // nobody's k-th keypoint is below n (uniform)
            const int i = t + k * TF_ST_THREADS;
            rank[k] += (tf_depth_before(q.x, j, w[k], i) ? 1 : 0) + (tf_depth_before(q.y, j + 1, w[k], i) ? 1 : 0) +
                       (tf_depth_before(q.z, j + 2, w[k], i) ? 1 : 0) + (tf_depth_before(q.w, j + 3, w[k], i) ? 1 : 0);
        }
    }
    const int n_proc = by_index ? n_valid : tf_n_processed(n_valid, n_close);
    bool create[TF_ST_OWN];
    int n_created = 0;
#pragma unroll
    for (int k = 0; k < TF_ST_OWN; k++) {
        const int i = t + k * TF_ST_THREADS;
        create[k] = false;
        if (w[k] != TF_WORD_NONE && rank[k] < n_proc) {
            const size_t at = (size_t)f * fr.kp_cap + i;
            const int p = fr.frame_mappoint[at];
            if (by_index || !tf_slot_ok(p, m.n_mappoints)) {
                create[k] = true;
            } else if (m.mp_nobs[p] < 1) {
                create[k] = true;
                if (mode == ORBTF_KEYFRAME) fr.frame_mappoint[at] = -1;   // :721
            }
        }
        if (i < n4) s_flag[i] = create[k] ? 1 : 0;
        n_created += create[k] ? 1 : 0;
    }
    n_created = tf_sum1024(n_created, s);   // (publishes s_flag)
    int pos[TF_ST_OWN];
#pragma unroll
    for (int k = 0; k < TF_ST_OWN; k++) pos[k] = 0;
    for (int j = 0; j < n4; j += 4) {   // position = the created pairs before this one
        const uint4 q = *reinterpret_cast<const uint4*>(s_w + j);
        const uint32_t fl = *reinterpret_cast<const uint32_t*>(s_flag + j);
        if (!fl) continue;
#pragma unroll
        for (int k = 0; k < TF_ST_OWN; k++) {
            if (k * TF_ST_THREADS >= n) break;
            const int i = t + k * TF_ST_THREADS;
            pos[k] += ((fl & 0xffu) && tf_depth_before(q.x, j, w[k], i) ? 1 : 0) +
                      ((fl & 0xff00u) && tf_depth_before(q.y, j + 1, w[k], i) ? 1 : 0) +
                      ((fl & 0xff0000u) && tf_depth_before(q.z, j + 2, w[k], i) ? 1 : 0) +
                      ((fl & 0xff000000u) && tf_depth_before(q.w, j + 3, w[k], i) ? 1 : 0);
        }
    }
#pragma unroll
    for (int k = 0; k < TF_ST_OWN; k++) {
        if (!create[k]) continue;
        const int i = t + k * TF_ST_THREADS;
        const size_t at = (size_t)f * fr.kp_cap + i, to = (size_t)f * fr.kp_cap + pos[k];   // pos < n_created <= n
        float X[3];
        float Z;
        memcpy(&Z, &zb[k], 4);
        tf_unproject(fr.pose + 12 * (size_t)f, fr.camera + 5 * (size_t)f, fr.kp_xy[2 * at], fr.kp_xy[2 * at + 1], Z,
                     mode == ORBTF_VO, X);
        o.created_kp[to] = i;
        o.created_xw[3 * to] = X[0];
        o.created_xw[3 * to + 1] = X[1];
        o.created_xw[3 * to + 2] = X[2];
    }
    if (t == 0) {
        o.n_created[f] = n_created;
        o.n_processed[f] = n_proc;
    }
}

}  // namespace orbamd

using namespace orbamd;

namespace {

thread_local Scratch g_tf;

int tf_check_frames(const orbtf_frames* fr) {
    ORB_CHECK_ARG(fr, "null frames");
    ORB_CHECK_ARG(fr->n_frames >= 0, "negative n_frames");
    ORB_CHECK_ARG(fr->n_frames < 65536, "65536 frames or more in one call");
    ORB_CHECK_ARG(fr->kp_cap >= 1 && fr->kp_cap <= ORBM_PROJ_MAX_KP, "kp_cap must be in [1, ORBM_PROJ_MAX_KP]");
    ORB_CHECK_ARG(fr->n_frames == 0 || fr->frame_n, "null frame_n");
    return ORB_OK;
}

int tf_check_map(const orbtf_map* m) {
    ORB_CHECK_ARG(m, "null map");
    ORB_CHECK_ARG(m->n_mappoints >= 0 && m->n_keyframes >= 0, "negative sizes");
    return ORB_OK;
}

// frame_n, and the map-point slots when they are given
int tf_host_frames(const orbtf_frames* fr, int M) {
    for (int f = 0; f < fr->n_frames; f++)
        ORB_CHECK_ARG(fr->frame_n[f] >= 0 && fr->frame_n[f] <= fr->kp_cap, "frame_n outside [0, kp_cap]");
    if (M < 0 || !fr->frame_mappoint) return ORB_OK;
    return check_range(fr->frame_mappoint, (size_t)fr->n_frames * fr->kp_cap, -1, M, "frame_mappoint entry outside [-1, n_mappoints)");
}

dim3 tf_grid(const orbtf_frames& fr, int per_frame) { return dim3((per_frame + 255) / 256, fr.n_frames); }

}  // namespace

// ---- 1 apply_matches
static int tf_apply_check(const orbtf_frames* fr, int32_t mode, const int32_t* kp_match, const int32_t* src, int32_t n_rows,
                          int32_t src_cap, int32_t n_mappoints) {
    int rc;
    if ((rc = tf_check_frames(fr))) return rc;
    ORB_CHECK_ARG(mode == ORBTF_MERGE || mode == ORBTF_REPLACE, "unknown mode");
    ORB_CHECK_ARG(n_rows >= 0 && n_mappoints >= 0, "negative sizes");
    ORB_CHECK_ARG(src_cap >= 1, "src_cap must be at least 1");
    if (fr->n_frames == 0) return ORB_OK;
    ORB_CHECK_ARG(fr->frame_mappoint && kp_match && src, "null frame_mappoint, kp_match or src");
    return ORB_OK;
}

extern "C" int orbtf_apply_matches_device(const orbtf_frames* fr, int32_t mode, const int32_t* kp_match, const int32_t* src,
                                          int32_t n_rows, int32_t src_cap, const int32_t* src_row, int32_t n_mappoints,
                                          void* stream) {
    int rc;
    if ((rc = tf_apply_check(fr, mode, kp_match, src, n_rows, src_cap, n_mappoints))) return rc;
    if (fr->n_frames == 0) return ORB_OK;
    hipLaunchKernelGGL(tf_apply_kernel, tf_grid(*fr, fr->kp_cap), dim3(256), 0, (hipStream_t)stream, *fr, mode, kp_match, src,
                       n_rows, src_cap, src_row, n_mappoints);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbtf_apply_matches(const orbtf_frames* fr, int32_t mode, const int32_t* kp_match, const int32_t* src,
                                   int32_t n_rows, int32_t src_cap, const int32_t* src_row, int32_t n_mappoints, int device) {
    int rc;
    if ((rc = tf_apply_check(fr, mode, kp_match, src, n_rows, src_cap, n_mappoints))) return rc;
    if (fr->n_frames == 0) return ORB_OK;
    const size_t F = fr->n_frames, pc = fr->kp_cap;
    if ((rc = tf_host_frames(fr, n_mappoints))) return rc;
    if ((rc = check_range(kp_match, F * pc, -1, src_cap, "kp_match entry outside [-1, src_cap)"))) return rc;
    if ((rc = check_range(src, (size_t)n_rows * src_cap, -1, n_mappoints, "src entry outside [-1, n_mappoints)"))) return rc;
    if (src_row) {
        if ((rc = check_range(src_row, F, 0, n_rows, "src_row outside [0, n_rows)"))) return rc;
    } else {
        ORB_CHECK_ARG(n_rows >= fr->n_frames, "src has fewer rows than frames and no src_row");
    }
    orbtf_frames d = *fr;
    Mirror io;
    io.add(d.frame_n, F, true, false); io.add(d.frame_mappoint, F * pc, true, true);
    io.add(kp_match, F * pc, true, false); io.add(src, (size_t)n_rows * src_cap, true, false); io.add(src_row, F, true, false);
    return run_host(g_tf, device, io, [&] {
        return orbtf_apply_matches_device(&d, mode, kp_match, src, n_rows, src_cap, src_row, n_mappoints, nullptr);
    });
}

// ---- 2 pose_edges
static int tf_edges_check(const orbtf_frames* fr, const orbtf_map* m, const float* table, int32_t n_levels, const orbtf_edges* o) {
    int rc;
    if ((rc = tf_check_frames(fr)) || (rc = tf_check_map(m))) return rc;
    ORB_CHECK_ARG(o, "null edges");
    ORB_CHECK_ARG(n_levels >= 1 && n_levels <= ORBTF_MAX_LEVELS, "n_levels must be in [1, ORBTF_MAX_LEVELS]");
    if (fr->n_frames == 0) return ORB_OK;
    ORB_CHECK_ARG(fr->frame_mappoint && fr->frame_outlier && fr->pose && fr->camera && fr->kp_xy && fr->kp_octave && fr->kp_uright,
                  "null frame array");
    ORB_CHECK_ARG(m->n_mappoints == 0 || m->mp_xw, "null mp_xw");
    ORB_CHECK_ARG(table, "null inv_sigma2_table");
    ORB_CHECK_ARG(o->edge_begin && o->pose_R && o->pose_t && o->cam && o->xw && o->obs && o->inv_sigma2 && o->edge_kp,
                  "null edge array");
    return ORB_OK;
}

extern "C" int orbtf_pose_edges_device(const orbtf_frames* fr, const orbtf_map* map, const float* inv_sigma2_table,
                                       int32_t n_levels, const orbtf_edges* out, void* stream) {
    int rc;
    if ((rc = tf_edges_check(fr, map, inv_sigma2_table, n_levels, out))) return rc;
    if (fr->n_frames == 0) return ORB_OK;
    if ((rc = g_tf.use_current_device())) return rc;
    if ((rc = g_tf.ws.reserve((size_t)fr->n_frames * sizeof(int32_t)))) return rc;
    int32_t* cnt = g_tf.ws.as<int32_t>();
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(tf_edge_count_kernel, dim3(fr->n_frames), dim3(256), 0, st, *fr, map->n_mappoints, *out, cnt);
    hipLaunchKernelGGL(tf_edge_emit_kernel, dim3(fr->n_frames), dim3(256), 0, st, *fr, *map, inv_sigma2_table, n_levels, *out, cnt);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbtf_pose_edges(const orbtf_frames* fr, const orbtf_map* map, const float* inv_sigma2_table, int32_t n_levels,
                                const orbtf_edges* out, int device) {
    int rc;
    if ((rc = tf_edges_check(fr, map, inv_sigma2_table, n_levels, out))) return rc;
    if (fr->n_frames == 0) return ORB_OK;
    if ((rc = tf_host_frames(fr, map->n_mappoints))) return rc;
    const size_t F = fr->n_frames, pc = fr->kp_cap, M = map->n_mappoints;
    for (size_t f = 0; f < F; f++)
        if ((rc = check_range(fr->kp_octave + f * pc, fr->frame_n[f], 0, n_levels, "kp_octave outside [0, n_levels)"))) return rc;
    orbtf_frames d = *fr;
    orbtf_map dm = *map;
    orbtf_edges de = *out;
    Mirror io;
    io.add(d.frame_n, F, true, false); io.add(d.frame_mappoint, F * pc, true, false); io.add(d.frame_outlier, F * pc, true, true);
    io.add(d.pose, F * 12, true, false); io.add(d.camera, F * 5, true, false); io.add(d.kp_xy, F * pc * 2, true, false);
    io.add(d.kp_octave, F * pc, true, false); io.add(d.kp_uright, F * pc, true, false); io.add(dm.mp_xw, M * 3, true, false);
    io.add(inv_sigma2_table, (size_t)n_levels, true, false);
    io.add(de.edge_begin, F + 1, false, true); io.add(de.pose_R, F * 9, false, true); io.add(de.pose_t, F * 3, false, true);
    io.add(de.cam, F * 5, false, true); // (the rows past the last edge go up too, so that they come back as the caller left them)
    io.add(de.xw, F * pc * 3, true, true); io.add(de.obs, F * pc * 3, true, true);
    io.add(de.inv_sigma2, F * pc, true, true); io.add(de.edge_kp, F * pc, true, true);
    return run_host(g_tf, device, io, [&] { return orbtf_pose_edges_device(&d, &dm, inv_sigma2_table, n_levels, &de, nullptr); });
}

// ---- 3 finish_pose
static int tf_finish_check(const orbtf_frames* fr, const orbtf_map* m, int32_t mode, const orbtf_edges* e,
                           const orbba_pose_result* r, const int32_t* n_inliers, const int32_t* discarded,
                           const int32_t* n_discarded) {
    int rc;
    if ((rc = tf_check_frames(fr)) || (rc = tf_check_map(m))) return rc;
    ORB_CHECK_ARG(mode == ORBTF_DISCARD || mode == ORBTF_LOCAL_MAP, "unknown mode");
    ORB_CHECK_ARG(e && r, "null edges or result");
    if (fr->n_frames == 0) return ORB_OK;
    ORB_CHECK_ARG(fr->frame_mappoint && fr->frame_outlier && fr->pose, "null frame array");
    ORB_CHECK_ARG(m->n_mappoints == 0 || (m->mp_nobs && (mode == ORBTF_DISCARD || m->mp_found)), "null mp_nobs or mp_found");
    ORB_CHECK_ARG(e->edge_begin && e->edge_kp && r->pose_R && r->pose_t && r->outlier && n_inliers, "null edge or result array");
    ORB_CHECK_ARG(mode != ORBTF_DISCARD || (discarded && n_discarded), "null discarded or n_discarded");
    return ORB_OK;
}

extern "C" int orbtf_finish_pose_device(const orbtf_frames* fr, const orbtf_map* map, int32_t mode, const orbtf_edges* edges,
                                        const orbba_pose_result* result, int32_t localization, int32_t stereo,
                                        int32_t* n_inliers, int32_t* discarded, int32_t* n_discarded, void* stream) {
    int rc;
    if ((rc = tf_finish_check(fr, map, mode, edges, result, n_inliers, discarded, n_discarded))) return rc;
    if (fr->n_frames == 0) return ORB_OK;
    hipLaunchKernelGGL(tf_finish_kernel, dim3(fr->n_frames), dim3(256), 0, (hipStream_t)stream, *fr, *map, mode, *edges, *result,
                       localization, stereo, n_inliers, discarded, n_discarded);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbtf_finish_pose(const orbtf_frames* fr, const orbtf_map* map, int32_t mode, const orbtf_edges* edges,
                                 const orbba_pose_result* result, int32_t localization, int32_t stereo, int32_t* n_inliers,
                                 int32_t* discarded, int32_t* n_discarded, int device) {
    int rc;
    if ((rc = tf_finish_check(fr, map, mode, edges, result, n_inliers, discarded, n_discarded))) return rc;
    if (fr->n_frames == 0) return ORB_OK;
    if ((rc = tf_host_frames(fr, map->n_mappoints))) return rc;
    const size_t F = fr->n_frames, pc = fr->kp_cap, M = map->n_mappoints;
    if ((rc = check_csr(edges->edge_begin, (int)F, (int)(F * pc), "edge_begin"))) return rc;
    const size_t E = edges->edge_begin[F];
    if ((rc = check_range(edges->edge_kp, E, 0, fr->kp_cap, "edge_kp outside [0, kp_cap)"))) return rc;
    orbtf_frames d = *fr;
    orbtf_map dm = *map;
    orbtf_edges de = *edges;
    orbba_pose_result dr = *result;
    Mirror io;
    io.add(d.frame_n, F, true, false); io.add(d.frame_mappoint, F * pc, true, true); io.add(d.frame_outlier, F * pc, true, true);
    io.add(d.pose, F * 12, true, true); io.add(dm.mp_nobs, M, true, false);
    if (mode == ORBTF_LOCAL_MAP) io.add(dm.mp_found, M, true, true);
    io.add(de.edge_begin, F + 1, true, false); io.add(de.edge_kp, E, true, false); io.add(dr.pose_R, F * 9, true, false);
    io.add(dr.pose_t, F * 3, true, false); io.add(dr.outlier, E, true, false); io.add(n_inliers, F, false, true);
    if (mode == ORBTF_DISCARD) { io.add(discarded, F * pc, true, true); io.add(n_discarded, F, false, true); }
    return run_host(g_tf, device, io, [&] {
        return orbtf_finish_pose_device(&d, &dm, mode, &de, &dr, localization, stereo, n_inliers, discarded, n_discarded, nullptr);
    });
}

// ---- 4 motion_project
static int tf_motion_check(const orbtf_frames* cur, const orbtf_frames* last, const orbtf_map* m, const float* velocity,
                           const float* baseline, const orbtf_motion* o) {
    int rc;
    if ((rc = tf_check_frames(cur)) || (rc = tf_check_frames(last)) || (rc = tf_check_map(m))) return rc;
    ORB_CHECK_ARG(cur->n_frames == last->n_frames, "the current and the last frames differ in n_frames");
    ORB_CHECK_ARG(o, "null motion output");
    if (cur->n_frames == 0) return ORB_OK;
    ORB_CHECK_ARG(cur->frame_mappoint && cur->pose && cur->camera && cur->bounds, "null array of the current frames");
    ORB_CHECK_ARG(last->frame_mappoint && last->frame_outlier && last->pose && last->kp_octave && last->kp_angle,
                  "null array of the last frames");
    ORB_CHECK_ARG(m->n_mappoints == 0 || (m->mp_xw && m->mp_nobs && m->mp_replaced && m->mp_desc), "null map-point table");
    ORB_CHECK_ARG(velocity && baseline, "null velocity or baseline");
    ORB_CHECK_ARG(o->motion && o->kp_begin && o->mp_begin && o->kp_claimed && o->mp_valid && o->mp_proj && o->mp_octave &&
                      o->mp_desc && o->mp_has_obs && o->mp_angle,
                  "null output array");
    return ORB_OK;
}

extern "C" int orbtf_motion_project_device(const orbtf_frames* cur, const orbtf_frames* last, const orbtf_map* map,
                                           const float* velocity, const float* baseline, int32_t monocular,
                                           const orbtf_motion* out, void* stream) {
    int rc;
    if ((rc = tf_motion_check(cur, last, map, velocity, baseline, out))) return rc;
    if (cur->n_frames == 0) return ORB_OK;
    ORB_CHECK_ARG(((uintptr_t)map->mp_desc | (uintptr_t)out->mp_desc) % 16 == 0, "mp_desc arrays must be 16-byte aligned");
    hipLaunchKernelGGL(tf_motion_kernel, tf_grid(*cur, std::max(cur->kp_cap, last->kp_cap)), dim3(256), 0, (hipStream_t)stream,
                       *cur, *last, *map, velocity, baseline, monocular, *out);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbtf_motion_project(const orbtf_frames* cur, const orbtf_frames* last, const orbtf_map* map,
                                    const float* velocity, const float* baseline, int32_t monocular, const orbtf_motion* out,
                                    int device) {
    int rc;
    if ((rc = tf_motion_check(cur, last, map, velocity, baseline, out))) return rc;
    if (cur->n_frames == 0) return ORB_OK;
    const size_t F = cur->n_frames, pc = cur->kp_cap, lc = last->kp_cap, M = map->n_mappoints;
    if ((rc = tf_host_frames(cur, -1)) || (rc = tf_host_frames(last, map->n_mappoints))) return rc;
    if ((rc = check_range(map->mp_replaced, M, -1, map->n_mappoints, "mp_replaced outside [-1, n_mappoints)"))) return rc;
    orbtf_frames dc = *cur, dl = *last;
    orbtf_map dm = *map;
    orbtf_motion dout = *out;
    Mirror io;
    io.add(dc.frame_n, F, true, false); io.add(dc.frame_mappoint, F * pc, true, true); io.add(dc.pose, F * 12, false, true);
    io.add(dc.camera, F * 5, true, false); io.add(dc.bounds, F * 4, true, false);
    io.add(dl.frame_n, F, true, false); io.add(dl.frame_mappoint, F * lc, true, true); io.add(dl.frame_outlier, F * lc, true, false);
    io.add(dl.pose, F * 12, true, false); io.add(dl.kp_octave, F * lc, true, false); io.add(dl.kp_angle, F * lc, true, false);
    io.add(dm.mp_xw, M * 3, true, false); io.add(dm.mp_nobs, M, true, false); io.add(dm.mp_replaced, M, true, false);
    io.add(dm.mp_desc, M * 32, true, false); io.add(velocity, F * 12, true, false); io.add(baseline, F, true, false);
    io.add(dout.motion, F, false, true); io.add(dout.kp_begin, F + 1, false, true); io.add(dout.mp_begin, F + 1, false, true);
    io.add(dout.kp_claimed, F * pc, false, true); io.add(dout.mp_valid, F * lc, false, true); io.add(dout.mp_proj, F * lc * 3, false, true);
    io.add(dout.mp_octave, F * lc, false, true); io.add(dout.mp_desc, F * lc * 32, false, true);
    io.add(dout.mp_has_obs, F * lc, false, true); io.add(dout.mp_angle, F * lc, false, true);
    return run_host(g_tf, device, io,
                    [&] { return orbtf_motion_project_device(&dc, &dl, &dm, velocity, baseline, monocular, &dout, nullptr); });
}

// ---- 5 end_frame
static int tf_end_check(const orbtf_frames* fr, const orbtf_map* m, const int32_t* reference_kf, const int32_t* min_obs,
                        const int32_t* n_observations, const int32_t* counts) {
    int rc;
    if ((rc = tf_check_frames(fr)) || (rc = tf_check_map(m))) return rc;
    ORB_CHECK_ARG(m->kf_cap >= 1, "kf_cap must be at least 1");
    ORB_CHECK_ARG((long long)m->n_keyframes * m->kf_cap < 0x7fffffffLL, "a table of 2^31 entries or more");
    if (fr->n_frames == 0) return ORB_OK;
    ORB_CHECK_ARG(fr->frame_mappoint && fr->frame_outlier, "null frame array");
    ORB_CHECK_ARG(m->n_mappoints == 0 || (m->mp_nobs && m->mp_bad), "null mp_nobs or mp_bad");
    ORB_CHECK_ARG(m->n_keyframes == 0 || (m->kf_n && m->kf_mappoint), "null kf_n or kf_mappoint");
    ORB_CHECK_ARG(reference_kf && min_obs && n_observations && counts, "null reference_kf, min_obs, n_observations or counts");
    return ORB_OK;
}

extern "C" int orbtf_end_frame_device(const orbtf_frames* fr, const orbtf_map* map, float th_depth, const int32_t* reference_kf,
                                      const int32_t* min_obs, int32_t* n_observations, int32_t* counts, void* stream) {
    int rc;
    if ((rc = tf_end_check(fr, map, reference_kf, min_obs, n_observations, counts))) return rc;
    if (fr->n_frames == 0) return ORB_OK;
    hipLaunchKernelGGL(tf_end_kernel, dim3(fr->n_frames), dim3(256), 0, (hipStream_t)stream, *fr, *map, th_depth, reference_kf,
                       min_obs, n_observations, counts);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbtf_end_frame(const orbtf_frames* fr, const orbtf_map* map, float th_depth, const int32_t* reference_kf,
                               const int32_t* min_obs, int32_t* n_observations, int32_t* counts, int device) {
    int rc;
    if ((rc = tf_end_check(fr, map, reference_kf, min_obs, n_observations, counts))) return rc;
    if (fr->n_frames == 0) return ORB_OK;
    if ((rc = tf_host_frames(fr, map->n_mappoints))) return rc;
    const size_t F = fr->n_frames, pc = fr->kp_cap, M = map->n_mappoints, K = map->n_keyframes, kc = map->kf_cap;
    if ((rc = check_range(reference_kf, F, -1, map->n_keyframes, "reference_kf outside [-1, n_keyframes)"))) return rc;
    for (size_t k = 0; k < K; k++) ORB_CHECK_ARG(map->kf_n[k] >= 0 && map->kf_n[k] <= map->kf_cap, "kf_n outside [0, kf_cap]");
    if ((rc = check_range(map->kf_mappoint, K * kc, -1, map->n_mappoints, "kf_mappoint entry outside [-1, n_mappoints)"))) return rc;
    orbtf_frames d = *fr;
    orbtf_map dm = *map;
    Mirror io;
    io.add(d.frame_n, F, true, false); io.add(d.frame_mappoint, F * pc, true, true); io.add(d.frame_outlier, F * pc, true, true);
    io.add(d.kp_depth, F * pc, true, false); io.add(dm.mp_nobs, M, true, false); io.add(dm.mp_bad, M, true, false);
    io.add(dm.kf_n, K, true, false); io.add(dm.kf_mappoint, K * kc, true, false);
    io.add(reference_kf, F, true, false); io.add(min_obs, F, true, false); io.add(n_observations, F * pc, false, true);
    io.add(counts, F * 3, false, true);
    return run_host(g_tf, device, io,
                    [&] { return orbtf_end_frame_device(&d, &dm, th_depth, reference_kf, min_obs, n_observations, counts, nullptr); });
}

// ---- 6 drop_outliers
static int tf_drop_check(const orbtf_frames* fr) {
    int rc;
    if ((rc = tf_check_frames(fr))) return rc;
    ORB_CHECK_ARG(fr->n_frames == 0 || (fr->frame_mappoint && fr->frame_outlier), "null frame array");
    return ORB_OK;
}

extern "C" int orbtf_drop_outliers_device(const orbtf_frames* fr, void* stream) {
    int rc;
    if ((rc = tf_drop_check(fr))) return rc;
    if (fr->n_frames == 0) return ORB_OK;
    hipLaunchKernelGGL(tf_drop_kernel, tf_grid(*fr, fr->kp_cap), dim3(256), 0, (hipStream_t)stream, *fr);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbtf_drop_outliers(const orbtf_frames* fr, int device) {
    int rc;
    if ((rc = tf_drop_check(fr))) return rc;
    if (fr->n_frames == 0) return ORB_OK;
    if ((rc = tf_host_frames(fr, -1))) return rc;
    const size_t F = fr->n_frames, pc = fr->kp_cap;
    orbtf_frames d = *fr;
    Mirror io;
    io.add(d.frame_n, F, true, false); io.add(d.frame_mappoint, F * pc, true, true); io.add(d.frame_outlier, F * pc, true, false);
    return run_host(g_tf, device, io, [&] { return orbtf_drop_outliers_device(&d, nullptr); });
}

// ---- 7 stereo_points
static int tf_stereo_check(const orbtf_frames* fr, const orbtf_map* m, int32_t mode, const orbtf_created* o) {
    int rc;
    if ((rc = tf_check_frames(fr)) || (rc = tf_check_map(m))) return rc;
    ORB_CHECK_ARG(mode == ORBTF_KEYFRAME || mode == ORBTF_VO || mode == ORBTF_INIT, "unknown mode");
    ORB_CHECK_ARG(o, "null output");
    if (fr->n_frames == 0) return ORB_OK;
    ORB_CHECK_ARG(fr->frame_mappoint && fr->pose && fr->camera && fr->kp_xy && fr->kp_depth, "null frame array");
    ORB_CHECK_ARG(m->n_mappoints == 0 || m->mp_nobs, "null mp_nobs");
    ORB_CHECK_ARG(o->created_kp && o->created_xw && o->n_created && o->n_processed, "null output array");
    return ORB_OK;
}

extern "C" int orbtf_stereo_points_device(const orbtf_frames* fr, const orbtf_map* map, int32_t mode, float th_depth,
                                          const orbtf_created* out, void* stream) {
    int rc;
    if ((rc = tf_stereo_check(fr, map, mode, out))) return rc;
    if (fr->n_frames == 0) return ORB_OK;
    const size_t cap4 = ((size_t)fr->kp_cap + 3) & ~(size_t)3;
    hipLaunchKernelGGL(tf_stereo_kernel, dim3(fr->n_frames), dim3(TF_ST_THREADS), 5 * cap4, (hipStream_t)stream, *fr, *map, mode,
                       th_depth, *out);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbtf_stereo_points(const orbtf_frames* fr, const orbtf_map* map, int32_t mode, float th_depth,
                                   const orbtf_created* out, int device) {
    int rc;
    if ((rc = tf_stereo_check(fr, map, mode, out))) return rc;
    if (fr->n_frames == 0) return ORB_OK;
    if ((rc = tf_host_frames(fr, map->n_mappoints))) return rc;
    const size_t F = fr->n_frames, pc = fr->kp_cap, M = map->n_mappoints;
    orbtf_frames d = *fr;
    orbtf_map dm = *map;
    orbtf_created dout = *out;
    Mirror io;
    io.add(d.frame_n, F, true, false); io.add(d.frame_mappoint, F * pc, true, true); io.add(d.pose, F * 12, true, false);
    io.add(d.camera, F * 5, true, false); io.add(d.kp_xy, F * pc * 2, true, false); io.add(d.kp_depth, F * pc, true, false);
    io.add(dm.mp_nobs, M, true, false);
    io.add(dout.created_kp, F * pc, true, true); io.add(dout.created_xw, F * pc * 3, true, true);
    io.add(dout.n_created, F, false, true); io.add(dout.n_processed, F, false, true);
    return run_host(g_tf, device, io, [&] { return orbtf_stereo_points_device(&d, &dm, mode, th_depth, &dout, nullptr); });
}
