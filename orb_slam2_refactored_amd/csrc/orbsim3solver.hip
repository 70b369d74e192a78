// orbsim3solver.hip — Sim3Solver::iterate (3-point RANSAC) on gfx950, batched over (keyframe 1, keyframe 2)
// pairs in orbm_sim3_batch's slot layout.
//
// src/Sim3Solver.cc:206-365.  The CPU evaluates a candidate's hypotheses one after another; they depend on
// one another only through the running maximum of the inlier counts, so the counts n[k] of a whole range of
// iterations are computed at once and the stop rule becomes a prefix maximum over them.  Three launches on
// the caller's stream:
//   s3s_prepare_kernel  one wavefront per pair: the kept slots compacted in ascending order (ballot + mbcnt,
//                       as orbsim3.hip), one 64-byte record per correspondence (Xc1, Xc2, points1, points2 in
//                       float, both thresholds in double) into the workspace, nmatches, and the range
//                       [k0, k1) of iterations this call evaluates (the cap from the host's table)
//   s3s_eval_kernel     one lane per hypothesis, one wavefront per 64 hypotheses of a pair, grid
//                       (n_pairs, ceil(min(maxk, max_iterations) / 64)): every lane draws its three
//                       correspondences and builds its own S12 / S21 in registers (sim3_hyp.h); the wave
//                       stages the pair's records into LDS a tile at a time and every lane walks the tile
//                       at a wave-uniform address (a broadcast read: no bank conflict), counting in a
//                       register: no reduction, no block barrier, no atomics
//   s3s_select_kernel   one wavefront per pair: the prefix maximum over n[k0 .. k1) seeded with the incoming
//                       max_inliers, the first success, that hypothesis rebuilt by every lane and its
//                       inlier mask with lanes over correspondences, then the outputs and the state
// Hypothesis k of pair p always uses draws[p, k, :], so a result does not depend on how the iterations were
// chunked over calls.  No fast-math: a zero or negative depth gives inf or NaN and is simply not an inlier.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "sim3_hyp.h"
#include "world_to_camera.h"

namespace orbamd {

constexpr int S3S_TILE = 128;                   // correspondences per LDS tile: 8 KiB
constexpr int S3S_MAXKP = ORBM_PROJ_MAX_KP;
constexpr int S3S_MAX_LEVELS = 32;
constexpr int S3S_CAPS = S3S_MAXKP + 1;          // the iteration cap for every nmatches in 0 .. S3S_MAXKP

// one correspondence: 12 floats and 2 doubles
struct alignas(16) S3SRec {
    float X1[3], X2[3];      // Xc1, Xc2
    float p1[2], p2[2];      // points1, points2 (FromCameraToImage)
    float pad[2];
    double thr1, thr2;       // maxErrorSq1, maxErrorSq2
};
static_assert(sizeof(S3SRec) == 64, "");

struct S3SArgs {
    int n_pairs;
    const int32_t *kp1_begin, *kp2_begin;
    const int32_t *kp1_oct, *kp2_oct;
    const float *pose1, *pose2, *cam1, *cam2;
    const uint8_t *valid1, *valid2;
    const float *xw1, *xw2;
    const int32_t* match12;
    const int32_t* draws;    // n_pairs x max_iterations x 3
    int32_t rand_max;
    int min_inliers, max_iterations, maxk;
    int n_levels;
    float sigma2[S3S_MAX_LEVELS];
    int fix_scale;
    const int32_t* caps;     // S3S_CAPS
    // outputs
    float* o_s12;
    uint8_t* o_inlier;
    int32_t* o_match12;
    int32_t *o_found, *o_ninl, *o_iter, *o_maxinl, *o_term;
    int32_t* hyp;            // n_pairs x max_iterations: the caller's hyp_inliers or the workspace
    int hyp_is_output;
    // workspace
    int32_t* slots;          // total_kp1: pair p's kept slots, compacted, at kp1_begin[p]
    S3SRec* recs;            // total_kp1: their records
    int32_t* info;           // n_pairs x 4: nmatches, k0, k1, cap
};

// writes of other lanes of this wavefront become readable
__device__ __forceinline__ void s3s_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ bool s3s_over_limit(const S3SArgs& a, int p) {
    return a.kp1_begin[p + 1] - a.kp1_begin[p] > S3S_MAXKP || a.kp2_begin[p + 1] - a.kp2_begin[p] > S3S_MAXKP;
}

__global__ __launch_bounds__(64) void s3s_prepare_kernel(S3SArgs a) {
    const int lane = threadIdx.x, p = blockIdx.x;
    const int k1b = a.kp1_begin[p], k2b = a.kp2_begin[p];
    const int n1 = a.kp1_begin[p + 1] - k1b, n2 = a.kp2_begin[p + 1] - k2b;
    int32_t* info = a.info + 4 * (size_t)p;
    if (a.hyp_is_output)
        for (int k = lane; k < a.max_iterations; k += 64) a.hyp[(size_t)p * a.max_iterations + k] = -1;
    if (s3s_over_limit(a, p)) {
        if (lane == 0) { info[0] = -1; info[1] = 0; info[2] = 0; info[3] = 0; }
        return;
    }
    const float* P1 = a.pose1 + 12 * (size_t)p;
    const float* P2 = a.pose2 + 12 * (size_t)p;
    const float* K1 = a.cam1 + 4 * (size_t)p;
    const float* K2 = a.cam2 + 4 * (size_t)p;
    // the kept slots in ascending order (:225-255)
    int ncorr = 0;
    for (int base = 0; base < n1; base += 64) {
        const int i = base + lane;
        bool keep = false;
        int m = -1;
        if (i < n1) {
            m = a.match12[k1b + i];
            keep = a.valid1[k1b + i] && m >= 0 && m < n2 && a.valid2[k2b + m];
        }
        const uint64_t bal = __ballot(keep);
        if (keep) {
            const int pos = ncorr + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
            const size_t s1 = (size_t)k1b + i, s2 = (size_t)k2b + m;
            a.slots[k1b + pos] = i;   // pos < n1
            S3SRec r;
            const float3 c1 = pj_world_to_camera(P1, a.xw1[3 * s1], a.xw1[3 * s1 + 1], a.xw1[3 * s1 + 2]);
            const float3 c2 = pj_world_to_camera(P2, a.xw2[3 * s2], a.xw2[3 * s2 + 1], a.xw2[3 * s2 + 2]);
            r.X1[0] = c1.x; r.X1[1] = c1.y; r.X1[2] = c1.z;
            r.X2[0] = c2.x; r.X2[1] = c2.y; r.X2[2] = c2.z;
            s3h_to_image(K1, c1.x, c1.y, c1.z, r.p1);
            s3h_to_image(K2, c2.x, c2.y, c2.z, r.p2);
            r.pad[0] = 0.f; r.pad[1] = 0.f;
            r.thr1 = 9.21 * (double)a.sigma2[min(max(a.kp1_oct[s1], 0), a.n_levels - 1)];
            r.thr2 = 9.21 * (double)a.sigma2[min(max(a.kp2_oct[s2], 0), a.n_levels - 1)];
            a.recs[k1b + pos] = r;
        }
        ncorr += __popcll(bal);
    }
    if (lane == 0) {
        const int cap = a.caps[ncorr];   // ncorr <= n1 <= S3S_MAXKP
        const int it = min(max(a.o_iter[p], 0), cap);
        info[0] = ncorr;
        info[1] = it;
        info[2] = ncorr < a.min_inliers ? it : (int)min((long long)it + a.maxk, (long long)cap);
        info[3] = cap;
    }
}

// the records of hypothesis k's three correspondences -> S12, S21
__device__ __forceinline__ void s3s_hypothesis(const S3SArgs& a, int p, int k, int n, const S3SRec* recs, float* S12, float* S21) {
    int idx[3];
    s3h_pick(a.draws + 3 * ((size_t)p * a.max_iterations + k), a.rand_max, n, idx);
    float P1[9], P2[9];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const S3SRec& r = recs[idx[c]];
#pragma unroll
        for (int i = 0; i < 3; i++) { P1[3 * c + i] = r.X1[i]; P2[3 * c + i] = r.X2[i]; }
    }
    s3h_compute_sim3(P1, P2, a.fix_scale != 0, S12, S21);
}

__device__ __forceinline__ bool s3s_is_inlier(const S3SRec& r, const float* m12, const float* m21, const float* K1, const float* K2) {
    const float e1 = s3h_error_sq(m12, K1, r.X2[0], r.X2[1], r.X2[2], r.p1[0], r.p1[1]);
    const float e2 = s3h_error_sq(m21, K2, r.X1[0], r.X1[1], r.X1[2], r.p2[0], r.p2[1]);
    return (double)e1 < r.thr1 && (double)e2 < r.thr2;
}

__global__ __launch_bounds__(64) void s3s_eval_kernel(S3SArgs a) {
    __shared__ S3SRec tile[S3S_TILE];
    const int lane = threadIdx.x, p = blockIdx.x;
    const int32_t* info = a.info + 4 * (size_t)p;
    const int n = info[0], k0 = info[1], k1 = info[2];
    const int kw = k0 + blockIdx.y * 64;
    if (kw >= k1) return;   // wave-uniform: nothing to evaluate (also the over-limit and the too-few pairs)
    const int k = min(kw + lane, k1 - 1);   // the lanes past the range repeat its last hypothesis and write nothing
    const S3SRec* recs = a.recs + a.kp1_begin[p];
    const float* K1 = a.cam1 + 4 * (size_t)p;
    const float* K2 = a.cam2 + 4 * (size_t)p;
    const float cam1[4] = {K1[0], K1[1], K1[2], K1[3]}, cam2[4] = {K2[0], K2[1], K2[2], K2[3]};
    float S12[13], S21[13], m12[12], m21[12];
    s3s_hypothesis(a, p, k, n, recs, S12, S21);
    s3h_map_matrix(S12, m12);
    s3h_map_matrix(S21, m21);
    int count = 0;
    for (int base = 0; base < n; base += S3S_TILE) {
        const int nt = min(S3S_TILE, n - base);
        s3s_wave_sync();   // the previous tile has been read
        {   // 16 bytes per lane per step, coalesced
            const float4* src = reinterpret_cast<const float4*>(recs + base);
            float4* dst = reinterpret_cast<float4*>(tile);
            for (int j = lane; j < 4 * nt; j += 64) dst[j] = src[j];
        }
        s3s_wave_sync();
        for (int c = 0; c < nt; c++) count += s3s_is_inlier(tile[c], m12, m21, cam1, cam2) ? 1 : 0;
    }
    if (kw + lane < k1) a.hyp[(size_t)p * a.max_iterations + k] = count;
}

__global__ __launch_bounds__(64) void s3s_select_kernel(S3SArgs a) {
    const int lane = threadIdx.x, p = blockIdx.x;
    const int32_t* info = a.info + 4 * (size_t)p;
    const int n = info[0], k0 = info[1], k1 = info[2], cap = info[3];
    const int k1b = a.kp1_begin[p];
    const int n1 = a.kp1_begin[p + 1] - k1b;
    // isInlier.assign(nkeypoints1_, false) (:292), and no match survives until a hypothesis succeeds
    for (int i = lane; i < n1; i += 64) {
        a.o_inlier[k1b + i] = 0;
        a.o_match12[k1b + i] = -1;
    }
    int found = 0, ninl = 0, term = 0, iter = k1;
    int best = a.o_maxinl[p];
    int kstar = -1;
    if (n < 0) {   // over the keypoint limit
        found = -1; term = 1; iter = a.o_iter[p];
    } else if (n < a.min_inliers) {   // :294-298
        term = 1; iter = a.o_iter[p];
    } else {
        const int32_t* hyp = a.hyp + (size_t)p * a.max_iterations;
        for (int base = k0; base < k1 && kstar < 0; base += 64) {
            const int k = base + lane;
            const int v = k < k1 ? hyp[k] : -1;
            int ex = best;   // the maximum before k: the incoming state and every earlier count
            {
                int inc = v;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) {
                    const int o = __shfl_up(inc, d);
                    if (lane >= d) inc = max(inc, o);
                }
                const int prev = __shfl_up(inc, 1);
                if (lane > 0) ex = max(ex, prev);
                // :346-351: k updates iff n[k] >= maxInliers_, and succeeds iff it also has n[k] > minInliers_
                const uint64_t ok = __ballot(k < k1 && v >= ex && v > a.min_inliers);
                if (ok) {
                    const int l = __builtin_ctzll(ok);
                    kstar = base + l;
                    best = __shfl(v, l);
                } else {
                    best = max(best, __shfl(inc, 63));
                }
            }
        }
        if (kstar >= 0) {
            found = 1;
            iter = kstar + 1;
            const S3SRec* recs = a.recs + k1b;
            const float* K1 = a.cam1 + 4 * (size_t)p;
            const float* K2 = a.cam2 + 4 * (size_t)p;
            const float cam1[4] = {K1[0], K1[1], K1[2], K1[3]}, cam2[4] = {K2[0], K2[1], K2[2], K2[3]};
            float S12[13], S21[13], m12[12], m21[12];
            s3s_hypothesis(a, p, kstar, n, recs, S12, S21);   // wave-uniform, every lane the same
            s3h_map_matrix(S12, m12);
            s3h_map_matrix(S21, m21);
            s3s_wave_sync();   // the zeroes above, before other lanes set the same slots
            for (int base = 0; base < n; base += 64) {
                const int c = base + lane;
                const bool in = c < n && s3s_is_inlier(recs[c], m12, m21, cam1, cam2);
                if (in) {
                    const int i = a.slots[k1b + c];
                    a.o_inlier[k1b + i] = 1;
                    a.o_match12[k1b + i] = a.match12[k1b + i];
                }
                ninl += __popcll(__ballot(in));
            }
#pragma unroll
            for (int j = 0; j < 13; j++)
                if (lane == j) a.o_s12[13 * (size_t)p + j] = S12[j];
            if (a.hyp_is_output)   // the reference evaluated nothing past the success
                for (int k = kstar + 1 + lane; k < k1; k += 64) a.hyp[(size_t)p * a.max_iterations + k] = -1;
        } else {
            term = iter >= cap ? 1 : 0;   // :361-362
        }
    }
    if (found != 1 && lane < 13) a.o_s12[13 * (size_t)p + lane] = 0.f;
    if (lane == 0) {
        a.o_found[p] = found;
        a.o_ninl[p] = ninl;
        a.o_iter[p] = iter;
        a.o_maxinl[p] = best;
        a.o_term[p] = term;
    }
}

// SetRansacParameters (:266-287) for every nmatches: libm's values, which the device's log would not give.
// niterations is compared in double before it is narrowed (the reference narrows first, which overflows int
// for a tiny epsilon); below min_inliers the entry is not used (iterate() terminates first).
static void s3s_cap_table(double probability, int min_inliers, int max_iterations, int32_t* caps) {
    for (int n = 0; n < S3S_CAPS; n++) {
        int cap = 1;
        if (n > min_inliers) {
            const float epsilon = 1.f * min_inliers / n;
            const double it = std::ceil(std::log(1 - probability) / std::log(1 - std::pow(epsilon, 3)));
            cap = it >= (double)max_iterations ? max_iterations : (it >= 1.0 ? (int)it : 1);   // (NaN: 1)
        }
        caps[n] = std::max(1, std::min(cap, max_iterations));
    }
}

struct S3SCapEntry {
    double probability = 0;
    int min_inliers = 0, max_iterations = 0;
    DevBuf buf;
};

struct S3SScratch : Scratch {
    S3SCapEntry caps[4];   // the tables of the last parameter sets, uploaded once each
    int next_cap = 0;
    void device_changed() override {
        for (S3SCapEntry& c : caps) { c.buf.release(); c.max_iterations = 0; }
    }
    // The device copy of the cap table.  A new parameter set is uploaded with a synchronous copy (once, like
    // the workspace allocation); every later call with it enqueues nothing but the kernels.
    int cap_table(double probability, int min_inliers, int max_iterations, const int32_t** out) {
        for (S3SCapEntry& c : caps)
            if (c.max_iterations == max_iterations && c.min_inliers == min_inliers && c.probability == probability) {
                *out = c.buf.as<int32_t>();
                return ORB_OK;
            }
        S3SCapEntry& c = caps[next_cap];
        next_cap = (next_cap + 1) % 4;
        c.max_iterations = 0;
        int rc;
        if ((rc = c.buf.reserve(S3S_CAPS * sizeof(int32_t)))) return rc;
        std::vector<int32_t> host(S3S_CAPS);
        s3s_cap_table(probability, min_inliers, max_iterations, host.data());
        ORB_HIP_TRY(hipDeviceSynchronize());   // a kernel in flight may still read the table this one replaces
        ORB_HIP_TRY(hipMemcpy(c.buf.ptr, host.data(), S3S_CAPS * sizeof(int32_t), hipMemcpyHostToDevice));
        c.probability = probability; c.min_inliers = min_inliers; c.max_iterations = max_iterations;
        *out = c.buf.as<int32_t>();
        return ORB_OK;
    }
};
thread_local S3SScratch g_s3s;

}  // namespace orbamd

using namespace orbamd;

// The checks both entries share, and the kernel's arguments but for the workspace.
static int s3s_common(const orb_sim3solver_batch* in, const orb_sim3solver_result* out, S3SArgs& a) {
    ORB_CHECK_ARG(in && out, "null argument");
    ORB_CHECK_ARG(in->n_pairs >= 0 && in->total_kp1 >= 0 && in->total_kp2 >= 0, "negative sizes");
    ORB_CHECK_ARG(in->n_levels >= 1 && in->n_levels <= S3S_MAX_LEVELS && in->level_sigma2, "bad scale pyramid");
    ORB_CHECK_ARG(in->min_inliers >= 3, "min_inliers must be at least 3 (a hypothesis draws three correspondences)");
    ORB_CHECK_ARG(in->maxk >= 1, "maxk must be at least 1");
    ORB_CHECK_ARG(in->max_iterations >= 1, "max_iterations must be at least 1");
    ORB_CHECK_ARG(in->probability > 0.0 && in->probability < 1.0, "probability must lie in (0, 1)");
    ORB_CHECK_ARG(in->rand_max >= 1, "rand_max must be positive");
    if (in->n_pairs == 0) return ORB_OK;
    ORB_CHECK_ARG((long long)in->n_pairs * in->max_iterations * 3 < (1ll << 31), "n_pairs x max_iterations x 3 exceeds int32");
    ORB_CHECK_ARG(in->kp1_begin && in->kp2_begin && in->pose1 && in->pose2 && in->camera1 && in->camera2 && in->draws,
                  "null array");
    ORB_CHECK_ARG(in->total_kp1 == 0 || (in->kp1_octave && in->mp1_valid && in->mp1_xw && in->match12),
                  "null keyframe 1 array");
    ORB_CHECK_ARG(in->total_kp2 == 0 || (in->kp2_octave && in->mp2_valid && in->mp2_xw), "null keyframe 2 array");
    ORB_CHECK_ARG(out->s12 && out->found && out->n_inliers && out->iterations && out->max_inliers && out->terminate &&
                      (in->total_kp1 == 0 || (out->inlier && out->match12)),
                  "null output array");
    ORB_CHECK_ARG(out->match12 != in->match12 || in->total_kp1 == 0, "match12 out must not alias the input");
    std::memset(&a, 0, sizeof(a));
    a.n_pairs = in->n_pairs;
    a.kp1_begin = in->kp1_begin; a.kp2_begin = in->kp2_begin;
    a.kp1_oct = in->kp1_octave; a.kp2_oct = in->kp2_octave;
    a.pose1 = in->pose1; a.pose2 = in->pose2; a.cam1 = in->camera1; a.cam2 = in->camera2;
    a.valid1 = in->mp1_valid; a.valid2 = in->mp2_valid;
    a.xw1 = in->mp1_xw; a.xw2 = in->mp2_xw;
    a.match12 = in->match12;
    a.draws = in->draws;
    a.rand_max = in->rand_max;
    a.min_inliers = in->min_inliers; a.max_iterations = in->max_iterations; a.maxk = in->maxk;
    a.n_levels = in->n_levels;
    for (int l = 0; l < in->n_levels; l++) a.sigma2[l] = in->level_sigma2[l];
    a.fix_scale = in->fix_scale != 0;
    a.o_s12 = out->s12; a.o_inlier = out->inlier; a.o_match12 = out->match12;
    a.o_found = out->found; a.o_ninl = out->n_inliers; a.o_iter = out->iterations; a.o_maxinl = out->max_inliers;
    a.o_term = out->terminate;
    a.hyp = out->hyp_inliers;
    a.hyp_is_output = out->hyp_inliers != nullptr;
    return ORB_OK;
}

extern "C" int orb_sim3solver_iterate_device(const orb_sim3solver_batch* in, orb_sim3solver_result* out, void* stream) {
    S3SArgs a;
    int rc;
    if ((rc = s3s_common(in, out, a))) return rc;
    if (in->n_pairs == 0) return ORB_OK;
    if ((rc = g_s3s.use_current_device())) return rc;
    if ((rc = g_s3s.cap_table(in->probability, in->min_inliers, in->max_iterations, &a.caps))) return rc;
    const size_t K1 = std::max<size_t>(in->total_kp1, 1), F = in->n_pairs;
    const size_t o_recs = 0, o_slots = o_recs + align_up(K1 * sizeof(S3SRec), 256), o_info = o_slots + align_up(K1 * 4, 256),
                 o_hyp = o_info + align_up(F * 16, 256), total = o_hyp + (a.hyp ? 0 : F * in->max_iterations * 4);
    if ((rc = g_s3s.ws.reserve(total))) return rc;
    char* w = g_s3s.ws.as<char>();
    a.recs = (S3SRec*)(w + o_recs);
    a.slots = (int32_t*)(w + o_slots);
    a.info = (int32_t*)(w + o_info);
    if (!a.hyp) a.hyp = (int32_t*)(w + o_hyp);
    const hipStream_t st = (hipStream_t)stream;
    const int waves = (std::min(in->maxk, in->max_iterations) + 63) / 64;
    hipLaunchKernelGGL(s3s_prepare_kernel, dim3(a.n_pairs), dim3(64), 0, st, a);
    hipLaunchKernelGGL(s3s_eval_kernel, dim3(a.n_pairs, waves), dim3(64), 0, st, a);
    hipLaunchKernelGGL(s3s_select_kernel, dim3(a.n_pairs), dim3(64), 0, st, a);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orb_sim3solver_iterate(const orb_sim3solver_batch* in, orb_sim3solver_result* out, int device) {
    S3SArgs a;
    int rc;
    if ((rc = s3s_common(in, out, a))) return rc;   // the checks, before any copy
    const size_t F = in->n_pairs, K1 = in->total_kp1, K2 = in->total_kp2;
    if (F == 0) return ORB_OK;
    const int32_t *b1 = in->kp1_begin, *b2 = in->kp2_begin;
    ORB_CHECK_ARG(b1[0] == 0 && b2[0] == 0 && b1[F] == in->total_kp1 && b2[F] == in->total_kp2,
                  "kp1_begin / kp2_begin must start at 0 and end at total_kp1 / total_kp2");
    for (size_t p = 0; p < F; p++)
        ORB_CHECK_ARG(b1[p + 1] >= b1[p] && b2[p + 1] >= b2[p], "kp1_begin / kp2_begin must be non-decreasing");
    for (size_t p = 0; p < F; p++) {
        const int n2 = b2[p + 1] - b2[p];
        ORB_CHECK_ARG(b1[p + 1] - b1[p] <= S3S_MAXKP && n2 <= S3S_MAXKP, "a keyframe has more than ORBM_PROJ_MAX_KP keypoints");
        for (int i = b1[p]; i < b1[p + 1]; i++) {
            const int m = in->match12[i];
            ORB_CHECK_ARG(m >= -1 && m < n2, "match12 must be -1 or an index into keyframe 2 of its pair");
            ORB_CHECK_ARG(in->kp1_octave[i] >= 0 && in->kp1_octave[i] < in->n_levels, "kp1_octave out of range");
        }
        ORB_CHECK_ARG(out->iterations[p] >= 0 && out->max_inliers[p] >= 0, "iterations and max_inliers must not be negative");
    }
    for (size_t j = 0; j < K2; j++)
        ORB_CHECK_ARG(in->kp2_octave[j] >= 0 && in->kp2_octave[j] < in->n_levels, "kp2_octave out of range");
    const size_t n_draws = F * in->max_iterations * 3;
    for (size_t j = 0; j < n_draws; j++)
        ORB_CHECK_ARG(in->draws[j] >= 0 && in->draws[j] <= in->rand_max, "draws must lie in [0, rand_max]");
    orb_sim3solver_batch d = *in;
    d.kp1_xy = nullptr; d.kp2_xy = nullptr; d.s12 = nullptr;
    orb_sim3solver_result r = *out;
    Mirror io;
    io.add(d.kp1_begin, F + 1, true, false); io.add(d.kp2_begin, F + 1, true, false);
    io.add(d.kp1_octave, K1, true, false); io.add(d.kp2_octave, K2, true, false);
    io.add(d.pose1, F * 12, true, false); io.add(d.pose2, F * 12, true, false);
    io.add(d.camera1, F * 4, true, false); io.add(d.camera2, F * 4, true, false);
    io.add(d.mp1_valid, K1, true, false); io.add(d.mp2_valid, K2, true, false);
    io.add(d.mp1_xw, K1 * 3, true, false); io.add(d.mp2_xw, K2 * 3, true, false);
    io.add(d.match12, K1, true, false); io.add(d.draws, n_draws, true, false);
    io.add(r.iterations, F, true, true); io.add(r.max_inliers, F, true, true);
    io.add(r.s12, F * 13, false, true); io.add(r.inlier, K1, false, true); io.add(r.match12, K1, false, true);
    io.add(r.found, F, false, true); io.add(r.n_inliers, F, false, true); io.add(r.terminate, F, false, true);
    io.add(r.hyp_inliers, F * in->max_iterations, false, true);
    return run_host(g_s3s, device, io, [&] { return orb_sim3solver_iterate_device(&d, &r, nullptr); });
}
