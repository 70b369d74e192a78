// orbpnp.hip — PnPsolver::iterate (EPnP RANSAC, src/PnPsolver.cc:67-339) on gfx950, batched over the candidate
// keyframes of Tracking::Relocalization: one solver per frame slot range [kp_begin[p], kp_begin[p + 1]).
//
// A hypothesis depends on the solver's state only through the draw table, so the inlier counts n[k] of the whole
// range a call evaluates are computed at once and the control flow of iterate() walks them afterwards.  Three
// launches on the caller's stream, everything in fp64 except where the reference computes in float:
//   pnp_prepare_kernel  one wavefront per candidate: the matched slots compacted in ascending order (ballot +
//                       mbcnt), one 32-byte record per correspondence (P3Dw, P2D, maxError), N, the adjusted
//                       minInliers, the cap (host table, libm) and the range [k0, k1) of this call under the
//                       reference's OR rule (:182): k1 = max(cap, k0 + maxk)
//   pnp_eval_kernel     one lane per hypothesis, one wavefront per 64 hypotheses of a candidate: four draws, EPnP
//                       on four points (epnp.h) with the lane's work arrays private, the pose to the workspace,
//                       then the count over the candidate's records staged through LDS and read at a
//                       wave-uniform address
//   pnp_select_kernel   one wavefront per candidate: the events n[k] >= minInliers in order; a record (a strict
//                       new maximum) rewrites best_mask / best_tcw from the stored pose; Refine() runs at the
//                       first event and at every record (between records the best mask has not changed, so a
//                       repeated Refine() would fail again) with lanes over the best inliers and the wave sums of
//                       wave_sum.h, the 12x12 eigenproblem and the beta solves on lane 0 in LDS; then the outputs
//                       and the state
// Hypothesis k of candidate p always uses draws[p, k, :], so a result does not depend on how the iterations were
// split over calls.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "epnp.h"
#include "wave_sum.h"

namespace orbamd {

constexpr int PNP_TILE = 128;                  // correspondences per LDS tile: 4 KiB
constexpr int PNP_MAXKP = ORBM_PROJ_MAX_KP;
constexpr int PNP_MAX_LEVELS = 32;
constexpr int PNP_CAPS = PNP_MAXKP + 1;         // the cap for every N in 0 .. PNP_MAXKP

struct alignas(16) PnPRec {
    float X[3];      // P3Dw
    float p[2];      // P2D
    float max_err;   // mvMaxError
    float pad[2];
};
static_assert(sizeof(PnPRec) == 32, "");

struct PnPArgs {
    int n_frames;
    const int32_t* kp_begin;
    const float* kp_xy;
    const int32_t* kp_oct;
    const float* cam;
    const uint8_t* valid;
    const float* xw;
    const int32_t* draws;   // n_frames x n_draws x 4
    int n_draws;
    int32_t rand_max;
    int min_inliers, maxk, width;
    float epsilon, th2;
    int n_levels;
    float sigma2[PNP_MAX_LEVELS];
    const int32_t* caps;    // PNP_CAPS
    // outputs and state
    float* o_tcw;
    uint8_t* o_inlier;
    int32_t *o_found, *o_ninl, *o_term, *o_iter, *o_best;
    uint8_t* o_mask;
    float* o_btcw;
    int32_t* hyp;           // n_frames x n_draws: the caller's hyp_inliers or the workspace
    int hyp_is_output;
    // workspace
    int32_t* slots;         // total_kp: candidate p's matched slots, compacted, at kp_begin[p]
    PnPRec* recs;           // total_kp
    int32_t* info;          // n_frames x 8: N (-1: refused), k0, k1, cap, minInliers
    double* poses;          // n_frames x width x 12: R (row-major), t of hypothesis k0 + j
};

__device__ __forceinline__ void pnp_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// SetRansacParameters' minInliers (:134-139): int(N * epsilon) in float.
__host__ __device__ inline int pnp_min_inliers(int N, float epsilon, int min_inliers) {
    int m = static_cast<int>(N * epsilon);
    if (m < min_inliers) m = min_inliers;
    if (m < 4) m = 4;
    return m;
}

__global__ __launch_bounds__(64) void pnp_prepare_kernel(PnPArgs a) {
    const int lane = threadIdx.x, p = blockIdx.x;
    const int kb = a.kp_begin[p], nkp = a.kp_begin[p + 1] - kb;
    int32_t* info = a.info + 8 * (size_t)p;
    if (a.hyp_is_output)
        for (int k = lane; k < a.n_draws; k += 64) a.hyp[(size_t)p * a.n_draws + k] = -1;
    if (nkp > PNP_MAXKP) {
        if (lane == 0) { info[0] = -1; info[1] = 0; info[2] = 0; info[3] = 0; info[4] = 0; }
        return;
    }
    int n = 0;
    for (int base = 0; base < nkp; base += 64) {
        const int i = base + lane;
        const bool keep = i < nkp && a.valid[kb + i];
        const uint64_t bal = __ballot(keep);
        if (keep) {
            const int pos = n + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
            const size_t s = (size_t)kb + i;
            a.slots[kb + pos] = i;   // pos < nkp
            PnPRec r;
            r.X[0] = a.xw[3 * s]; r.X[1] = a.xw[3 * s + 1]; r.X[2] = a.xw[3 * s + 2];
            r.p[0] = a.kp_xy[2 * s]; r.p[1] = a.kp_xy[2 * s + 1];
            r.max_err = a.sigma2[min(max(a.kp_oct[s], 0), a.n_levels - 1)] * a.th2;
            r.pad[0] = 0.f; r.pad[1] = 0.f;
            a.recs[kb + pos] = r;
        }
        n += __popcll(bal);
    }
    if (lane == 0) {
        const int mi = pnp_min_inliers(n, a.epsilon, a.min_inliers);
        const int cap = a.caps[n];   // n <= nkp <= PNP_MAXKP
        const int it = max(a.o_iter[p], 0);
        long long k1 = it;
        if (n >= mi) k1 = std::max<long long>(cap, (long long)it + a.maxk);   // :182
        if (k1 > a.n_draws) {   // the range would read past the draw table
            info[0] = -1; info[1] = 0; info[2] = 0; info[3] = 0; info[4] = 0;
        } else {
            info[0] = n; info[1] = it; info[2] = (int)k1; info[3] = cap; info[4] = mi;
        }
    }
}

__global__ __launch_bounds__(64) void pnp_eval_kernel(PnPArgs a) {
    __shared__ PnPRec tile[PNP_TILE];
    const int lane = threadIdx.x, p = blockIdx.x;
    const int32_t* info = a.info + 8 * (size_t)p;
    const int n = info[0], k0 = info[1], k1 = info[2];
    const int kw = k0 + blockIdx.y * 64;
    if (kw >= k1) return;   // wave-uniform (also the refused candidates and those with too few correspondences)
    const int k = min(kw + lane, k1 - 1);   // the lanes past the range repeat its last hypothesis and write nothing
    const PnPRec* recs = a.recs + a.kp_begin[p];
    const float* K = a.cam + 4 * (size_t)p;
    const double cam[4] = {K[0], K[1], K[2], K[3]};
    double R[9], t[3];
    {
        int idx[4];
        epnp_pick4(a.draws + 4 * ((size_t)p * a.n_draws + k), a.rand_max, n, idx);
        double pw[12], us[8], alphas[16], W[144];
        for (int c = 0; c < 4; c++) {
            const PnPRec r = recs[idx[c]];
            pw[3 * c] = r.X[0]; pw[3 * c + 1] = r.X[1]; pw[3 * c + 2] = r.X[2];
            us[2 * c] = r.p[0]; us[2 * c + 1] = r.p[1];
        }
        epnp_pose_serial<true>(4, pw, us, cam, alphas, W, nullptr, R, t);
    }
    int count = 0;
    for (int base = 0; base < n; base += PNP_TILE) {
        const int nt = min(PNP_TILE, n - base);
        pnp_wave_sync();   // the previous tile has been read
        {
            const float4* src = reinterpret_cast<const float4*>(recs + base);
            float4* dst = reinterpret_cast<float4*>(tile);
            for (int j = lane; j < 2 * nt; j += 64) dst[j] = src[j];
        }
        pnp_wave_sync();
        for (int c = 0; c < nt; c++) count += epnp_is_inlier(R, t, cam, tile[c].X, tile[c].p, tile[c].max_err) ? 1 : 0;
    }
    if (kw + lane < k1) {
        a.hyp[(size_t)p * a.n_draws + k] = count;
        double* o = a.poses + 12 * ((size_t)p * a.width + (k - k0));   // k - k0 < width
        for (int i = 0; i < 9; i++) o[i] = R[i];
        for (int i = 0; i < 3; i++) o[9 + i] = t[i];
    }
}

struct PnPShared {
    double A[144], V[144], v[48], betas[12];
};

// Refine() (:260-305) on the candidate's best mask: EPnP over its inliers, then CheckInliers over all N.  Every
// lane returns the same R, t and count.  Sums: a lane adds its records c = lane, lane + 64, ... in ascending
// order, then po_wave_sum.
__device__ int pnp_refine(const PnPArgs& a, int lane, int n, const PnPRec* recs, const int32_t* slots, const uint8_t* mask,
                          const double cam[4], PnPShared& sh, double R[9], double t[3]) {
    int ninl = 0, first = -1;
    double c0[3] = {0, 0, 0};
    for (int base = 0; base < n; base += 64) {
        const int c = base + lane;
        const bool in = c < n && mask[slots[c]];
        const uint64_t bal = __ballot(in);
        if (first < 0 && bal) first = base + __builtin_ctzll(bal);
        ninl += __popcll(bal);
        if (in)
            for (int j = 0; j < 3; j++) c0[j] += (double)recs[c].X[j];
    }
    if (first < 0) return 0;   // (an empty mask: a state that no call of this solver wrote)
    for (int j = 0; j < 3; j++) c0[j] = po_wave_sum(c0[j], lane) / ninl;
    double S[6] = {0, 0, 0, 0, 0, 0};
    for (int c = lane; c < n; c += 64)
        if (mask[slots[c]]) {
            const double x = recs[c].X[0] - c0[0], y = recs[c].X[1] - c0[1], z = recs[c].X[2] - c0[2];
            S[0] += x * x; S[1] += x * y; S[2] += x * z; S[3] += y * y; S[4] += y * z; S[5] += z * z;
        }
    for (int j = 0; j < 6; j++) S[j] = po_wave_sum(S[j], lane);
    double cws[12], ci[9];
    epnp_control_points(S, ninl, c0, cws, ci);
    {   // MtM: the 78 entries of the upper triangle
        double acc[78];
#pragma unroll
        for (int i = 0; i < 78; i++) acc[i] = 0.0;
        for (int c = lane; c < n; c += 64)
            if (mask[slots[c]]) {
                const double pw[3] = {recs[c].X[0], recs[c].X[1], recs[c].X[2]};
                double al[4], m1[12], m2[12];
                epnp_alphas(ci, c0, pw, al);
                epnp_rows(al, recs[c].p[0], recs[c].p[1], cam, m1, m2);
                int e = 0;
#pragma unroll
                for (int r = 0; r < 12; r++)
#pragma unroll
                    for (int q = r; q < 12; q++) acc[e++] += m1[r] * m1[q] + m2[r] * m2[q];
            }
        pnp_wave_sync();   // the previous Refine() has read sh
        int e = 0;
#pragma unroll
        for (int r = 0; r < 12; r++)
#pragma unroll
            for (int q = r; q < 12; q++) {
                const double s = po_wave_sum(acc[e++], lane);
                if (lane == 0) { sh.A[12 * r + q] = s; sh.A[12 * q + r] = s; }
            }
    }
    if (lane == 0) {
        epnp_null_basis_refine(sh.A, sh.V, sh.v);
        epnp_all_betas(sh.v, cws, sh.betas);
    }
    pnp_wave_sync();
    double best = 0.0;
    for (int w = 0; w < 3; w++) {
        double ccs[12], be[4];
        for (int i = 0; i < 4; i++) be[i] = sh.betas[4 * w + i];
        epnp_ccs(be, sh.v, ccs);
        {   // solve_for_sign on the first inlier
            const double pw[3] = {recs[first].X[0], recs[first].X[1], recs[first].X[2]};
            double al[4], pc[3];
            epnp_alphas(ci, c0, pw, al);
            epnp_pc(al, ccs, pc);
            if (pc[2] < 0.0)
                for (int j = 0; j < 12; j++) ccs[j] = -ccs[j];
        }
        double pc0[3] = {0, 0, 0};
        for (int c = lane; c < n; c += 64)
            if (mask[slots[c]]) {
                const double pw[3] = {recs[c].X[0], recs[c].X[1], recs[c].X[2]};
                double al[4], pc[3];
                epnp_alphas(ci, c0, pw, al);
                epnp_pc(al, ccs, pc);
                for (int j = 0; j < 3; j++) pc0[j] += pc[j];
            }
        for (int j = 0; j < 3; j++) pc0[j] = po_wave_sum(pc0[j], lane) / ninl;
        double abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int c = lane; c < n; c += 64)
            if (mask[slots[c]]) {
                const double pw[3] = {recs[c].X[0], recs[c].X[1], recs[c].X[2]};
                double al[4], pc[3];
                epnp_alphas(ci, c0, pw, al);
                epnp_pc(al, ccs, pc);
                for (int j = 0; j < 3; j++)
                    for (int q = 0; q < 3; q++) abt[3 * j + q] += (pc[j] - pc0[j]) * (pw[q] - c0[q]);
            }
        for (int j = 0; j < 9; j++) abt[j] = po_wave_sum(abt[j], lane);
        double Rw[9], tw[3], err = 0.0;
        epnp_R_t(abt, pc0, c0, Rw, tw);   // pw0 is the centroid c0: the same sum
        for (int c = lane; c < n; c += 64)
            if (mask[slots[c]]) {
                const double pw[3] = {recs[c].X[0], recs[c].X[1], recs[c].X[2]};
                err += epnp_reproj(Rw, tw, cam, pw, recs[c].p[0], recs[c].p[1]);
            }
        err = po_wave_sum(err, lane) / ninl;
        if (w == 0 || err < best) {
            best = err;
            for (int i = 0; i < 9; i++) R[i] = Rw[i];
            for (int i = 0; i < 3; i++) t[i] = tw[i];
        }
    }
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int c = base + lane;
        const bool in = c < n && epnp_is_inlier(R, t, cam, recs[c].X, recs[c].p, recs[c].max_err);
        count += __popcll(__ballot(in));
    }
    return count;
}

__global__ __launch_bounds__(64) void pnp_select_kernel(PnPArgs a) {
    __shared__ PnPShared sh;
    const int lane = threadIdx.x, p = blockIdx.x;
    const int32_t* info = a.info + 8 * (size_t)p;
    const int n = info[0], k0 = info[1], k1 = info[2], cap = info[3], mi = info[4];
    const int kb = a.kp_begin[p], nkp = a.kp_begin[p + 1] - kb;
    for (int i = lane; i < nkp; i += 64) a.o_inlier[kb + i] = 0;
    pnp_wave_sync();   // before other lanes set the same slots
    const PnPRec* recs = a.recs + kb;
    const int32_t* slots = a.slots + kb;
    uint8_t* mask = a.o_mask + kb;
    float* btcw = a.o_btcw + 12 * (size_t)p;
    const float* K = a.cam + 4 * (size_t)p;
    const double cam[4] = {K[0], K[1], K[2], K[3]};
    int found = 0, ninl = 0, term = 0, iter = k1;
    int best = a.o_best[p];
    float tcw[12];
    for (int i = 0; i < 12; i++) tcw[i] = 0.f;
    if (n < 0) {   // refused
        found = -1; term = 1; iter = a.o_iter[p];
    } else if (n < mi) {   // :173-177
        term = 1; iter = a.o_iter[p];
    } else {
        const int32_t* hyp = a.hyp + (size_t)p * a.n_draws;
        bool first = true;
        for (int base = k0; base < k1 && !found; base += 64) {
            const int kl = base + lane;
            const int v = kl < k1 ? hyp[kl] : -1;
            uint64_t ev = __ballot(v >= mi);   // :209
            while (ev && !found) {
                const int l = __builtin_ctzll(ev);
                ev &= ev - 1;
                const int k = base + l, nk = __shfl(v, l);
                const bool record = nk > best;   // :212
                if (record) {
                    best = nk;
                    const double* P = a.poses + 12 * ((size_t)p * a.width + (k - k0));
                    double R[9], t[3];
                    for (int i = 0; i < 9; i++) R[i] = P[i];
                    for (int i = 0; i < 3; i++) t[i] = P[9 + i];
                    for (int i = lane; i < nkp; i += 64) mask[i] = 0;
                    pnp_wave_sync();
                    for (int c = lane; c < n; c += 64)
                        if (epnp_is_inlier(R, t, cam, recs[c].X, recs[c].p, recs[c].max_err)) mask[slots[c]] = 1;
                    if (lane < 12) btcw[lane] = (float)P[lane];
                    pnp_wave_sync();
                }
                if (record || first) {   // :226
                    double R[9], t[3];
                    const int cnt = pnp_refine(a, lane, n, recs, slots, mask, cam, sh, R, t);
                    if (cnt > mi) {   // :292
                        found = 1; ninl = cnt; iter = k + 1;
                        for (int i = 0; i < 9; i++) tcw[i] = (float)R[i];
                        for (int i = 0; i < 3; i++) tcw[9 + i] = (float)t[i];
                        for (int c = lane; c < n; c += 64)
                            if (epnp_is_inlier(R, t, cam, recs[c].X, recs[c].p, recs[c].max_err)) a.o_inlier[kb + slots[c]] = 1;
                        if (a.hyp_is_output)   // the reference evaluated nothing past the success
                            for (int j = k + 1 + lane; j < k1; j += 64) a.hyp[(size_t)p * a.n_draws + j] = -1;
                    }
                }
                first = false;
            }
        }
        if (!found) {
            term = iter >= cap ? 1 : 0;   // :241-255
            if (term && best >= mi) {
                found = 2; ninl = best;
                for (int i = 0; i < 12; i++) tcw[i] = btcw[i];
                for (int i = lane; i < nkp; i += 64) a.o_inlier[kb + i] = mask[i];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 12; j++)
        if (lane == j) a.o_tcw[12 * (size_t)p + j] = tcw[j];
    if (lane == 0) {
        a.o_found[p] = found;
        a.o_ninl[p] = ninl;
        a.o_iter[p] = iter;
        a.o_best[p] = best;
        a.o_term[p] = term;
    }
}

// SetRansacParameters (:121-152) for every N: libm's values, which the device's log and pow would not give.
// nIterations is compared in double before it is narrowed.  Below minInliers the entry is not used.
static void pnp_cap_table(double probability, int min_inliers, int max_iterations, float epsilon, int32_t* caps) {
    for (int n = 0; n < PNP_CAPS; n++) {
        const int mi = pnp_min_inliers(n, epsilon, min_inliers);
        int cap = 1;
        if (n > mi) {
            float eps = epsilon;
            if (eps < (float)mi / n) eps = (float)mi / n;
            const double it = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)eps, 3)));
            cap = it >= (double)max_iterations ? max_iterations : (it >= 1.0 ? (int)it : 1);   // (NaN: 1)
        }
        caps[n] = std::max(1, std::min(cap, max_iterations));
    }
}

struct PnPCapEntry {
    double probability = 0;
    float epsilon = 0;
    int min_inliers = 0, max_iterations = 0;
    DevBuf buf;
};

struct PnPScratch : Scratch {
    PnPCapEntry caps[4];   // the tables of the last parameter sets, uploaded once each
    int next_cap = 0;
    void device_changed() override {
        for (PnPCapEntry& c : caps) { c.buf.release(); c.max_iterations = 0; }
    }
    int cap_table(double probability, int min_inliers, int max_iterations, float epsilon, const int32_t** out) {
        for (PnPCapEntry& c : caps)
            if (c.max_iterations == max_iterations && c.min_inliers == min_inliers && c.probability == probability && c.epsilon == epsilon) {
                *out = c.buf.as<int32_t>();
                return ORB_OK;
            }
        PnPCapEntry& c = caps[next_cap];
        next_cap = (next_cap + 1) % 4;
        c.max_iterations = 0;
        int rc;
        if ((rc = c.buf.reserve(PNP_CAPS * sizeof(int32_t)))) return rc;
        std::vector<int32_t> host(PNP_CAPS);
        pnp_cap_table(probability, min_inliers, max_iterations, epsilon, host.data());
        ORB_HIP_TRY(hipDeviceSynchronize());   // a kernel in flight may still read the table this one replaces
        ORB_HIP_TRY(hipMemcpy(c.buf.ptr, host.data(), PNP_CAPS * sizeof(int32_t), hipMemcpyHostToDevice));
        c.probability = probability; c.min_inliers = min_inliers; c.max_iterations = max_iterations; c.epsilon = epsilon;
        *out = c.buf.as<int32_t>();
        return ORB_OK;
    }
};
thread_local PnPScratch g_pnp;

}  // namespace orbamd

using namespace orbamd;

// The checks both entries share, and the kernel's arguments but for the workspace.
static int pnp_common(const orb_pnpsolver_batch* in, const orb_pnpsolver_result* out, PnPArgs& a) {
    ORB_CHECK_ARG(in && out, "null argument");
    ORB_CHECK_ARG(in->n_frames >= 0 && in->total_kp >= 0, "negative sizes");
    ORB_CHECK_ARG(in->n_levels >= 1 && in->n_levels <= PNP_MAX_LEVELS && in->level_sigma2, "bad scale pyramid");
    ORB_CHECK_ARG(in->min_set == 4, "min_set must be 4 (EPnP's minimal case)");
    ORB_CHECK_ARG(in->min_inliers >= 6, "min_inliers must be at least 6 (Refine needs six correspondences)");
    ORB_CHECK_ARG(in->maxk >= 1, "maxk must be at least 1");
    ORB_CHECK_ARG(in->max_iterations >= 1, "max_iterations must be at least 1");
    ORB_CHECK_ARG(in->probability > 0.0 && in->probability < 1.0, "probability must lie in (0, 1)");
    ORB_CHECK_ARG(in->epsilon >= 0.f && in->epsilon <= 1.f, "epsilon must lie in [0, 1]");
    ORB_CHECK_ARG(in->th2 > 0.f, "th2 must be positive");
    ORB_CHECK_ARG(in->rand_max >= 1, "rand_max must be positive");
    ORB_CHECK_ARG(in->n_draws >= 1, "n_draws must be at least 1");
    if (in->n_frames == 0) return ORB_OK;
    ORB_CHECK_ARG((long long)in->n_frames * in->n_draws * 4 < (1ll << 31), "n_frames x n_draws x 4 exceeds int32");
    ORB_CHECK_ARG(in->kp_begin && in->camera && in->draws, "null array");
    ORB_CHECK_ARG(in->total_kp == 0 || (in->kp_xy && in->kp_octave && in->mp_valid && in->mp_xw), "null frame array");
    ORB_CHECK_ARG(out->tcw && out->found && out->n_inliers && out->terminate && out->iterations && out->best_inliers &&
                      out->best_tcw && (in->total_kp == 0 || (out->inlier && out->best_mask)),
                  "null output array");
    std::memset(&a, 0, sizeof(a));
    a.n_frames = in->n_frames;
    a.kp_begin = in->kp_begin; a.kp_xy = in->kp_xy; a.kp_oct = in->kp_octave; a.cam = in->camera;
    a.valid = in->mp_valid; a.xw = in->mp_xw;
    a.draws = in->draws; a.n_draws = in->n_draws; a.rand_max = in->rand_max;
    a.min_inliers = in->min_inliers; a.maxk = in->maxk;
    a.width = (int)std::min<long long>(std::max(in->maxk, in->max_iterations), in->n_draws);
    a.epsilon = in->epsilon; a.th2 = in->th2;
    a.n_levels = in->n_levels;
    for (int l = 0; l < in->n_levels; l++) a.sigma2[l] = in->level_sigma2[l];
    a.o_tcw = out->tcw; a.o_inlier = out->inlier; a.o_found = out->found; a.o_ninl = out->n_inliers; a.o_term = out->terminate;
    a.o_iter = out->iterations; a.o_best = out->best_inliers; a.o_mask = out->best_mask; a.o_btcw = out->best_tcw;
    a.hyp = out->hyp_inliers;
    a.hyp_is_output = out->hyp_inliers != nullptr;
    return ORB_OK;
}

extern "C" int orb_pnpsolver_iterate_device(const orb_pnpsolver_batch* in, orb_pnpsolver_result* out, void* stream) {
    PnPArgs a;
    int rc;
    if ((rc = pnp_common(in, out, a))) return rc;
    if (in->n_frames == 0) return ORB_OK;
    if ((rc = g_pnp.use_current_device())) return rc;
    if ((rc = g_pnp.cap_table(in->probability, in->min_inliers, in->max_iterations, in->epsilon, &a.caps))) return rc;
    const size_t K = std::max<size_t>(in->total_kp, 1), F = in->n_frames;
    const size_t o_recs = 0, o_slots = o_recs + align_up(K * sizeof(PnPRec), 256), o_info = o_slots + align_up(K * 4, 256),
                 o_poses = o_info + align_up(F * 32, 256), o_hyp = o_poses + align_up(F * a.width * 96, 256),
                 total = o_hyp + (a.hyp ? 0 : F * in->n_draws * 4);
    if ((rc = g_pnp.ws.reserve(total))) return rc;
    char* w = g_pnp.ws.as<char>();
    a.recs = (PnPRec*)(w + o_recs);
    a.slots = (int32_t*)(w + o_slots);
    a.info = (int32_t*)(w + o_info);
    a.poses = (double*)(w + o_poses);
    if (!a.hyp) a.hyp = (int32_t*)(w + o_hyp);
    const hipStream_t st = (hipStream_t)stream;
    const int waves = (a.width + 63) / 64;
    hipLaunchKernelGGL(pnp_prepare_kernel, dim3(a.n_frames), dim3(64), 0, st, a);
    hipLaunchKernelGGL(pnp_eval_kernel, dim3(a.n_frames, waves), dim3(64), 0, st, a);
    hipLaunchKernelGGL(pnp_select_kernel, dim3(a.n_frames), dim3(64), 0, st, a);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orb_pnpsolver_iterate(const orb_pnpsolver_batch* in, orb_pnpsolver_result* out, int device) {
    PnPArgs a;
    int rc;
    if ((rc = pnp_common(in, out, a))) return rc;   // the checks, before any copy
    const size_t F = in->n_frames, K = in->total_kp;
    if (F == 0) return ORB_OK;
    const int32_t* kb = in->kp_begin;
    ORB_CHECK_ARG(kb[0] == 0 && kb[F] == in->total_kp, "kp_begin must start at 0 and end at total_kp");
    for (size_t p = 0; p < F; p++) ORB_CHECK_ARG(kb[p + 1] >= kb[p], "kp_begin must be non-decreasing");
    std::vector<int32_t> caps(PNP_CAPS);
    pnp_cap_table(in->probability, in->min_inliers, in->max_iterations, in->epsilon, caps.data());
    for (size_t p = 0; p < F; p++) {
        ORB_CHECK_ARG(kb[p + 1] - kb[p] <= PNP_MAXKP, "a frame has more than ORBM_PROJ_MAX_KP keypoints");
        ORB_CHECK_ARG(out->iterations[p] >= 0 && out->best_inliers[p] >= 0, "iterations and best_inliers must not be negative");
        int n = 0;
        for (int i = kb[p]; i < kb[p + 1]; i++) n += in->mp_valid[i] != 0;
        const int mi = pnp_min_inliers(n, in->epsilon, in->min_inliers);
        if (n >= mi)
            ORB_CHECK_ARG(std::max<long long>(caps[n], (long long)out->iterations[p] + in->maxk) <= in->n_draws,
                          "n_draws is too small for the range this call evaluates: max(cap, iterations + maxk)");
    }
    for (size_t j = 0; j < K; j++)
        ORB_CHECK_ARG(in->kp_octave[j] >= 0 && in->kp_octave[j] < in->n_levels, "kp_octave out of range");
    const size_t n_draws = F * in->n_draws * 4;
    for (size_t j = 0; j < n_draws; j++)
        ORB_CHECK_ARG(in->draws[j] >= 0 && in->draws[j] <= in->rand_max, "draws must lie in [0, rand_max]");
    orb_pnpsolver_batch d = *in;
    orb_pnpsolver_result r = *out;
    Mirror io;
    io.add(d.kp_begin, F + 1, true, false); io.add(d.kp_xy, K * 2, true, false); io.add(d.kp_octave, K, true, false);
    io.add(d.camera, F * 4, true, false); io.add(d.mp_valid, K, true, false); io.add(d.mp_xw, K * 3, true, false);
    io.add(d.draws, n_draws, true, false);
    io.add(r.iterations, F, true, true); io.add(r.best_inliers, F, true, true); io.add(r.best_mask, K, true, true);
    io.add(r.best_tcw, F * 12, true, true);
    io.add(r.tcw, F * 12, false, true); io.add(r.inlier, K, false, true); io.add(r.found, F, false, true);
    io.add(r.n_inliers, F, false, true); io.add(r.terminate, F, false, true);
    io.add(r.hyp_inliers, F * in->n_draws, false, true);
    return run_host(g_pnp, device, io, [&] { return orb_pnpsolver_iterate_device(&d, &r, nullptr); });
}
