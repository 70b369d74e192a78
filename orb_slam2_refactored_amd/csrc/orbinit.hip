// orbinit.hip — Initializer::Initialize (H / F RANSAC + reconstruction) on gfx950, batched over (reference frame,
// current frame) pairs.
//
// src/Initializer.cc:45-122.  Every RANSAC hypothesis is independent and the winner is the first maximum of the
// per-hypothesis scores, so all of them are evaluated at once.  Five launches on the caller's stream:
//   ini_prepare_kernel      one wavefront per pair: Normalize (:750-796) over all keypoints of either frame, the
//                           matched slots compacted in ascending order (ballot + mbcnt), one 48-byte record per
//                           correspondence (raw u1 v1 u2 v2, the normalised pairs, the slot), the eight indices of
//                           every hypothesis (:83-98, init_hyp.h), hyp_score zeroed
//   ini_eval_kernel         one lane per hypothesis, grid (n_pairs, 2 models x ceil(max_iterations / 64)): the
//                           lane's H21i / H12i or F21i in registers (fp64 Jacobi, init_hyp.h), then the pair's raw
//                           records staged through LDS a tile at a time and read at a wave-uniform address (a
//                           broadcast), score += in the reference's order: no reduction, no atomics
//   ini_select_kernel       one wavefront per (pair, model): the first maximum of the scores, the winner's matrix,
//                           its inlier mask rebuilt with lanes over correspondences
//   ini_reconstruct_kernel  one wavefront per (pair, motion hypothesis): RH, the model, DecomposeE or the eight
//                           hypotheses of ReconstructH (every lane the same), CheckRT with lanes over
//                           correspondences, nGood by ballot, the parallax by rank counting over LDS
//   ini_finish_kernel       one wavefront per pair: the decision rules of ReconstructF / ReconstructH, then the
//                           winner's points into keypoint slots; everything zeroed without a success
// Normalize's sums are float: lane l adds the keypoints l, l + 64, ... in ascending order, then the 64 partial
// sums are combined by a butterfly (s = s + shfl_xor(s, d), d = 32, 16, .. 1), which gives every lane the same
// value.  Departures from the reference: see init_hyp.h.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "common.h"
#include "init_hyp.h"

namespace orbamd {

constexpr int INI_TILE = 256;                   // correspondences per LDS tile: 4 KiB
constexpr int INI_MAXKP = ORBM_PROJ_MAX_KP;

struct alignas(16) IniRec {
    float raw[4];    // u1, v1, u2, v2 (keypointsUn)
    float nrm[4];    // vPn1[first], vPn2[second]
    int32_t slot;    // first
    int32_t second;
    int32_t pad[2];
};
static_assert(sizeof(IniRec) == 48, "");

struct IniArgs {
    int n_pairs;
    const int32_t *kp1_begin, *kp2_begin;
    const float *kp1_xy, *kp2_xy;
    const int32_t* matches12;
    const float* camera;
    const int32_t* draws;
    int32_t rand_max;
    float sigma, min_parallax;
    int T, min_triangulated;
    double rh_threshold;
    // outputs
    int32_t *o_found, *o_model;
    float *o_rt, *o_p3d;
    uint8_t* o_tri;
    float* o_score[2];
    int32_t* o_best[2];
    float* o_mat[2];
    uint8_t* o_inl[2];
    float* o_hyp;
    int32_t* o_ngood;
    float* o_parallax;
    // workspace
    IniRec* recs;        // total_kp1: pair p's records, compacted, at kp1_begin[p]
    int32_t* info;       // n_pairs x 4: N (-1: over the limit), model, inliers of the model, ReconstructH went on
    float* tnorm;        // n_pairs x 8: T1, T2 as (sX, sY, -meanX sX, -meanY sY)
    int32_t* sets;       // n_pairs x T x 8
    float* hyp_mat;      // n_pairs x 2 x T x 9
    float* cand_p3d;     // 8 x total_kp1 x 3: motion hypothesis j of pair p at 8 * kp1_begin[p] + j * n1
    uint8_t* cand_flag;  // 8 x total_kp1: 1 counted, 2 vbGood
    float* cand_rt;      // n_pairs x 8 x 12
};

// writes of other lanes of this wavefront become readable
__device__ __forceinline__ void ini_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ float ini_wave_sum(float s) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s = s + __shfl_xor(s, d);
    return s;
}

// Normalize (:750-796) of one frame: nm = meanX, meanY, sX, sY
__device__ __forceinline__ void ini_normalize(const float* xy, int n, int lane, float* nm) {
    float sx = 0, sy = 0;
    for (int i = lane; i < n; i += 64) { sx += xy[2 * i]; sy += xy[2 * i + 1]; }
    const float meanX = ini_wave_sum(sx) / n, meanY = ini_wave_sum(sy) / n;
    float dx = 0, dy = 0;
    for (int i = lane; i < n; i += 64) { dx += fabsf(xy[2 * i] - meanX); dy += fabsf(xy[2 * i + 1] - meanY); }
    const float meanDevX = ini_wave_sum(dx) / n, meanDevY = ini_wave_sum(dy) / n;
    nm[0] = meanX; nm[1] = meanY; nm[2] = 1.f / meanDevX; nm[3] = 1.f / meanDevY;
}

__global__ __launch_bounds__(64) void ini_prepare_kernel(IniArgs a) {
    const int lane = threadIdx.x, p = blockIdx.x;
    const int k1b = a.kp1_begin[p], k2b = a.kp2_begin[p];
    const int n1 = a.kp1_begin[p + 1] - k1b, n2 = a.kp2_begin[p + 1] - k2b;
    int32_t* info = a.info + 4 * (size_t)p;
    for (int k = lane; k < 2 * a.T; k += 64) a.o_hyp[(size_t)p * 2 * a.T + k] = 0.f;
    if (n1 > INI_MAXKP || n2 > INI_MAXKP || n1 < 0 || n2 < 0) {
        if (lane == 0) { info[0] = -1; info[1] = 0; info[2] = 0; info[3] = 0; }
        return;
    }
    const float* xy1 = a.kp1_xy + 2 * (size_t)k1b;
    const float* xy2 = a.kp2_xy + 2 * (size_t)k2b;
    float m1[4], m2[4];
    ini_normalize(xy1, n1, lane, m1);
    ini_normalize(xy2, n2, lane, m2);
    if (lane == 0) {
        float* T = a.tnorm + 8 * (size_t)p;
        T[0] = m1[2]; T[1] = m1[3]; T[2] = -m1[0] * m1[2]; T[3] = -m1[1] * m1[3];
        T[4] = m2[2]; T[5] = m2[3]; T[6] = -m2[0] * m2[2]; T[7] = -m2[1] * m2[3];
    }
    // mvMatches12 (:55-64)
    int ncorr = 0;
    for (int base = 0; base < n1; base += 64) {
        const int i = base + lane;
        int m = -1;
        if (i < n1) m = a.matches12[k1b + i];
        const bool keep = m >= 0 && m < n2;
        const uint64_t bal = __ballot(keep);
        if (keep) {
            const int pos = ncorr + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
            IniRec r;
            r.raw[0] = xy1[2 * i]; r.raw[1] = xy1[2 * i + 1]; r.raw[2] = xy2[2 * m]; r.raw[3] = xy2[2 * m + 1];
            r.nrm[0] = (r.raw[0] - m1[0]) * m1[2]; r.nrm[1] = (r.raw[1] - m1[1]) * m1[3];
            r.nrm[2] = (r.raw[2] - m2[0]) * m2[2]; r.nrm[3] = (r.raw[3] - m2[1]) * m2[3];
            r.slot = i; r.second = m; r.pad[0] = 0; r.pad[1] = 0;
            a.recs[k1b + pos] = r;   // pos < n1
        }
        ncorr += __popcll(bal);
    }
    if (lane == 0) { info[0] = ncorr; info[1] = 0; info[2] = 0; info[3] = 0; }
    if (ncorr < 8) return;
    for (int it = lane; it < a.T; it += 64) {
        int idx[8];
        const size_t at = 8 * ((size_t)p * a.T + it);
        ini_pick8(a.draws + at, a.rand_max, ncorr, idx);
#pragma unroll
        for (int j = 0; j < 8; j++) a.sets[at + j] = idx[j];
    }
}

__global__ __launch_bounds__(64) void ini_eval_kernel(IniArgs a, int waves) {
    __shared__ float4 tile[INI_TILE];
    const int lane = threadIdx.x, p = blockIdx.x;
    const int model = blockIdx.y / waves, it0 = (blockIdx.y % waves) * 64;
    const int n = a.info[4 * (size_t)p];
    if (n < 8 || it0 >= a.T) return;   // wave-uniform
    const int it = min(it0 + lane, a.T - 1);   // the lanes past the end repeat the last hypothesis and write nothing
    const IniRec* recs = a.recs + a.kp1_begin[p];
    const float* T = a.tnorm + 8 * (size_t)p;
    const float T1[4] = {T[0], T[1], T[2], T[3]}, T2[4] = {T[4], T[5], T[6], T[7]};
    float pn1[16], pn2[16];
    {
        const int32_t* set = a.sets + 8 * ((size_t)p * a.T + it);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float4 v = *reinterpret_cast<const float4*>(recs[set[j]].nrm);   // set[j] < n
            pn1[2 * j] = v.x; pn1[2 * j + 1] = v.y; pn2[2 * j] = v.z; pn2[2 * j + 1] = v.w;
        }
    }
    float M[9], Minv[9];
    if (model == 0) {
        double Hn[9], H[9], Hi[9];
        ini_compute_h21(pn1, pn2, Hn);
        ini_h21i(T1, T2, Hn, H);
        ini_round9(H, M);
        ini_inv3f(M, Hi);
        ini_round9(Hi, Minv);
    } else {
        double Fpre[9], Fn[9], F[9];
        ini_compute_f21(pn1, pn2, Fpre, Fn);
        ini_f21i(T1, T2, Fn, F);
        ini_round9(F, M);
#pragma unroll
        for (int i = 0; i < 9; i++) Minv[i] = 0.f;
    }
    const float invSigmaSquare = 1.f / (a.sigma * a.sigma);
    float score = 0;
    for (int base = 0; base < n; base += INI_TILE) {
        const int nt = min(INI_TILE, n - base);
        ini_wave_sync();   // the previous tile has been read
        for (int j = lane; j < nt; j += 64) tile[j] = *reinterpret_cast<const float4*>(recs[base + j].raw);
        ini_wave_sync();
        if (model == 0) {
            for (int c = 0; c < nt; c++) {
                const float4 r = tile[c];
                ini_check_h(M, Minv, r.x, r.y, r.z, r.w, invSigmaSquare, score);
            }
        } else {
            for (int c = 0; c < nt; c++) {
                const float4 r = tile[c];
                ini_check_f(M, r.x, r.y, r.z, r.w, invSigmaSquare, score);
            }
        }
    }
    if (it0 + lane < a.T) {
        const size_t h = ((size_t)p * 2 + model) * a.T + it;
        a.o_hyp[h] = score;
#pragma unroll
        for (int i = 0; i < 9; i++) a.hyp_mat[9 * h + i] = M[i];
    }
}

__global__ __launch_bounds__(64) void ini_select_kernel(IniArgs a) {
    const int lane = threadIdx.x, p = blockIdx.x, model = blockIdx.y;
    const int n = a.info[4 * (size_t)p];
    const int k1b = a.kp1_begin[p];
    const int n1 = n < 0 ? 0 : a.kp1_begin[p + 1] - k1b;
    uint8_t* inl = a.o_inl[model];
    if (n < 0) {   // over the limit: its slots are still the caller's to read
        for (int i = lane; i < a.kp1_begin[p + 1] - k1b; i += 64) inl[k1b + i] = 0;
    }
    for (int i = lane; i < n1; i += 64) inl[k1b + i] = 0;
    // FindHomography / FindFundamental (:149-172, :200-223): currentScore > score from score = 0, it ascending
    float bs = 0.f;
    int bi = INT_MAX;
    if (n >= 8) {
        const float* hyp = a.o_hyp + ((size_t)p * 2 + model) * a.T;
        for (int it = lane; it < a.T; it += 64) {
            const float s = hyp[it];
            if (s > bs) { bs = s; bi = it; }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float os = __shfl_xor(bs, d);
            const int oi = __shfl_xor(bi, d);
            const bool take = os > bs || (os == bs && oi < bi);
            bs = take ? os : bs;
            bi = take ? oi : bi;
        }
    }
    const bool have = bi != INT_MAX;
    float M[9], Minv[9];
#pragma unroll
    for (int i = 0; i < 9; i++) { M[i] = 0.f; Minv[i] = 0.f; }
    if (have) {
        const float* src = a.hyp_mat + 9 * (((size_t)p * 2 + model) * a.T + bi);
#pragma unroll
        for (int i = 0; i < 9; i++) M[i] = src[i];
        if (model == 0) {
            double Hi[9];
            ini_inv3f(M, Hi);
            ini_round9(Hi, Minv);
        }
        const IniRec* recs = a.recs + k1b;
        const float invSigmaSquare = 1.f / (a.sigma * a.sigma);
        ini_wave_sync();   // the zeroes above, before other lanes set the same slots
        for (int base = 0; base < n; base += 64) {
            const int c = base + lane;
            if (c < n) {
                const IniRec& r = recs[c];
                float unused = 0;
                const bool in = model == 0 ? ini_check_h(M, Minv, r.raw[0], r.raw[1], r.raw[2], r.raw[3], invSigmaSquare, unused)
                                           : ini_check_f(M, r.raw[0], r.raw[1], r.raw[2], r.raw[3], invSigmaSquare, unused);
                if (in) inl[k1b + r.slot] = 1;
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 9; i++)
        if (lane == i) a.o_mat[model][9 * (size_t)p + i] = M[i];
    if (lane == 0) {
        a.o_score[model][p] = have ? bs : 0.f;
        a.o_best[model][p] = have ? bi : -1;
    }
}

__global__ __launch_bounds__(64) void ini_reconstruct_kernel(IniArgs a) {
    __shared__ float cosv[INI_MAXKP];
    const int lane = threadIdx.x, p = blockIdx.x, j = blockIdx.y;
    const int n = a.info[4 * (size_t)p];
    const int k1b = a.kp1_begin[p];
    const int n1 = a.kp1_begin[p + 1] - k1b;
    // :113-119
    const float SH = a.o_score[0][p], SF = a.o_score[1][p];
    const float RH = SH / (SH + SF);
    const int model = RH > a.rh_threshold ? 0 : 1;
    const int best = a.o_best[model][p];
    int ngood = 0, N = 0, went_on = 0;
    float parallax = 0.f;
    if (n >= 8 && best >= 0 && !(model == 1 && j >= 4)) {
        const float* cam = a.camera + 4 * (size_t)p;
        const float camf[4] = {cam[0], cam[1], cam[2], cam[3]};
        float M[9];
#pragma unroll
        for (int i = 0; i < 9; i++) M[i] = a.o_mat[model][9 * (size_t)p + i];
        float R[9], t[3];
        bool ok = true;
        if (model == 1) {
            float R1[9], R2[9], tt[3];
            ini_decompose_e(M, camf, R1, R2, tt);
            const bool second = (j & 1) != 0, neg = j >= 2;   // (R1, t), (R2, t), (R1, -t), (R2, -t) (:495-498)
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = second ? R2[i] : R1[i];
#pragma unroll
            for (int i = 0; i < 3; i++) t[i] = neg ? -tt[i] : tt[i];
        } else {
            float R8[72], t8[24];
            ok = ini_decompose_h(M, camf, R8, t8);
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = 0.f;
#pragma unroll
            for (int i = 0; i < 3; i++) t[i] = 0.f;
#pragma unroll
            for (int h = 0; h < 8; h++) {
#pragma unroll
                for (int i = 0; i < 9; i++) R[i] = h == j ? R8[9 * h + i] : R[i];
#pragma unroll
                for (int i = 0; i < 3; i++) t[i] = h == j ? t8[3 * h + i] : t[i];
            }
        }
        went_on = ok ? 1 : 0;
        const uint8_t* mask = a.o_inl[model] + k1b;
        const IniRec* recs = a.recs + k1b;
        if (ok) {
            IniView view;
            ini_view(R, t, camf, view);
            const float th2 = 4.f * (a.sigma * a.sigma);
            const size_t cb = 8 * (size_t)k1b + (size_t)j * n1;
            for (int base = 0; base < n; base += 64) {
                const int c = base + lane;
                bool in = false, counted = false, good = false;
                float cp = 0.f, x[3] = {0.f, 0.f, 0.f};
                if (c < n) {
                    const IniRec& r = recs[c];
                    in = mask[r.slot] != 0;
                    if (in) counted = ini_check_rt(view, r.raw[0], r.raw[1], r.raw[2], r.raw[3], th2, x, cp, good);
                    a.cand_p3d[3 * (cb + c)] = x[0];   // c < n <= n1
                    a.cand_p3d[3 * (cb + c) + 1] = x[1];
                    a.cand_p3d[3 * (cb + c) + 2] = x[2];
                    a.cand_flag[cb + c] = (uint8_t)((counted ? 1 : 0) | (good ? 2 : 0));
                    cosv[c] = counted ? cp : std::numeric_limits<float>::infinity();   // c < n <= INI_MAXKP
                }
                ngood += __popcll(__ballot(counted));
                N += __popcll(__ballot(in));
            }
#pragma unroll
            for (int i = 0; i < 12; i++)
                if (lane == i) a.cand_rt[12 * ((size_t)p * 8 + j) + i] = i < 9 ? R[i < 9 ? i : 0] : t[i >= 9 ? i - 9 : 0];
            if (ngood > 0) {
                // the element of rank min(50, nGood - 1) of the sorted vCosParallax (:899-902): the counted c with
                // exactly that many counted (cos, index) pairs below it
                ini_wave_sync();
                const int target = min(50, ngood - 1);
                for (int base = 0; base < n; base += 64) {
                    const int c = base + lane;
                    const float mine = c < n ? cosv[c] : std::numeric_limits<float>::infinity();
                    const bool cand = c < n && mine != std::numeric_limits<float>::infinity();
                    int rank = 0;
                    for (int o = 0; o < n; o++) {
                        const float v = cosv[o];
                        rank += (v < mine || (v == mine && o < c)) ? 1 : 0;
                    }
                    const uint64_t hit = __ballot(cand && rank == target);
                    if (hit) parallax = ini_parallax_deg(__shfl(mine, __builtin_ctzll(hit)));
                }
            }
        } else {
            for (int base = 0; base < n; base += 64) {
                const int c = base + lane;
                N += __popcll(__ballot(c < n && mask[recs[min(c, n - 1)].slot] != 0));
            }
        }
    }
    if (lane == 0) {
        a.o_ngood[(size_t)p * 8 + j] = ngood;
        a.o_parallax[(size_t)p * 8 + j] = parallax;
        if (j == 0) {
            int32_t* info = a.info + 4 * (size_t)p;
            info[1] = model; info[2] = N; info[3] = went_on;
        }
    }
}

__global__ __launch_bounds__(64) void ini_finish_kernel(IniArgs a) {
    const int lane = threadIdx.x, p = blockIdx.x;
    const int32_t* info = a.info + 4 * (size_t)p;
    const int n = info[0], model = info[1], N = info[2], went_on = info[3];
    const int k1b = a.kp1_begin[p];
    const int n1 = a.kp1_begin[p + 1] - k1b;
    for (int i = lane; i < n1; i += 64) {
        a.o_p3d[3 * ((size_t)k1b + i)] = 0.f;
        a.o_p3d[3 * ((size_t)k1b + i) + 1] = 0.f;
        a.o_p3d[3 * ((size_t)k1b + i) + 2] = 0.f;
        a.o_tri[k1b + i] = 0;
    }
    int g[8];
    float par[8];
#pragma unroll
    for (int h = 0; h < 8; h++) { g[h] = a.o_ngood[(size_t)p * 8 + h]; par[h] = a.o_parallax[(size_t)p * 8 + h]; }
    int win = -1;
    if (n >= 8 && model == 1) {   // ReconstructF (:500-570)
        const int maxGood = max(g[0], max(g[1], max(g[2], g[3])));
        const int nMinGood = max((int)(0.9 * N), a.min_triangulated);
        int nsimilar = 0;
#pragma unroll
        for (int h = 0; h < 4; h++) nsimilar += g[h] > 0.7 * maxGood ? 1 : 0;
        if (!(maxGood < nMinGood || nsimilar > 1)) {
            const int first = maxGood == g[0] ? 0 : maxGood == g[1] ? 1 : maxGood == g[2] ? 2 : 3;
            float pf = par[0];
#pragma unroll
            for (int h = 1; h < 4; h++) pf = first == h ? par[h] : pf;
            if (pf > a.min_parallax) win = first;
        }
    } else if (n >= 8 && went_on) {   // ReconstructH (:690-730)
        int bestGood = 0, secondBestGood = 0, bestIdx = -1;
        float bestParallax = -1;
#pragma unroll
        for (int h = 0; h < 8; h++) {
            if (g[h] > bestGood) {
                secondBestGood = bestGood;
                bestGood = g[h];
                bestIdx = h;
                bestParallax = par[h];
            } else if (g[h] > secondBestGood) {
                secondBestGood = g[h];
            }
        }
        if (secondBestGood < 0.75 * bestGood && bestParallax >= a.min_parallax && bestGood > a.min_triangulated &&
            bestGood > 0.9 * N)
            win = bestIdx;
    }
    if (win >= 0) {
        const IniRec* recs = a.recs + k1b;
        const size_t cb = 8 * (size_t)k1b + (size_t)win * n1;
        ini_wave_sync();   // the zeroes above
        for (int c = lane; c < n; c += 64) {
            const uint8_t f = a.cand_flag[cb + c];
            const size_t s = (size_t)k1b + recs[c].slot;
            if (f & 1) {
                a.o_p3d[3 * s] = a.cand_p3d[3 * (cb + c)];
                a.o_p3d[3 * s + 1] = a.cand_p3d[3 * (cb + c) + 1];
                a.o_p3d[3 * s + 2] = a.cand_p3d[3 * (cb + c) + 2];
            }
            if (f & 2) a.o_tri[s] = 1;
        }
    }
    if (lane < 12) a.o_rt[12 * (size_t)p + lane] = win >= 0 ? a.cand_rt[12 * ((size_t)p * 8 + win) + lane] : 0.f;
    if (lane == 0) {
        a.o_found[p] = n < 0 ? -1 : (win >= 0 ? 1 : 0);
        a.o_model[p] = n < 0 ? 0 : model;
    }
}

thread_local Scratch g_ini;

}  // namespace orbamd

using namespace orbamd;

// The checks both entries share, and the kernel's arguments but for the workspace.
static int ini_common(const orb_initializer_batch* in, const orb_initializer_result* out, IniArgs& a) {
    ORB_CHECK_ARG(in && out, "null argument");
    ORB_CHECK_ARG(in->n_pairs >= 0 && in->total_kp1 >= 0 && in->total_kp2 >= 0, "negative sizes");
    ORB_CHECK_ARG(in->max_iterations >= 1, "max_iterations must be at least 1");
    ORB_CHECK_ARG(in->sigma > 0.f, "sigma must be positive");
    ORB_CHECK_ARG(in->rand_max >= 1, "rand_max must be positive");
    ORB_CHECK_ARG(in->min_triangulated >= 0, "min_triangulated must not be negative");
    if (in->n_pairs == 0) return ORB_OK;
    ORB_CHECK_ARG((long long)in->n_pairs * in->max_iterations * 18 < (1ll << 31), "n_pairs x max_iterations x 18 exceeds int32");
    ORB_CHECK_ARG(in->kp1_begin && in->kp2_begin && in->camera && in->draws, "null array");
    ORB_CHECK_ARG(in->total_kp1 == 0 || (in->kp1_xy && in->matches12), "null frame 1 array");
    ORB_CHECK_ARG(in->total_kp2 == 0 || in->kp2_xy, "null frame 2 array");
    ORB_CHECK_ARG(out->found && out->model && out->r21t21 && out->score_h && out->score_f && out->best_h && out->best_f &&
                      out->h21 && out->f21 && out->hyp_score && out->n_good && out->parallax &&
                      (in->total_kp1 == 0 || (out->p3d && out->triangulated && out->inlier_h && out->inlier_f)),
                  "null output array");
    std::memset(&a, 0, sizeof(a));
    a.n_pairs = in->n_pairs;
    a.kp1_begin = in->kp1_begin; a.kp2_begin = in->kp2_begin;
    a.kp1_xy = in->kp1_xy; a.kp2_xy = in->kp2_xy;
    a.matches12 = in->matches12;
    a.camera = in->camera;
    a.draws = in->draws;
    a.rand_max = in->rand_max;
    a.sigma = in->sigma; a.min_parallax = in->min_parallax;
    a.T = in->max_iterations; a.min_triangulated = in->min_triangulated;
    a.rh_threshold = in->rh_threshold;
    a.o_found = out->found; a.o_model = out->model; a.o_rt = out->r21t21; a.o_p3d = out->p3d; a.o_tri = out->triangulated;
    a.o_score[0] = out->score_h; a.o_score[1] = out->score_f;
    a.o_best[0] = out->best_h; a.o_best[1] = out->best_f;
    a.o_mat[0] = out->h21; a.o_mat[1] = out->f21;
    a.o_inl[0] = out->inlier_h; a.o_inl[1] = out->inlier_f;
    a.o_hyp = out->hyp_score; a.o_ngood = out->n_good; a.o_parallax = out->parallax;
    return ORB_OK;
}

extern "C" int orb_initializer_initialize_device(const orb_initializer_batch* in, orb_initializer_result* out, void* stream) {
    IniArgs a;
    int rc;
    if ((rc = ini_common(in, out, a))) return rc;
    if (in->n_pairs == 0) return ORB_OK;
    if ((rc = g_ini.use_current_device())) return rc;
    const size_t K1 = std::max<size_t>(in->total_kp1, 1), F = in->n_pairs, T = in->max_iterations;
    auto carve = [&](char* base) {
        Carver c{base};
        c.take(a.recs, K1); c.take(a.info, F * 4); c.take(a.tnorm, F * 8); c.take(a.sets, F * T * 8);
        c.take(a.hyp_mat, F * 2 * T * 9); c.take(a.cand_p3d, 8 * K1 * 3); c.take(a.cand_flag, 8 * K1); c.take(a.cand_rt, F * 8 * 12);
        return c.off;
    };
    if ((rc = g_ini.ws.reserve(carve(nullptr)))) return rc;
    carve(g_ini.ws.as<char>());
    const hipStream_t st = (hipStream_t)stream;
    const int waves = (in->max_iterations + 63) / 64;
    hipLaunchKernelGGL(ini_prepare_kernel, dim3(a.n_pairs), dim3(64), 0, st, a);
    hipLaunchKernelGGL(ini_eval_kernel, dim3(a.n_pairs, 2 * waves), dim3(64), 0, st, a, waves);
    hipLaunchKernelGGL(ini_select_kernel, dim3(a.n_pairs, 2), dim3(64), 0, st, a);
    hipLaunchKernelGGL(ini_reconstruct_kernel, dim3(a.n_pairs, 8), dim3(64), 0, st, a);
    hipLaunchKernelGGL(ini_finish_kernel, dim3(a.n_pairs), dim3(64), 0, st, a);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orb_initializer_initialize(const orb_initializer_batch* in, orb_initializer_result* out, int device) {
    IniArgs a;
    int rc;
    if ((rc = ini_common(in, out, a))) return rc;   // the checks, before any copy
    const size_t F = in->n_pairs, K1 = in->total_kp1, K2 = in->total_kp2, T = in->max_iterations;
    if (F == 0) return ORB_OK;
    const int32_t *b1 = in->kp1_begin, *b2 = in->kp2_begin;
    ORB_CHECK_ARG(b1[0] == 0 && b2[0] == 0 && b1[F] == in->total_kp1 && b2[F] == in->total_kp2,
                  "kp1_begin / kp2_begin must start at 0 and end at total_kp1 / total_kp2");
    for (size_t p = 0; p < F; p++)
        ORB_CHECK_ARG(b1[p + 1] >= b1[p] && b2[p + 1] >= b2[p], "kp1_begin / kp2_begin must be non-decreasing");
    for (size_t p = 0; p < F; p++) {
        const int n2 = b2[p + 1] - b2[p];
        ORB_CHECK_ARG(b1[p + 1] - b1[p] <= INI_MAXKP && n2 <= INI_MAXKP, "a frame has more than ORBM_PROJ_MAX_KP keypoints");
        for (int i = b1[p]; i < b1[p + 1]; i++)
            ORB_CHECK_ARG(in->matches12[i] >= -1 && in->matches12[i] < n2, "matches12 must be -1 or an index into frame 2 of its pair");
    }
    const size_t n_draws = F * T * 8;
    for (size_t j = 0; j < n_draws; j++)
        ORB_CHECK_ARG(in->draws[j] >= 0 && in->draws[j] <= in->rand_max, "draws must lie in [0, rand_max]");
    orb_initializer_batch d = *in;
    orb_initializer_result r = *out;
    Mirror io;
    io.add(d.kp1_begin, F + 1, true, false); io.add(d.kp2_begin, F + 1, true, false); io.add(d.kp1_xy, K1 * 2, true, false);
    io.add(d.kp2_xy, K2 * 2, true, false); io.add(d.matches12, K1, true, false); io.add(d.camera, F * 4, true, false);
    io.add(d.draws, n_draws, true, false);
    io.add(r.found, F, false, true); io.add(r.model, F, false, true); io.add(r.r21t21, F * 12, false, true);
    io.add(r.p3d, K1 * 3, false, true); io.add(r.triangulated, K1, false, true); io.add(r.score_h, F, false, true);
    io.add(r.score_f, F, false, true); io.add(r.best_h, F, false, true); io.add(r.best_f, F, false, true);
    io.add(r.h21, F * 9, false, true); io.add(r.f21, F * 9, false, true); io.add(r.inlier_h, K1, false, true);
    io.add(r.inlier_f, K1, false, true); io.add(r.hyp_score, F * 2 * T, false, true); io.add(r.n_good, F * 8, false, true);
    io.add(r.parallax, F * 8, false, true);
    return run_host(g_ini, device, io, [&] { return orb_initializer_initialize_device(&d, &r, nullptr); });
}
