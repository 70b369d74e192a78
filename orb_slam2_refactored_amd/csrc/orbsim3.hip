// orbsim3.hip — Optimizer::OptimizeSim3 on gfx950, batched over (keyframe 1, keyframe 2, S12) pairs.
//
// src/Optimizer.cc:944-1100: one VertexSim3Expmap, two fixed points and two binary edges
// (EdgeSim3ProjectXYZ, EdgeInverseSim3ProjectXYZ; types_seven_dof_expmap.h:130-171) per correspondence,
// g2o's Levenberg-Marquardt over the dense 7x7, optimize(5), a chi2 cut, optimize(5 or 10), a chi2 cut.
// The edges define no linearizeOplus, so the Jacobian is g2o's central difference at delta = 1e-9
// (base_binary_edge.hpp:143-200) and the iterates are defined by it: it is restated, not replaced.
//
// One wavefront owns one pair for the whole optimisation (one launch per batch, S3_WAVES pairs per block,
// no block barrier: the waves of a block never meet):
//   - the wave scans the pair's keyframe-1 slots 64 at a time and compacts the kept ones (ballot + mbcnt)
//     into a slot list in the workspace; correspondence c belongs to lane c & 63;
//   - the first S3_LDS_CORR correspondences are staged once into the wave's LDS slice (12 fp64 each: Xc1,
//     Xc2, both measurements, both Omega); a pair with more rebuilds the rest from the slot list per pass
//     with the same float expressions;
//   - per linearisation lane j < 14 builds the perturbed estimate Sim3(+-delta e_d) * S and its inverse
//     once and parks them in LDS, where the edge loop reads them at a wave-uniform address;
//   - H (28), b (7) and the robust chi2 are summed edge by edge in insertion order (e12 then e21 of
//     correspondence 0, 1, ...), one addition at a time, as g2o's loop over the active edges adds them: 64
//     correspondences at a time every lane builds its two edges' 36 terms, then the wave walks the active
//     lanes in order and every lane adds the v_readlane broadcast to its own copy of the totals.  A tree sum
//     is some 4x faster, but delta = 1e-9 magnifies its different rounding by 5e8 and, once LM has converged,
//     rho is rounding noise around 0 and decides accept, reject and the stop: the reference's iteration
//     counts are reproduced only with its order of additions;
//   - every lane runs the LM control, the packed 7x7 LDL^T and the Sim3 exp redundantly on wave-uniform
//     values, so the estimate stays in registers.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>

#include "common.h"
#include "se3.h"
#include "sim3_g2o.h"
#include "wave_sum.h"
#include "world_to_camera.h"

namespace orbamd {

constexpr int S3_WAVES = 4;                    // pairs per block
constexpr int S3_THREADS = 64 * S3_WAVES;
constexpr int S3_LDS_CORR = 128;               // staged correspondences per pair: 12 KiB per wave
constexpr int S3_MAX_CORR = ORBBA_SIM3_MAX_CORR;
constexpr int S3_MAX_LEVELS = 32;
static_assert(S3_MAX_CORR <= 64 * 128, "a lane's removed-edge mask is two u64");
static_assert(S3_LDS_CORR % 64 == 0, "");

struct S3Args {
    int n_pairs;
    const int32_t *kp1_begin, *kp2_begin;
    const float *kp1_xy, *kp2_xy;
    const int32_t *kp1_oct, *kp2_oct;
    const float *pose1, *pose2, *cam1, *cam2;
    const uint8_t *valid1, *valid2;
    const float *xw1, *xw2;
    const float* s12;
    const int32_t* match12;
    int n_levels;
    float isig2[S3_MAX_LEVELS];
    float max_chi2;
    int fix_scale;
    float* o_s12;
    double* o_g2o;
    int32_t* o_match12;
    int32_t* o_ninl;
    int32_t* o_iter;
    int32_t* slots;   // workspace, total_kp1: pair p's kept slots, compacted, at kp1_begin[p]
};

struct S3Corr { double X1[3], X2[3], z1[2], z2[2], w1, w2; };

struct S3Cam { double f1[2], c1[2], f2[2], c2[2]; };

// g2o::Sim3 itself (exp, *, inverse) is in sim3_g2o.h

// cam_map(project(S.map(X))) subtracted from z: computeError of either edge
// (types_seven_dof_expmap.h:74-88, :138-145, :160-167; se3_ops.hpp:49-55; sim3.h:144-146)
__device__ __forceinline__ void s3_error(const double* q, const double* t, double s, const double* X, const double* f,
                                         const double* c, const double* z, double* e) {
    double r[3];
    q_rotate(q, X, r);
    const double p0 = s * r[0] + t[0], p1 = s * r[1] + t[1], p2 = s * r[2] + t[2];
    e[0] = z[0] - ((p0 / p2) * f[0] + c[0]);
    e[1] = z[1] - ((p1 / p2) * f[1] + c[1]);
}

__device__ __forceinline__ double s3_chi2(const double* e, double w) { return e[0] * (w * e[0]) + e[1] * (w * e[1]); }

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:65-91)
__device__ __forceinline__ void s3_robustify(double delta, double c, double& r0, double& r1) {
    const double dsqr = delta * delta;
    if (c <= dsqr) { r0 = c; r1 = 1.0; }
    else { const double sq = sqrt(c); r0 = 2 * sq * delta - dsqr; r1 = delta / sq; }
}

// ---------------------------------------------------------------- the pair's correspondences
// writes of other lanes of this wavefront (LDS or the slot list) become readable
__device__ __forceinline__ void s3_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

struct S3Pair {
    int k1, k2;                 // first slot of either keyframe
    const float *P1, *P2;       // poses
    double* lds;                // this wave's 12 x S3_LDS_CORR
    int ncorr;
};

// The fixed points, measurements and information of the correspondence at keyframe-1 slot `slot`
// (Optimizer.cc:1006-1036); the camera-frame points in float, in the reference's expression order.
__device__ __forceinline__ void s3_make(const S3Args& a, const S3Pair& pr, int slot, S3Corr& d) {
    const size_t i = (size_t)pr.k1 + slot;
    const size_t j = (size_t)pr.k2 + a.match12[i];
    const float3 c1 = pj_world_to_camera(pr.P1, a.xw1[3 * i], a.xw1[3 * i + 1], a.xw1[3 * i + 2]);
    const float3 c2 = pj_world_to_camera(pr.P2, a.xw2[3 * j], a.xw2[3 * j + 1], a.xw2[3 * j + 2]);
    d.X1[0] = c1.x; d.X1[1] = c1.y; d.X1[2] = c1.z;
    d.X2[0] = c2.x; d.X2[1] = c2.y; d.X2[2] = c2.z;
    d.z1[0] = a.kp1_xy[2 * i]; d.z1[1] = a.kp1_xy[2 * i + 1];
    d.z2[0] = a.kp2_xy[2 * j]; d.z2[1] = a.kp2_xy[2 * j + 1];
    d.w1 = a.isig2[min(max(a.kp1_oct[i], 0), a.n_levels - 1)];
    d.w2 = a.isig2[min(max(a.kp2_oct[j], 0), a.n_levels - 1)];
}

__device__ __forceinline__ void s3_load(const S3Args& a, const S3Pair& pr, int c, S3Corr& d) {
    if (c < S3_LDS_CORR) {
        const double* L = pr.lds + c;
#pragma unroll
        for (int k = 0; k < 3; k++) { d.X1[k] = L[k * S3_LDS_CORR]; d.X2[k] = L[(3 + k) * S3_LDS_CORR]; }
#pragma unroll
        for (int k = 0; k < 2; k++) { d.z1[k] = L[(6 + k) * S3_LDS_CORR]; d.z2[k] = L[(8 + k) * S3_LDS_CORR]; }
        d.w1 = L[10 * S3_LDS_CORR];
        d.w2 = L[11 * S3_LDS_CORR];
    } else {
        s3_make(a, pr, a.slots[pr.k1 + c], d);
    }
}

// bit k of a lane's mask: its k-th correspondence (lane + 64 k) has been removed
struct S3Mask {
    uint64_t m[2];
    __device__ __forceinline__ bool get(int k) const { return ((k < 64 ? m[0] >> k : m[1] >> (k - 64)) & 1) != 0; }
    __device__ __forceinline__ void set(int k) { if (k < 64) m[0] |= 1ull << k; else m[1] |= 1ull << (k - 64); }
};

// H (packed upper, 28, row-major) | b (7) | robust chi2, wave-uniform in every lane
struct S3Sys { double v[36]; };

__host__ __device__ constexpr int pk7(int r, int c) { return r * 7 - r * (r - 1) / 2 + (c - r); }

// computeActiveErrors + linearizeOplus + constructQuadraticForm over the active edges at S:
// base_binary_edge.hpp:54-120 (the point vertex is fixed: only the Sim3 block) and :143-200.
__device__ __forceinline__ void s3_linearize(const S3Args& a, const S3Pair& pr, const S3Mask& dead, const S3Cam& cam,
                                             const S3& S, double* pert, double huber, int lane, S3Sys& sys) {
    const double delta = 1e-9, scalar = 1.0 / (2 * delta);
    S3 Si;
    s3_inverse(S, Si);
    if (lane < 14) {   // lane 2d: +delta along d, lane 2d + 1: -delta (oplusImpl: Sim3(update) * estimate)
        double u[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int d = 0; d < 7; d++)
            if ((lane >> 1) == d) u[d] = (lane & 1) ? -delta : delta;
        if (a.fix_scale) u[6] = 0;
        S3 U, P, Pi;
        s3_exp(u, U);
        s3_mul(U, S, P);
        s3_inverse(P, Pi);
        double* o = pert + 16 * lane;
#pragma unroll
        for (int k = 0; k < 4; k++) { o[k] = P.q[k]; o[8 + k] = Pi.q[k]; }
#pragma unroll
        for (int k = 0; k < 3; k++) { o[4 + k] = P.t[k]; o[12 + k] = Pi.t[k]; }
        o[7] = P.s;
        o[15] = Pi.s;
    }
    s3_wave_sync();
    double tot[36];   // H, b, chi2: wave-uniform running sums
#pragma unroll
    for (int j = 0; j < 36; j++) tot[j] = 0;
    for (int base = 0, k = 0; base < pr.ncorr; base += 64, k++) {
        const int c = base + lane;
        const bool on = c < pr.ncorr && !dead.get(k);
        double h[2][36];   // this lane's two edges: e12 then e21
#pragma unroll
        for (int j = 0; j < 36; j++) { h[0][j] = 0; h[1][j] = 0; }
        if (on) {
            S3Corr d;
            s3_load(a, pr, c, d);
            double e12[2], e21[2];
            s3_error(S.q, S.t, S.s, d.X2, cam.f1, cam.c1, d.z1, e12);
            s3_error(Si.q, Si.t, Si.s, d.X1, cam.f2, cam.c2, d.z2, e21);
            double J12[2][7], J21[2][7];
#pragma unroll 1
            for (int dd = 0; dd < 7; dd++) {
                asm volatile("" ::: "memory");   // the perturbed estimates are read here, per column: hoisted out
                                                 // of the loops they would hold 448 VGPRs
                const double* pp = pert + 32 * dd;
                const double* pm = pp + 16;
                double ep[2], em[2];
                s3_error(pp, pp + 4, pp[7], d.X2, cam.f1, cam.c1, d.z1, ep);
                s3_error(pm, pm + 4, pm[7], d.X2, cam.f1, cam.c1, d.z1, em);
                J12[0][dd] = scalar * (ep[0] - em[0]);
                J12[1][dd] = scalar * (ep[1] - em[1]);
                s3_error(pp + 8, pp + 12, pp[15], d.X1, cam.f2, cam.c2, d.z2, ep);
                s3_error(pm + 8, pm + 12, pm[15], d.X1, cam.f2, cam.c2, d.z2, em);
                J21[0][dd] = scalar * (ep[0] - em[0]);
                J21[1][dd] = scalar * (ep[1] - em[1]);
            }
#pragma unroll
            for (int edge = 0; edge < 2; edge++) {
                const double* e = edge ? e21 : e12;
                const double om = edge ? d.w2 : d.w1;
                const double (&J)[2][7] = edge ? J21 : J12;
                double r0, r1;
                s3_robustify(huber, s3_chi2(e, om), r0, r1);
                h[edge][35] = r0;
                const double or0 = r1 * -(om * e[0]), or1 = r1 * -(om * e[1]);   // omega_r = -Omega e, *= rho'
                const double w = r1 * om;                                         // weightedOmega
                int n = 0;
#pragma unroll
                for (int r = 0; r < 7; r++) {
                    h[edge][28 + r] = J[0][r] * or0 + J[1][r] * or1;
#pragma unroll
                    for (int cc = r; cc < 7; cc++, n++) h[edge][n] = J[0][r] * w * J[0][cc] + J[1][r] * w * J[1][cc];
                }
            }
        }
        // the edges in insertion order, one addition at a time, as g2o's loop over the active edges adds them
        for (uint64_t m = __ballot(on); m; m &= m - 1) {
            const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
#pragma unroll
            for (int edge = 0; edge < 2; edge++)
#pragma unroll
                for (int j = 0; j < 36; j++) tot[j] += po_readlane(h[edge][j], l);
        }
    }
#pragma unroll
    for (int j = 0; j < 36; j++) sys.v[j] = tot[j];
    s3_wave_sync();   // the next linearisation overwrites pert
}

// computeActiveErrors + activeRobustChi2 at S
__device__ __forceinline__ double s3_chi_pass(const S3Args& a, const S3Pair& pr, const S3Mask& dead, const S3Cam& cam,
                                              const S3& S, double huber, int lane) {
    S3 Si;
    s3_inverse(S, Si);
    double sum = 0;
    for (int base = 0, k = 0; base < pr.ncorr; base += 64, k++) {
        const int c = base + lane;
        const bool on = c < pr.ncorr && !dead.get(k);
        double r12 = 0, r21 = 0;
        if (on) {
            S3Corr d;
            s3_load(a, pr, c, d);
            double e12[2], e21[2], r1;
            s3_error(S.q, S.t, S.s, d.X2, cam.f1, cam.c1, d.z1, e12);
            s3_error(Si.q, Si.t, Si.s, d.X1, cam.f2, cam.c2, d.z2, e21);
            s3_robustify(huber, s3_chi2(e12, d.w1), r12, r1);
            s3_robustify(huber, s3_chi2(e21, d.w2), r21, r1);
        }
        for (uint64_t m = __ballot(on); m; m &= m - 1) {   // in insertion order, as s3_linearize
            const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(m));
            sum += po_readlane(r12, l);
            sum += po_readlane(r21, l);
        }
    }
    return sum;
}

// LinearSolverDense (linear_solver_dense.h:65-113): LDL^T of H + lambda I in place on the packed triangle
// (L(i,j) overwrites H(j,i), D the diagonal), unpivoted as in orbpo.hip; a negative pivot fails the solve.
__device__ __forceinline__ bool s3_solve(const S3Sys& S, double lambda, double (&x)[7]) {
    double A[28];
#pragma unroll
    for (int k = 0; k < 28; k++) A[k] = S.v[k];
#pragma unroll
    for (int i = 0; i < 7; i++) A[pk7(i, i)] += lambda;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double v = A[pk7(j, j)];
#pragma unroll
        for (int k = 0; k < j; k++) v -= A[pk7(k, j)] * A[pk7(k, j)] * A[pk7(k, k)];
        ok = ok && (v >= 0) && isfinite(v);
        A[pk7(j, j)] = v;
#pragma unroll
        for (int i = j + 1; i < 7; i++) {
            double s = A[pk7(j, i)];
#pragma unroll
            for (int k = 0; k < j; k++) s -= A[pk7(k, i)] * A[pk7(k, j)] * A[pk7(k, k)];
            A[pk7(j, i)] = v != 0 ? s / v : 0;
        }
    }
    double y[7];
#pragma unroll
    for (int i = 0; i < 7; i++) {
        double s = S.v[28 + i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= A[pk7(k, i)] * y[k];
        y[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 7; i++) y[i] = A[pk7(i, i)] != 0 ? y[i] / A[pk7(i, i)] : 0;
#pragma unroll
    for (int i = 6; i >= 0; i--) {
        double s = y[i];
#pragma unroll
        for (int k = i + 1; k < 7; k++) s -= A[pk7(i, k)] * x[k];
        x[i] = s;
    }
    if (!ok)
#pragma unroll
        for (int i = 0; i < 7; i++) x[i] = 0;
    return ok;
}

__global__ __launch_bounds__(S3_THREADS) void optimize_sim3_kernel(S3Args a) {
    __shared__ double s3_edges[S3_WAVES][12 * S3_LDS_CORR];
    __shared__ double s3_pert[S3_WAVES][14 * 16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int p = blockIdx.x * S3_WAVES + w;
    if (p >= a.n_pairs) return;   // wave-uniform; no block barrier anywhere below
    S3Pair pr;
    pr.k1 = a.kp1_begin[p];
    pr.k2 = a.kp2_begin[p];
    pr.P1 = a.pose1 + 12 * (size_t)p;
    pr.P2 = a.pose2 + 12 * (size_t)p;
    pr.lds = s3_edges[w];
    const int n1 = a.kp1_begin[p + 1] - pr.k1, n2 = a.kp2_begin[p + 1] - pr.k2;
    // the kept slots in ascending order (Optimizer.cc:991-1001); the output matches start as the input's
    int ncorr = 0;
    for (int base = 0; base < n1; base += 64) {
        const int i = base + lane;
        bool keep = false;
        if (i < n1) {
            const int m = a.match12[pr.k1 + i];
            if (a.o_match12 != a.match12) a.o_match12[pr.k1 + i] = m;
            keep = a.valid1[pr.k1 + i] && m >= 0 && m < n2 && a.valid2[pr.k2 + m];
        }
        const uint64_t bal = __ballot(keep);
        if (keep) {
            const int pos = ncorr + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0));
            a.slots[pr.k1 + pos] = i;   // pos < n1
        }
        ncorr += __popcll(bal);
    }
    pr.ncorr = ncorr;
    const float* S0 = a.s12 + 13 * (size_t)p;
    S3 est;   // ToG2OSim3 (Optimizer.cc:183-188)
    {
        double Rm[9];
#pragma unroll
        for (int i = 0; i < 9; i++) Rm[i] = S0[i];
        const Q4 qq = q_from_R(Rm);
        est.q[0] = qq.x; est.q[1] = qq.y; est.q[2] = qq.z; est.q[3] = qq.w;
        est.t[0] = S0[9]; est.t[1] = S0[10]; est.t[2] = S0[11];
        est.s = S0[12];
    }
    int iters[2] = {0, 0};
    int result = 0;
    bool keep_input = true;
    if (ncorr > S3_MAX_CORR) {
        result = -1;
    } else if (ncorr > 0) {
        s3_wave_sync();   // the slot list
        for (int c = lane; c < min(ncorr, S3_LDS_CORR); c += 64) {
            S3Corr d;
            s3_make(a, pr, a.slots[pr.k1 + c], d);
            double* L = pr.lds + c;
#pragma unroll
            for (int k = 0; k < 3; k++) { L[k * S3_LDS_CORR] = d.X1[k]; L[(3 + k) * S3_LDS_CORR] = d.X2[k]; }
#pragma unroll
            for (int k = 0; k < 2; k++) { L[(6 + k) * S3_LDS_CORR] = d.z1[k]; L[(8 + k) * S3_LDS_CORR] = d.z2[k]; }
            L[10 * S3_LDS_CORR] = d.w1;
            L[11 * S3_LDS_CORR] = d.w2;
        }
        s3_wave_sync();
        const float* K1 = a.cam1 + 4 * (size_t)p;
        const float* K2 = a.cam2 + 4 * (size_t)p;
        const S3Cam cam{{K1[0], K1[1]}, {K1[2], K1[3]}, {K2[0], K2[1]}, {K2[2], K2[3]}};
        const double max_chi2 = a.max_chi2, huber = sqrt((double)a.max_chi2);
        S3Mask dead{{0, 0}};
        int nbad = 0;
        for (int round = 0; round < 2; round++) {   // Optimizer.cc:1046-1047, :1073-1076
            const int max_it = round == 0 ? 5 : (nbad > 0 ? 10 : 5);
            S3 Se = est;   // the estimate of the last computeActiveErrors
            double lambda = 0, ni = 2;
            int lm_bad = 0;
            for (int it = 0; it < max_it; it++) {   // optimization_algorithm_levenberg.cpp:61-164
                iters[round]++;
                S3Sys sys;
                s3_linearize(a, pr, dead, cam, est, s3_pert[w], huber, lane, sys);
                Se = est;
                double cur = sys.v[35];
                const double ini = cur;
                if (it == 0) {   // computeLambdaInit, tau = 1e-5
                    double m = 0;
#pragma unroll
                    for (int j = 0; j < 7; j++) m = fmax(m, fabs(sys.v[pk7(j, j)]));
                    lambda = 1e-5 * m; ni = 2; lm_bad = 0;
                }
                double rho = 0;
                int qn = 0;
                do {
                    const S3 saved = est;
                    double x[7];
                    const bool ok = s3_solve(sys, lambda, x);
                    if (a.fix_scale) x[6] = 0;   // oplusImpl
                    S3 U, N;
                    s3_exp(x, U);
                    s3_mul(U, est, N);
                    est = N;
                    double tmp = s3_chi_pass(a, pr, dead, cam, est, huber, lane);
                    Se = est;
                    if (!ok) tmp = DBL_MAX;
                    rho = cur - tmp;
                    double sc = 0;   // computeScale
#pragma unroll
                    for (int j = 0; j < 7; j++) sc += x[j] * (lambda * x[j] + sys.v[28 + j]);
                    rho /= sc + 1e-3;
                    if (rho > 0 && isfinite(tmp)) {
                        const double u = 2 * rho - 1;
                        double alpha = 1. - u * u * u;
                        alpha = fmin(alpha, 2. / 3.);
                        lambda *= fmax(1. / 3., alpha);
                        ni = 2;
                        cur = tmp;
                    } else {
                        lambda *= ni;
                        ni *= 2;
                        est = saved;
                    }
                    qn++;
                } while (rho < 0 && qn < 10);
                if (qn == 10 || rho == 0) break;
                if ((ini - cur) * 1e3 < ini) lm_bad++; else lm_bad = 0;
                if (lm_bad >= 3) break;
            }
            // :1049-1068 / :1078-1094: chi2() of the last computed error, nothing recomputed
            S3 Sei;
            s3_inverse(Se, Sei);
            int cnt = 0, k = 0;
            for (int c = lane; c < ncorr; c += 64, k++) {
                if (dead.get(k)) continue;
                S3Corr d;
                s3_load(a, pr, c, d);
                double e12[2], e21[2];
                s3_error(Se.q, Se.t, Se.s, d.X2, cam.f1, cam.c1, d.z1, e12);
                s3_error(Sei.q, Sei.t, Sei.s, d.X1, cam.f2, cam.c2, d.z2, e21);
                if (s3_chi2(e12, d.w1) > max_chi2 || s3_chi2(e21, d.w2) > max_chi2) {
                    a.o_match12[pr.k1 + a.slots[pr.k1 + c]] = -1;
                    dead.set(k);
                    cnt++;
                }
            }
            const int removed = (int)po_wave_sum((double)cnt, lane);
            if (round == 0) {
                nbad = removed;
                if (ncorr - nbad < 10) break;   // return 0: S12 unchanged, the removed matches stay removed
            } else {
                result = ncorr - nbad - removed;
                keep_input = false;
            }
        }
    }
    if (lane < 13) {
        float v = S0[lane];
        if (!keep_input) {   // FromG2OSim3 (Optimizer.cc:190-195)
            double R[9];
            q_to_R(est.q, R);
            double o = est.s;
#pragma unroll
            for (int i = 0; i < 9; i++) if (lane == i) o = R[i];
#pragma unroll
            for (int i = 0; i < 3; i++) if (lane == 9 + i) o = est.t[i];
            v = (float)o;
        }
        a.o_s12[13 * (size_t)p + lane] = v;
    }
    if (a.o_g2o && lane < 8) {
        double o = est.s;
#pragma unroll
        for (int i = 0; i < 4; i++) if (lane == i) o = est.q[i];
#pragma unroll
        for (int i = 0; i < 3; i++) if (lane == 4 + i) o = est.t[i];
        a.o_g2o[8 * (size_t)p + lane] = o;
    }
    if (lane == 0) {
        a.o_ninl[p] = result;
        if (a.o_iter) { a.o_iter[2 * p] = iters[0]; a.o_iter[2 * p + 1] = iters[1]; }
    }
}

thread_local Scratch g_s3;

}  // namespace orbamd

using namespace orbamd;

// The checks both entries share, and the kernel's arguments but for the workspace.
static int s3_common(const orbba_sim3_batch* in, const orbba_sim3_result* out, S3Args& a) {
    ORB_CHECK_ARG(in && out, "null argument");
    ORB_CHECK_ARG(in->n_pairs >= 0 && in->total_kp1 >= 0 && in->total_kp2 >= 0, "negative sizes");
    ORB_CHECK_ARG(in->n_levels >= 1 && in->n_levels <= S3_MAX_LEVELS && in->inv_level_sigma2, "bad scale pyramid");
    if (in->n_pairs == 0) return ORB_OK;
    ORB_CHECK_ARG(in->kp1_begin && in->kp2_begin && in->pose1 && in->pose2 && in->camera1 && in->camera2 && in->s12,
                  "null array");
    ORB_CHECK_ARG(in->total_kp1 == 0 || (in->kp1_xy && in->kp1_octave && in->mp1_valid && in->mp1_xw && in->match12),
                  "null keyframe 1 array");
    ORB_CHECK_ARG(in->total_kp2 == 0 || (in->kp2_xy && in->kp2_octave && in->mp2_valid && in->mp2_xw),
                  "null keyframe 2 array");
    ORB_CHECK_ARG(out->s12 && out->n_inliers && (in->total_kp1 == 0 || out->match12), "null output array");
    std::memset(&a, 0, sizeof(a));
    a.n_pairs = in->n_pairs;
    a.kp1_begin = in->kp1_begin; a.kp2_begin = in->kp2_begin;
    a.kp1_xy = in->kp1_xy; a.kp2_xy = in->kp2_xy;
    a.kp1_oct = in->kp1_octave; a.kp2_oct = in->kp2_octave;
    a.pose1 = in->pose1; a.pose2 = in->pose2; a.cam1 = in->camera1; a.cam2 = in->camera2;
    a.valid1 = in->mp1_valid; a.valid2 = in->mp2_valid;
    a.xw1 = in->mp1_xw; a.xw2 = in->mp2_xw;
    a.s12 = in->s12;
    a.match12 = in->match12;
    a.n_levels = in->n_levels;
    for (int l = 0; l < in->n_levels; l++) a.isig2[l] = in->inv_level_sigma2[l];
    a.max_chi2 = in->max_chi2;
    a.fix_scale = in->fix_scale != 0;
    a.o_s12 = out->s12; a.o_g2o = out->s12_g2o; a.o_match12 = out->match12; a.o_ninl = out->n_inliers;
    a.o_iter = out->iterations;
    return ORB_OK;
}

extern "C" int orbba_optimize_sim3_device(const orbba_sim3_batch* in, orbba_sim3_result* out, void* stream) {
    S3Args a;
    int rc;
    if ((rc = s3_common(in, out, a))) return rc;
    if (in->n_pairs == 0) return ORB_OK;
    if ((rc = g_s3.use_current_device())) return rc;
    if ((rc = g_s3.ws.reserve(std::max<size_t>(in->total_kp1, 1) * sizeof(int32_t)))) return rc;
    a.slots = g_s3.ws.as<int32_t>();
    hipLaunchKernelGGL(optimize_sim3_kernel, dim3((a.n_pairs + S3_WAVES - 1) / S3_WAVES), dim3(S3_THREADS), 0,
                       (hipStream_t)stream, a);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbba_optimize_sim3(const orbba_sim3_batch* in, orbba_sim3_result* out, int device) {
    S3Args a;
    int rc;
    if ((rc = s3_common(in, out, a))) return rc;   // the checks, before any copy
    const size_t F = in->n_pairs, K1 = in->total_kp1, K2 = in->total_kp2;
    if (F == 0) return ORB_OK;
    const int32_t *b1 = in->kp1_begin, *b2 = in->kp2_begin;
    ORB_CHECK_ARG(b1[0] == 0 && b2[0] == 0 && b1[F] == in->total_kp1 && b2[F] == in->total_kp2,
                  "kp1_begin / kp2_begin must start at 0 and end at total_kp1 / total_kp2");
    for (size_t p = 0; p < F; p++) {
        ORB_CHECK_ARG(b1[p + 1] >= b1[p] && b2[p + 1] >= b2[p], "offsets must be non-decreasing");
        const int n2 = b2[p + 1] - b2[p];
        int ncorr = 0;
        for (int i = b1[p]; i < b1[p + 1]; i++) {
            const int m = in->match12[i];
            ORB_CHECK_ARG(m >= -1 && m < n2, "match12 must be -1 or an index into keyframe 2 of its pair");
            ORB_CHECK_ARG(in->kp1_octave[i] >= 0 && in->kp1_octave[i] < in->n_levels, "kp1_octave out of range");
            ncorr += in->mp1_valid[i] && m >= 0 && in->mp2_valid[b2[p] + m];
        }
        ORB_CHECK_ARG(ncorr <= S3_MAX_CORR, "pair has more than ORBBA_SIM3_MAX_CORR correspondences");
    }
    for (size_t j = 0; j < K2; j++)
        ORB_CHECK_ARG(in->kp2_octave[j] >= 0 && in->kp2_octave[j] < in->n_levels, "kp2_octave out of range");
    orbba_sim3_batch d = *in;
    orbba_sim3_result r = *out;
    Mirror io;
    io.add(d.kp1_begin, F + 1, true, false); io.add(d.kp2_begin, F + 1, true, false);
    io.add(d.kp1_xy, K1 * 2, true, false); io.add(d.kp2_xy, K2 * 2, true, false);
    io.add(d.kp1_octave, K1, true, false); io.add(d.kp2_octave, K2, true, false);
    io.add(d.pose1, F * 12, true, false); io.add(d.pose2, F * 12, true, false);
    io.add(d.camera1, F * 4, true, false); io.add(d.camera2, F * 4, true, false);
    io.add(d.mp1_valid, K1, true, false); io.add(d.mp2_valid, K2, true, false);
    io.add(d.mp1_xw, K1 * 3, true, false); io.add(d.mp2_xw, K2 * 3, true, false);
    io.add(d.s12, F * 13, true, false); io.add(d.match12, K1, true, false);
    io.add(r.s12, F * 13, false, true); io.add(r.s12_g2o, F * 8, false, true); io.add(r.match12, K1, false, true);
    io.add(r.n_inliers, F, false, true); io.add(r.iterations, F * 2, false, true);
    return run_host(g_s3, device, io, [&] { return orbba_optimize_sim3_device(&d, &r, nullptr); });
}
