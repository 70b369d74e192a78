// LocalBA on the device (orbba.hip): the control block, the problem as the kernels see it, and the
// helpers more than one stage uses.
#pragma once

#include "common.h"
#include "se3.h"

namespace orbamd {

struct BACtl {
    double lambda, ni, cur, ini, tmp, scale, rho;
    int ok2, accepted;
    double maxdiag;
    unsigned long long maxdiag_bits;   // computeLambdaInit's max |diag H| as the bits of a double >= 0
    // LM loop state, advanced on the device by ba_decide_step (g2o SparseOptimizer::optimize +
    // OptimizationAlgorithmLevenberg::solve): iteration, trial within it, nBad, flags
    int it, q, nbad, done, need_lin, iters_max, iters_done;
    int trials;    // LM trials since the start of the LocalBA call (both optimize() calls; test hook)
    int stopped;   // the force-stop flag ended the loop
    int seq;       // host snapshot sequence id (written last; see ba_decide_step)
    int n_active;  // level-0 edges after the outlier classification between the optimize() calls
    int pad_;
    double chi_out;
};

// Every kernel of an LM step returns at once when the loop has finished (steps are enqueued ahead
// of the host learning that); the linearisation kernels also skip on a retry trial.
#define BA_RETURN_IF_DONE(b) \
    do {                     \
        if ((b).ctl->done) return; \
    } while (0)

// ------------------------------------------------------------------ problem on the device
struct BADev {
    int P, N, E;
    double* q;      // P x 4
    double* t;      // P x 3
    double* q_sv;   // push/pop copies
    double* t_sv;
    double* X;      // N x 3
    double* X_sv;
    const uint8_t* fixed;
    const int* ep;
    const int* ek;
    const uint8_t* stereo;
    int cam_step;         // 5: a camera per edge; 0: one camera for every edge (uploaded once)
    const double* obs;    // E x 3
    const double* info;   // E
    const double* cam;    // E x 5
    uint8_t* robust;      // E
    double* err;          // E x 3 (last computed error, g2o's _error)
    const uint8_t* level; // E: g2o edge level; only level-0 edges take part (initializeOptimization(0))
    // active structure
    int Ea, np, nl, nblk;
    const int* act;       // Ea: edge id per active slot (ascending edge id)
    const int* hp;        // P: hessian index or -1
    const int* hl;        // N: point index or -1
    const int* pt_beg;    // nl+1: CSR of active slots per active point (slot order)
    const int* pt_slot;
    int4* pt_rec;         // Ea, per point-list entry u: {k = pt_slot[u], e = act[k], pose ek[e], hp[ek[e]]}
    const int* pt_id;     // nl: point id of point index
    const int* ps_beg;    // np+1: CSR of active slots per free pose
    const int* ps_slot;
    const int* ps_id;     // np: pose id
    const int* blk_i1;    // nblk
    const int* blk_i2;
    const int* blk_beg;   // nblk+1: CSR of (slot1, slot2) pairs
    const int2* blk_pair;
    // per active slot products
    double* J;            // Ea x 72: Hll(9) bl(3) Hpp(36) bp(6) Hpl(18, pose-major 6x3)
    double* W;            // Ea x 24: W = Hpl Dinv (18) | Hpl Dinv b_l (6)
    // per point / pose system
    double* Hll;          // nl x 9
    double* bl;           // nl x 3
    double* Dinv;         // nl x 9
    double* Hpp;          // np x 36
    double* bp;           // np x 6
    double* S;            // D x D reduced system
    double* Sg;           // Dp x (Dp+1) padded working copy for the global-memory solve (D > 128), else null
    double* bs;           // D
    double* x;            // D + 3 nl
    double* rchi;         // Ea: robust chi2 per active slot
    double* part;         // scale partials: nl + np
    double* Spart;         // the Schur-block parts' partial blocks (+ Hpp): (SB_SPLIT + 1) x nblk x 36 for the
                           // global solve, (SB_SPLIT + 1) row-major D x D matrices (both orientations) for the LDS solve
    unsigned* blk_done;    // nblk: parts of the block finished (the last one forms S)
    const int* blk_diag;   // np: block index of the diagonal block (i, i)
    BACtl* ctl;
    const int32_t* stop;   // device view of the host's force-stop flag (mapped pinned mirror), or null
    int stop_after;        // test hook: stop once this many trials have run (-1: off)
};

__device__ __forceinline__ double edge_chi2(const BADev& b, int e) {
    const int d = b.stereo[e] ? 3 : 2;
    double s = 0;
    for (int i = 0; i < d; i++) s += b.err[3 * e + i] * b.info[e] * b.err[3 * e + i];
    return s;
}
__device__ __forceinline__ void robustify(const BADev& b, int e, double chi, double& r0, double& r1) {
    if (!b.robust[e]) { r0 = chi; r1 = 1.0; return; }
    const double delta = b.stereo[e] ? sqrt(7.815) : sqrt(5.991);   // Optimizer.cc:44-47
    const double dsqr = delta * delta;
    if (chi <= dsqr) { r0 = chi; r1 = 1.0; }
    else { const double s = sqrt(chi); r0 = 2 * s * delta - dsqr; r1 = delta / s; }   // robust_kernel_impl.cpp:78-91
}

// EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ::computeError (types_six_dof_expmap.h:90-95,122-127)
// for edge e with camera-frame point Xc; stores g2o's _error and returns the robust chi2 term.
__device__ __forceinline__ double edge_error(const BADev& b, int e, const double* Xc) {
    const double* c = b.cam + b.cam_step * e;
    const double* z = b.obs + 3 * e;
    if (!b.stereo[e]) {
        b.err[3 * e + 0] = z[0] - (Xc[0] / Xc[2] * c[0] + c[2]);
        b.err[3 * e + 1] = z[1] - (Xc[1] / Xc[2] * c[1] + c[3]);
        b.err[3 * e + 2] = 0;
    } else {   // cam_project(..., bf): invz narrowed to float, bf*invz in float (.cpp:148-156)
        const float invz = 1.0f / Xc[2];
        const float bf = (float)c[4];
        const double u = Xc[0] * invz * c[0] + c[2];
        const double v = Xc[1] * invz * c[1] + c[3];
        b.err[3 * e + 0] = z[0] - u;
        b.err[3 * e + 1] = z[1] - v;
        b.err[3 * e + 2] = z[2] - (u - (double)(bf * invz));
    }
    double r0, r1;
    robustify(b, e, edge_chi2(b, e), r0, r1);
    return r0;
}

// fixed-order sum over the 8-lane group of a point
__device__ __forceinline__ double grp_sum(double v) {
    v += __shfl_xor(v, 1, 64);
    v += __shfl_xor(v, 2, 64);
    v += __shfl_xor(v, 4, 64);
    return v;
}

constexpr int GRP = 8;   // lanes per point

// parts a block's pair list is split into (ba_schur_block_kernel, orbba_schur.h; s_piece sums them)
#ifndef SB_SPLIT_DEF
#define SB_SPLIT_DEF 2
#endif
constexpr int SB_SPLIT = SB_SPLIT_DEF;

__device__ __forceinline__ bool inv3(const double* m, double* o) {
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
    if (det == 0) return false;
    const double id = 1.0 / det;
    o[0] = c00 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = c01 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = c02 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
    return true;
}

// Deterministic single-workgroup sum (fixed strided order + fixed tree).
__device__ double block_sum_1024(const double* v, int n, double* sh) {
    double s = 0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += v[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

constexpr int PA_SLOTS = 4096;   // a pose's edge-slot list staged in LDS when it has at most this many
__device__ __forceinline__ void stage_pose_slots(const BADev& b, int i, int* sslot) {
    const int beg = b.ps_beg[i], n = b.ps_beg[i + 1] - beg;
    if (n <= PA_SLOTS)
        for (int u = threadIdx.x; u < n; u += blockDim.x) sslot[u] = b.ps_slot[beg + u];
}

__device__ __forceinline__ void chi_total(const BADev& b, double* sh) {
    const double c = block_sum_1024(b.rchi, b.nl, sh);
    if (threadIdx.x == 0) {
        b.ctl->cur = c;
        b.ctl->ini = c;
    }
}

}  // namespace orbamd
