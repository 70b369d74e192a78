// orbeg.hip — Optimizer::OptimizeEssentialGraph on gfx950 (src/Optimizer.cc:743-942): the pose graph of every
// keyframe of the map after a loop closure, 7-DoF vertices, EdgeSim3 edges with g2o's numeric Jacobians, Levenberg
// over the dense system of the active free vertices (BlockSolver_7_3 with nothing marginalised: no Schur step),
// then the float pose recovery and map point correction.  include/orbslam2_amd.h states the contract.
//
// Everything is enqueued on one stream; the Levenberg control runs on the device, so the host enqueues the whole
// schedule (20 iterations x 10 trials) and every kernel of a step that is not taken returns at once:
//   eg_setup_kernel      one workgroup: edge validity, the per-vertex edge lists (CSR, edge order), the free-vertex
//                        numbering, ToG2OSim3 of the vertex table
//   eg_measure_kernel    one lane per edge: Sji in float (eg_edge.h), Quaterniond(R) in double
//   eg_linearize_kernel  32 lanes per edge: lane 2k + s (k = 7 a + d) evaluates the error with vertex a moved by
//                        +-delta along d, lane 28 the error itself; the pairs meet through one DPP exchange and
//                        write the Jacobian column; latency-bound (exp, log, acos, sincos chains in fp64)
//   eg_assemble_kernel   one workgroup per vertex, one thread per entry of its 7 x 7 row blocks and of b: the
//                        vertex's edges in insertion order, J^T J summed k ascending, no atomics (a row block is
//                        written by its vertex alone)
//   eg_begin_kernel      one wavefront: chi2 summed edge by edge in order, the iteration's Levenberg state
//   eg_stage_kernel      H + lambda I into the padded factorisation buffer (bandwidth-bound, 8 D^2 bytes each way)
//   eg_solve_kernel      one workgroup: ldlt_hbm_solve of ldlt_blocked.h (blocked LDL^T in HBM / L2, fp64 MFMA);
//                        ~D^3 / 3 flops on one CU, the bound of a large map
//   eg_update_kernel     one lane per vertex: push (a saved copy) and oplus
//   eg_chi_kernel        one lane per edge: the error at the trial estimate
//   eg_ctl_kernel        one wavefront: chi2 and g2o's computeScale summed in order, rho, accept or pop, lambda, the
//                        ten-trial, rho == 0 and nBad endings
//   eg_recover_kernel    lanes over keyframes then points: FromG2OSim3, Inverse, the 1 / s scaling in double, Map
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "eg_edge.h"
#include "eg_graph.h"
#include "ldlt_blocked.h"
#include "wave_sum.h"

namespace orbamd {

constexpr int EG_MAX_KF = ORBBA_EG_MAX_KEYFRAMES;
constexpr int EG_ITERS = 20, EG_TRIALS = 10;
static_assert(EG_ITERS * EG_TRIALS == ORBBA_EG_MAX_TRIALS, "");
static_assert(EG_MAX_KF <= 1024, "eg_setup_kernel: a thread per vertex in one workgroup");

struct EGCtl {
    int done, trial_on, iter, qn, ntrial, nfree, D, ok, nbad;
    double lambda, ni, cur, ini, rho;
};

struct EGDev {
    int V, E, N, fixed, fix_scale;
    const float *vs, *es;
    const int32_t *ei, *ej;
    const uint8_t* et;
    const float* pts;
    const int32_t* pref;
    // workspace
    EGCtl* ctl;
    double *est, *est_sv;    // V x 8: q, t, s
    double* meas;            // E x 8
    double* J;               // E x 2 x 49: vertex a, error row k, dof d
    double *err, *chi, *chi_t;   // E x 7, E, E
    double *H, *b, *x, *Sg;  // D x D, D, D, Dp x (Dp + 1)
    int32_t *vmap, *vbeg, *vlist;   // V, V + 1, 2 E (2 e + end)
    uint8_t* eok;            // E
    // results
    double* o_g2o;
    float *o_pose, *o_pts;
    double* o_meas;
    int32_t* o_iter;
    double* o_chi2;
    uint8_t* o_acc;
};

__device__ __forceinline__ void eg_load(const double* p, S3& s) {
#pragma unroll
    for (int k = 0; k < 4; k++) s.q[k] = p[k];
#pragma unroll
    for (int k = 0; k < 3; k++) s.t[k] = p[4 + k];
    s.s = p[7];
}
__device__ __forceinline__ void eg_store(double* p, const S3& s) {
#pragma unroll
    for (int k = 0; k < 4; k++) p[k] = s.q[k];
#pragma unroll
    for (int k = 0; k < 3; k++) p[4 + k] = s.t[k];
    p[7] = s.s;
}

// sum of v[0 .. n) one addition at a time in index order, wave-uniform (g2o's loops over the active edges and
// over x); one wavefront
template <class F>
__device__ __forceinline__ double eg_seq_sum(int n, int lane, F value) {
    double tot = 0;
    for (int base = 0; base < n; base += 64) {
        const double v = base + lane < n ? value(base + lane) : 0.0;
#pragma unroll
        for (int l = 0; l < 64; l++) tot += po_readlane(v, l);   // + 0.0 past the end changes nothing
    }
    return tot;
}

__global__ __launch_bounds__(1024) void eg_setup_kernel(EGDev g) {
    __shared__ int s_deg[EG_MAX_KF];
    const int tid = threadIdx.x;
    for (int e = tid; e < g.E; e += blockDim.x) {
        const int i = g.ei[e], j = g.ej[e];
        g.eok[e] = i >= 0 && i < g.V && j >= 0 && j < g.V && i != j;
    }
    for (int k = tid; k < ORBBA_EG_MAX_TRIALS; k += blockDim.x) g.o_acc[k] = 0;
    __syncthreads();
    if (tid < g.V) {
        int deg = 0;
        for (int e = 0; e < g.E; e++) deg += g.eok[e] && (g.ei[e] == tid || g.ej[e] == tid);
        s_deg[tid] = deg;
        F3 f;
        S3 s;
        f3_load(g.vs + 13 * tid, f);
        f3_to_g2o(f, s);
        eg_store(g.est + 8 * tid, s);
    }
    __syncthreads();
    if (tid == 0) {
        int pos = 0, nf = 0;
        for (int v = 0; v < g.V; v++) {   // a vertex with no edge is never activated
            g.vbeg[v] = pos;
            pos += s_deg[v];
            g.vmap[v] = s_deg[v] > 0 && v != g.fixed ? nf++ : -1;
        }
        g.vbeg[g.V] = pos;
        EGCtl c;
        memset(&c, 0, sizeof(c));
        c.nfree = nf;
        c.D = 7 * nf;
        *g.ctl = c;
    }
    __syncthreads();
    if (tid < g.V) {
        int pos = g.vbeg[tid];   // at most vbeg[tid] + s_deg[tid] <= 2 E entries
        for (int e = 0; e < g.E; e++) {
            if (!g.eok[e]) continue;
            if (g.ei[e] == tid) g.vlist[pos++] = 2 * e;
            else if (g.ej[e] == tid) g.vlist[pos++] = 2 * e + 1;
        }
    }
}

__global__ __launch_bounds__(64) void eg_measure_kernel(EGDev g) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= g.E) return;
    S3 m;
    memset(&m, 0, sizeof(m));
    if (g.eok[e]) {
        const float* tb = g.et[e] ? g.es : g.vs;
        eg_measurement(tb + 13 * (size_t)g.ei[e], tb + 13 * (size_t)g.ej[e], m);
    }
    eg_store(g.meas + 8 * (size_t)e, m);
    if (g.o_meas) eg_store(g.o_meas + 8 * (size_t)e, m);
}

constexpr int EG_LIN_EDGES = 8;   // edges per 256-thread workgroup, 32 lanes each

// computeActiveErrors + linearizeOplus (base_binary_edge.hpp:131-205) of every edge at the estimates
__global__ __launch_bounds__(32 * EG_LIN_EDGES) void eg_linearize_kernel(EGDev g) {
    if (g.ctl->done) return;
    const int e = blockIdx.x * EG_LIN_EDGES + (threadIdx.x >> 5), l = threadIdx.x & 31;
    const bool in = e < g.E;
    const bool valid = in && g.eok[e];
    const int a = l >= 14 && l < 28 ? 1 : 0, d = (l % 14) >> 1;
    double er[7] = {0, 0, 0, 0, 0, 0, 0};
    if (valid) {
        S3 C, v1, v2;
        eg_load(g.meas + 8 * (size_t)e, C);
        eg_load(g.est + 8 * (size_t)g.ei[e], v1);
        eg_load(g.est + 8 * (size_t)g.ej[e], v2);
        if (l < 28) {
            const double delta = 1e-9;
            double u[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int k = 0; k < 7; k++)
                if (k == d) u[k] = (l & 1) ? -delta : delta;
            S3 P;
            eg_oplus(u, g.fix_scale, a ? v2 : v1, P);
            if (a) v2 = P; else v1 = P;
        }
        eg_error(C, v1, v2, er);
    }
    const double scalar = 1.0 / (2 * 1e-9);
#pragma unroll
    for (int r = 0; r < 7; r++) {   // every lane of the wavefront takes part in the exchange
        const double other = __shfl_xor(er[r], 1);
        if (in && l < 28 && !(l & 1)) g.J[(size_t)e * 98 + a * 49 + r * 7 + d] = valid ? scalar * (er[r] - other) : 0.0;
    }
    if (in && l == 28) {
        double c = 0;
#pragma unroll
        for (int r = 0; r < 7; r++) {
            g.err[(size_t)e * 7 + r] = er[r];
            c += er[r] * er[r];   // chi2 = e . (I e)
        }
        g.chi[e] = c;
    }
}

// constructQuadraticForm (base_binary_edge.hpp:54-120) of the edges of one vertex, in insertion order
__global__ __launch_bounds__(64) void eg_assemble_kernel(EGDev g) {
    if (g.ctl->done) return;
    const int v = blockIdx.x, tid = threadIdx.x;
    const int fv = g.vmap[v];
    if (fv < 0 || tid >= 56) return;
    const int D = g.ctl->D;
    const bool isH = tid < 49;
    const int r = isH ? tid / 7 : tid - 49, c = isH ? tid % 7 : 0;
    const int beg = g.vbeg[v], end = g.vbeg[v + 1];
    double* Hrow = g.H + (size_t)(7 * fv + r) * D + c;
    if (isH)
        for (int p = beg; p < end; p++) {
            const int ent = g.vlist[p], e = ent >> 1;
            const int fo = g.vmap[(ent & 1) ? g.ei[e] : g.ej[e]];
            if (fo >= 0) Hrow[7 * fo] = 0.0;
        }
    double acc = 0;
    for (int p = beg; p < end; p++) {
        const int ent = g.vlist[p], e = ent >> 1, a = ent & 1;
        const double* Ja = g.J + (size_t)e * 98 + a * 49;
        if (isH) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 7; k++) s += Ja[7 * k + r] * Ja[7 * k + c];
            acc += s;
            const int fo = g.vmap[a ? g.ei[e] : g.ej[e]];
            if (fo >= 0) {
                const double* Jo = g.J + (size_t)e * 98 + (1 - a) * 49;
                double s2 = 0;
#pragma unroll
                for (int k = 0; k < 7; k++) s2 += Ja[7 * k + r] * Jo[7 * k + c];
                Hrow[7 * fo] += s2;
            }
        } else {
            const double* er = g.err + (size_t)e * 7;
            double s = 0;
#pragma unroll
            for (int k = 0; k < 7; k++) s += Ja[7 * k + r] * -er[k];
            acc += s;
        }
    }
    if (isH) Hrow[7 * fv] = acc;
    else g.b[7 * fv + r] = acc;
}

// The head of one Levenberg iteration (optimization_algorithm_levenberg.cpp:61-90)
__global__ __launch_bounds__(64) void eg_begin_kernel(EGDev g, int it) {
    EGCtl* c = g.ctl;
    if (c->done) return;
    const int lane = threadIdx.x;
    const double cur = eg_seq_sum(g.E, lane, [&](int e) { return g.chi[e]; });
    if (lane != 0) return;
    if (it == 0) {
        if (c->nfree == 0) { c->done = 1; c->cur = cur; return; }   // nothing to optimise
        c->lambda = 1e-16;   // setUserLambdaInit (Optimizer.cc:749)
        c->ni = 2;
        c->nbad = 0;
    }
    c->cur = cur;
    c->ini = cur;
    c->qn = 0;
    c->rho = 0;
    c->trial_on = 1;
    c->iter++;
}

__global__ __launch_bounds__(256) void eg_stage_kernel(EGDev g) {
    if (g.ctl->done || !g.ctl->trial_on) return;
    const int D = g.ctl->D, Dp = solve_dp(D), ld = Dp + 1;
    const int r = blockIdx.y, c = blockIdx.x * 256 + threadIdx.x;
    if (r >= Dp || c >= Dp) return;
    double v = r == c ? 1.0 : 0.0;
    if (r < D && c < D) v = g.H[(size_t)r * D + c] + (r == c ? g.ctl->lambda : 0.0);
    g.Sg[(size_t)r * ld + c] = v;
}

__global__ __launch_bounds__(1024) void eg_solve_kernel(EGDev g) {
    if (g.ctl->done || !g.ctl->trial_on) return;
    extern __shared__ __attribute__((aligned(16))) double ysh[];   // y | dinv | vz, Dp each
    __shared__ double Ad[SB * (SB + 1)];
    __shared__ int s_ok;
    const int D = g.ctl->D, Dp = solve_dp(D);
    double* y = ysh;
    double* dinv = y + Dp;
    double* vz = dinv + Dp;
    const int tid = threadIdx.x;
    for (int i = tid; i < Dp; i += blockDim.x) y[i] = i < D ? g.b[i] : 0.0;
    if (tid == 0) s_ok = 1;
    __syncthreads();
    const int ok = ldlt_hbm_solve(g.Sg, D, y, dinv, vz, Ad, &s_ok);
    for (int i = tid; i < D; i += blockDim.x) g.x[i] = ok ? y[i] : 0.0;
    if (tid == 0) g.ctl->ok = ok;
}

// push() and oplus of every active vertex
__global__ __launch_bounds__(64) void eg_update_kernel(EGDev g) {
    if (g.ctl->done || !g.ctl->trial_on) return;
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= g.V) return;
    S3 s;
    eg_load(g.est + 8 * (size_t)v, s);
    eg_store(g.est_sv + 8 * (size_t)v, s);
    const int fv = g.vmap[v];
    if (fv < 0) return;
    S3 n;
    eg_oplus(g.x + 7 * (size_t)fv, g.fix_scale, s, n);
    eg_store(g.est + 8 * (size_t)v, n);
}

__global__ __launch_bounds__(64) void eg_chi_kernel(EGDev g) {
    if (g.ctl->done || !g.ctl->trial_on) return;
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= g.E) return;
    double c = 0;
    if (g.eok[e]) {
        S3 C, v1, v2;
        eg_load(g.meas + 8 * (size_t)e, C);
        eg_load(g.est + 8 * (size_t)g.ei[e], v1);
        eg_load(g.est + 8 * (size_t)g.ej[e], v2);
        double er[7];
        eg_error(C, v1, v2, er);
#pragma unroll
        for (int r = 0; r < 7; r++) c += er[r] * er[r];
    }
    g.chi_t[e] = c;
}

// The tail of one trial (optimization_algorithm_levenberg.cpp:92-160)
__global__ __launch_bounds__(64) void eg_ctl_kernel(EGDev g) {
    EGCtl* c = g.ctl;
    if (c->done || !c->trial_on) return;
    const int lane = threadIdx.x;
    const double lambda = c->lambda;
    double tmp = eg_seq_sum(g.E, lane, [&](int e) { return g.chi_t[e]; });
    const double scale = eg_seq_sum(c->D, lane, [&](int j) { return g.x[j] * (lambda * g.x[j] + g.b[j]); });
    if (!c->ok) tmp = DBL_MAX;
    double rho = c->cur - tmp;
    rho /= scale + 1e-3;
    const bool accept = rho > 0 && isfinite(tmp);
    if (!accept)   // pop()
        for (int k = lane; k < 8 * g.V; k += 64) g.est[k] = g.est_sv[k];
    if (lane != 0) return;
    if (accept) {
        const double u = 2 * rho - 1;
        double alpha = 1. - u * u * u;
        alpha = fmin(alpha, 2. / 3.);
        c->lambda = lambda * fmax(1. / 3., alpha);
        c->ni = 2;
        c->cur = tmp;
    } else {
        c->lambda = lambda * c->ni;
        c->ni *= 2;
    }
    c->rho = rho;
    if (c->ntrial < ORBBA_EG_MAX_TRIALS) g.o_acc[c->ntrial] = accept;
    c->ntrial++;
    const int qn = ++c->qn;
    if (rho < 0 && qn < EG_TRIALS) return;   // the next trial of this iteration
    c->trial_on = 0;
    if (qn == EG_TRIALS || rho == 0) { c->done = 1; return; }
    if ((c->ini - c->cur) * 1e3 < c->ini) c->nbad++; else c->nbad = 0;
    if (c->nbad >= 3) c->done = 1;
}

__global__ __launch_bounds__(64) void eg_recover_kernel(EGDev g) {
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx == 0) {
        g.o_iter[0] = g.ctl->iter;
        g.o_iter[1] = g.ctl->ntrial;
        g.o_chi2[0] = g.ctl->cur;
    }
    if (idx < g.V) {
        S3 s;
        eg_load(g.est + 8 * (size_t)idx, s);
        eg_store(g.o_g2o + 8 * (size_t)idx, s);
        float pose[12];
        F3 swc;
        eg_recover_pose(s, pose, swc);
#pragma unroll
        for (int k = 0; k < 12; k++) g.o_pose[12 * (size_t)idx + k] = pose[k];
    } else if (idx - g.V < g.N) {
        const int p = idx - g.V, r = g.pref[p];
        float P[3] = {g.pts[3 * (size_t)p], g.pts[3 * (size_t)p + 1], g.pts[3 * (size_t)p + 2]};
        if (r >= 0 && r < g.V) {
            S3 s;
            eg_load(g.est + 8 * (size_t)r, s);
            float pose[12], o[3];
            F3 swc;
            eg_recover_pose(s, pose, swc);
            eg_correct_point(swc, g.vs + 13 * (size_t)r, P, o);
            P[0] = o[0]; P[1] = o[1]; P[2] = o[2];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) g.o_pts[3 * (size_t)p + k] = P[k];
    }
}

thread_local Scratch g_eg;
thread_local float* g_eg_stage_ms = nullptr;   // orbba_essential_graph_profile: per-kernel device time

enum { EG_K_SETUP, EG_K_MEASURE, EG_K_LINEARIZE, EG_K_ASSEMBLE, EG_K_BEGIN, EG_K_STAGE, EG_K_SOLVE, EG_K_UPDATE,
       EG_K_CHI, EG_K_CTL, EG_K_RECOVER, EG_K_COUNT };

}  // namespace orbamd

using namespace orbamd;

static int eg_common(const orbba_essential_graph* in, const orbba_essential_graph_result* out) {
    ORB_CHECK_ARG(in && out, "null argument");
    ORB_CHECK_ARG(in->n_keyframes >= 1, "n_keyframes must be at least 1");
    ORB_CHECK_ARG(in->n_keyframes <= EG_MAX_KF, "more than ORBBA_EG_MAX_KEYFRAMES keyframes");
    ORB_CHECK_ARG(in->n_edges >= 0 && in->n_points >= 0, "negative sizes");
    ORB_CHECK_ARG(in->fixed_slot >= 0 && in->fixed_slot < in->n_keyframes, "fixed_slot out of range");
    ORB_CHECK_ARG(in->vertex_sim3 && in->edge_sim3, "null Sim3 table");
    ORB_CHECK_ARG(in->n_edges == 0 || (in->edge_i && in->edge_j && in->edge_table), "null edge array");
    ORB_CHECK_ARG(in->n_points == 0 || (in->points && in->point_ref), "null point array");
    ORB_CHECK_ARG(out->sim3_g2o && out->pose && out->iterations && out->chi2 && out->accept, "null output array");
    ORB_CHECK_ARG(in->n_points == 0 || out->points, "null output array");
    return ORB_OK;
}

extern "C" int orbba_optimize_essential_graph_device(const orbba_essential_graph* in, orbba_essential_graph_result* out,
                                                     void* stream) {
    int rc;
    if ((rc = eg_common(in, out))) return rc;
    if ((rc = g_eg.use_current_device())) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t V = in->n_keyframes, E = in->n_edges, E1 = std::max<size_t>(E, 1);
    const size_t Dmax = 7 * V, Dpm = solve_dp((int)Dmax);
    EGDev g;
    memset(&g, 0, sizeof(g));
    auto carve = [&](char* base) {
        Carver c{base};
        c.take(g.ctl, 1); c.take(g.est, V * 8); c.take(g.est_sv, V * 8); c.take(g.meas, E1 * 8); c.take(g.J, E1 * 98);
        c.take(g.err, E1 * 7); c.take(g.chi, E1); c.take(g.chi_t, E1); c.take(g.H, Dmax * Dmax); c.take(g.b, Dmax);
        c.take(g.x, Dmax); c.take(g.Sg, Dpm * (Dpm + 1)); c.take(g.vmap, V); c.take(g.vbeg, V + 1); c.take(g.vlist, 2 * E1);
        c.take(g.eok, E1);
        return c.off;
    };
    if ((rc = g_eg.ws.reserve(carve(nullptr)))) return rc;
    carve(g_eg.ws.as<char>());
    g.V = (int)V; g.E = (int)E; g.N = in->n_points; g.fixed = in->fixed_slot; g.fix_scale = in->fix_scale != 0;
    g.vs = in->vertex_sim3; g.es = in->edge_sim3; g.ei = in->edge_i; g.ej = in->edge_j; g.et = in->edge_table;
    g.pts = in->points; g.pref = in->point_ref;
    g.o_g2o = out->sim3_g2o; g.o_pose = out->pose; g.o_pts = out->points; g.o_meas = out->measurement;
    g.o_iter = out->iterations; g.o_chi2 = out->chi2; g.o_acc = out->accept;

    const size_t solve_lds = 3 * Dpm * sizeof(double);
    {
        static thread_local size_t lim[64] = {};
        size_t& cur = lim[g_eg.device & 63];
        if (solve_lds > cur) {
            ORB_HIP_TRY(hipFuncSetAttribute((const void*)eg_solve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)solve_lds));
            cur = solve_lds;
        }
    }
    // per-kernel device time for orbba_essential_graph_profile: an event pair around every launch, read back at once
    float* ms = g_eg_stage_ms;
    struct Events {   // destroyed on every way out
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~Events() {
            if (e0) (void)hipEventDestroy(e0);
            if (e1) (void)hipEventDestroy(e1);
        }
    } ev;
    if (ms) {
        ORB_HIP_TRY(hipEventCreate(&ev.e0));
        ORB_HIP_TRY(hipEventCreate(&ev.e1));
    }
    int launch_rc = ORB_OK;
    auto timed = [&](int k, auto&& launch) {
        if (launch_rc) return;
        bool ok = !ms || hipEventRecord(ev.e0, st) == hipSuccess;
        launch();
        if (ms) {
            float t = 0;
            ok = ok && hipEventRecord(ev.e1, st) == hipSuccess && hipEventSynchronize(ev.e1) == hipSuccess &&
                 hipEventElapsedTime(&t, ev.e0, ev.e1) == hipSuccess;
            if (!ok) {
                set_error("orbba_essential_graph_profile: event timing failed");
                launch_rc = ORB_EHIP;
            }
            ms[k] += t;
        }
    };
    const dim3 gE((unsigned)((E1 + 63) / 64)), gV((unsigned)((V + 63) / 64));
    ORB_HIP_TRY(hipMemsetAsync(g.H, 0, Dmax * Dmax * 8, st));
    timed(EG_K_SETUP, [&] { hipLaunchKernelGGL(eg_setup_kernel, dim3(1), dim3(1024), 0, st, g); });
    timed(EG_K_MEASURE, [&] { hipLaunchKernelGGL(eg_measure_kernel, gE, dim3(64), 0, st, g); });
    for (int it = 0; it < EG_ITERS; it++) {
        timed(EG_K_LINEARIZE, [&] {
            hipLaunchKernelGGL(eg_linearize_kernel, dim3((unsigned)((E1 + EG_LIN_EDGES - 1) / EG_LIN_EDGES)),
                               dim3(32 * EG_LIN_EDGES), 0, st, g);
        });
        timed(EG_K_ASSEMBLE, [&] { hipLaunchKernelGGL(eg_assemble_kernel, dim3((unsigned)V), dim3(64), 0, st, g); });
        timed(EG_K_BEGIN, [&] { hipLaunchKernelGGL(eg_begin_kernel, dim3(1), dim3(64), 0, st, g, it); });
        for (int q = 0; q < EG_TRIALS; q++) {
            timed(EG_K_STAGE, [&] {
                hipLaunchKernelGGL(eg_stage_kernel, dim3((unsigned)((Dpm + 255) / 256), (unsigned)Dpm), dim3(256), 0, st, g);
            });
            timed(EG_K_SOLVE, [&] { hipLaunchKernelGGL(eg_solve_kernel, dim3(1), dim3(1024), solve_lds, st, g); });
            timed(EG_K_UPDATE, [&] { hipLaunchKernelGGL(eg_update_kernel, gV, dim3(64), 0, st, g); });
            timed(EG_K_CHI, [&] { hipLaunchKernelGGL(eg_chi_kernel, gE, dim3(64), 0, st, g); });
            timed(EG_K_CTL, [&] { hipLaunchKernelGGL(eg_ctl_kernel, dim3(1), dim3(64), 0, st, g); });
        }
    }
    timed(EG_K_RECOVER, [&] {
        hipLaunchKernelGGL(eg_recover_kernel, dim3((unsigned)((V + in->n_points + 63) / 64)), dim3(64), 0, st, g);
    });
    if (launch_rc) return launch_rc;
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

static bool eg_finite13(const float* row) {
    for (int k = 0; k < 13; k++)
        if (!std::isfinite(row[k])) return false;
    return true;
}

// The host entry's checks of the arrays' contents (the device entry cannot read them)
static int eg_check_host(const orbba_essential_graph* in) {
    const int V = in->n_keyframes;
    for (int v = 0; v < V; v++) {
        ORB_CHECK_ARG(eg_finite13(in->vertex_sim3 + 13 * v) && eg_finite13(in->edge_sim3 + 13 * v), "non-finite Sim3");
        ORB_CHECK_ARG(in->vertex_sim3[13 * v + 12] > 0 && in->edge_sim3[13 * v + 12] > 0, "a scale must be positive");
    }
    for (int e = 0; e < in->n_edges; e++) {
        const int i = in->edge_i[e], j = in->edge_j[e];
        ORB_CHECK_ARG(i >= 0 && i < V && j >= 0 && j < V, "edge index out of range");
        ORB_CHECK_ARG(i != j, "edge_i == edge_j");
    }
    for (int p = 0; p < in->n_points; p++) {
        ORB_CHECK_ARG(in->point_ref[p] >= -1 && in->point_ref[p] < V, "point_ref out of range");
        ORB_CHECK_ARG(std::isfinite(in->points[3 * p]) && std::isfinite(in->points[3 * p + 1]) &&
                          std::isfinite(in->points[3 * p + 2]), "non-finite point");
    }
    return ORB_OK;
}

static int eg_host(const orbba_essential_graph* in, orbba_essential_graph_result* out, int device) {
    int rc;
    if ((rc = eg_common(in, out))) return rc;   // the checks, before any device call
    if ((rc = eg_check_host(in))) return rc;
    const size_t V = in->n_keyframes, E = in->n_edges, N = in->n_points;
    orbba_essential_graph d = *in;
    orbba_essential_graph_result r = *out;
    Mirror io;
    io.add(d.vertex_sim3, V * 13, true, false); io.add(d.edge_sim3, V * 13, true, false); io.add(d.edge_i, E, true, false);
    io.add(d.edge_j, E, true, false); io.add(d.edge_table, E, true, false); io.add(d.points, N * 3, true, false);
    io.add(d.point_ref, N, true, false);
    io.add(r.sim3_g2o, V * 8, false, true); io.add(r.pose, V * 12, false, true); io.add(r.points, N * 3, false, true);
    io.add(r.measurement, E * 8, false, true); io.add(r.iterations, 2, false, true); io.add(r.chi2, 1, false, true);
    io.add(r.accept, ORBBA_EG_MAX_TRIALS, false, true);
    return run_host(g_eg, device, io, [&] { return orbba_optimize_essential_graph_device(&d, &r, nullptr); });
}

extern "C" int orbba_optimize_essential_graph(const orbba_essential_graph* in, orbba_essential_graph_result* out,
                                              int device) {
    return eg_host(in, out, device);
}

extern "C" int orbba_essential_graph_profile(const orbba_essential_graph* in, orbba_essential_graph_result* out,
                                             int device, float* kernel_ms) {
    ORB_CHECK_ARG(kernel_ms, "null argument");
    for (int k = 0; k < EG_K_COUNT; k++) kernel_ms[k] = 0;
    g_eg_stage_ms = kernel_ms;
    const int rc = eg_host(in, out, device);
    g_eg_stage_ms = nullptr;
    return rc;
}

extern "C" int orbba_essential_graph_edges(const orbba_eg_tables* g, int32_t min_weight, int32_t capacity,
                                           int32_t* edge_i, int32_t* edge_j, uint8_t* edge_table, int32_t* n_edges) {
    ORB_CHECK_ARG(g && n_edges, "null argument");
    ORB_CHECK_ARG(capacity >= 0 && (capacity == 0 || (edge_i && edge_j && edge_table)), "null edge array");
    const int V = g->n_keyframes;
    ORB_CHECK_ARG(V >= 1 && g->n_connections >= 0, "bad sizes");
    ORB_CHECK_ARG(g->kf_id && g->parent && g->loop_begin && g->covis_begin, "null table");
    ORB_CHECK_ARG(g->n_connections == 0 || (g->conn_kf && g->conn_begin), "null connection table");
    ORB_CHECK_ARG(g->curr_slot >= 0 && g->curr_slot < V && g->loop_kf_slot >= 0 && g->loop_kf_slot < V,
                  "curr_slot / loop_kf_slot out of range");
    auto rows_ok = [&](const int32_t* begin, int n, const int32_t* slot, int lo) {
        if (begin[0] != 0) return false;
        for (int k = 0; k < n; k++)
            if (begin[k + 1] < begin[k]) return false;
        if (begin[n] > 0 && !slot) return false;
        for (int p = 0; p < begin[n]; p++)
            if (slot[p] < lo || slot[p] >= V) return false;
        return true;
    };
    ORB_CHECK_ARG(rows_ok(g->loop_begin, V, g->loop_slot, -1), "bad loop edge rows");
    ORB_CHECK_ARG(rows_ok(g->covis_begin, V, g->covis_slot, -1), "bad covisibility rows");
    ORB_CHECK_ARG(g->covis_begin[V] == 0 || g->covis_weight, "null covis_weight");
    if (g->n_connections) ORB_CHECK_ARG(rows_ok(g->conn_begin, g->n_connections, g->conn_slot, 0), "bad connection rows");
    for (int k = 0; k < V; k++) ORB_CHECK_ARG(g->parent[k] >= -1 && g->parent[k] < V && g->parent[k] != k, "parent out of range");
    for (int c = 0; c < g->n_connections; c++) {
        ORB_CHECK_ARG(g->conn_kf[c] >= 0 && g->conn_kf[c] < V, "conn_kf out of range");
        for (int p = g->conn_begin[c]; p < g->conn_begin[c + 1]; p++)
            ORB_CHECK_ARG(g->conn_slot[p] != g->conn_kf[c], "a keyframe connected to itself");
    }
    for (int k = 0; k < V; k++) {
        for (int p = g->loop_begin[k]; p < g->loop_begin[k + 1]; p++)
            ORB_CHECK_ARG(g->loop_slot[p] != k, "a keyframe is its own loop edge");
        for (int p = g->covis_begin[k]; p < g->covis_begin[k + 1]; p++)
            ORB_CHECK_ARG(g->covis_slot[p] != k, "a keyframe covisible with itself");
    }
    const std::vector<EgEdge> ed = eg_build_edges(*g, min_weight);
    *n_edges = (int32_t)ed.size();
    for (size_t e = 0; e < ed.size() && e < (size_t)capacity; e++) {
        edge_i[e] = ed[e].i;
        edge_j[e] = ed[e].j;
        edge_table[e] = ed[e].table;
    }
    return ORB_OK;
}
