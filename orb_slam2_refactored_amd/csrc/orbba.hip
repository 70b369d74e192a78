// orbba.hip — Optimizer::LocalBundleAdjustment on gfx950.
//
// g2o's Levenberg-Marquardt over SE3Expmap poses and marginalised XYZ points, fp64 throughout.
// Points own their edges (CSR); a point is served by a group of 8 lanes (one edge per lane,
// fixed-order shuffle reductions), so per-point work spreads over ~N/8 wavefronts.
//   per LM trial (OptimizationAlgorithmLevenberg::solve, levenberg.cpp:61-164; the do { ... } while
//   (rho < 0 ...) retries re-run only the lambda-dependent parts), five launches:
//     ba_iter_kernel         on a new iteration: computeActiveErrors + robust chi2 + linearizeOplus +
//                            constructQuadraticForm, Hll / b_l per point, per-edge pose parts; then
//                            (lambda known) D^-1 = (Hll + lambda I)^-1, W = Hpl D^-1, Hpl D^-1 b_l
//     ba_schur_block_kernel  S(i1,i2) = Hpp + lambda I - sum W Hpl^T per block (pair list in parts);
//                            beside them one workgroup per pose: on a new iteration its Hpp / b_p,
//                            then b_schur; and the chi2 total
//     ba_solve_kernel        blocked LDL^T of the (6P)^2 reduced camera system in LDS, triangular
//                            solves, push + SE3 exp-update of the free poses
//     ba_point_update_kernel back-substitution, push, point +=, errors + robust chi2 of its edges
//     ba_decide_kernel       rho, lambda / nu update, accept or pop (restore)
//   The first trial of an optimize() call runs ba_pose_accum_kernel and ba_schur_point_kernel
//   (computeLambdaInit from the diagonal maxima the first two gather, then the Schur point terms)
//   between the first two.
// Every reduction runs in a fixed order, so results are bit-reproducible run to run.  The LM
// control scalars live on the device; the host reads one small status block per trial to decide
// whether to run another (the reference's loop condition), and polls the stop flag like g2o.
//
// This file is the host side.  The kernels are in the headers below, one translation unit, in
// dependency order; the buffer regions in ba_layout.h.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "ba_layout.h"
#include "ba_structure.h"
#include "common.h"
#include "host_helper.h"
#include "se3.h"
#include "ba_window.h"

#include "orbba_dev.h"
#include "orbba_linearize.h"
#include "orbba_schur.h"
#include "orbba_solve.h"
#include "orbba_step.h"
#include "orbba_struct.h"

using namespace orbamd;
using namespace orbamd_host;

namespace {

// Grow-only pinned host buffer.  Only grown when no copy from it is in flight.
struct PinnedBuf {
    char* ptr = nullptr;
    char* dptr = nullptr;   // the device's view (mapped buffers)
    size_t cap = 0;
    int ensure(size_t bytes, bool mapped = false) {
        if (bytes <= cap) return ORB_OK;
        if (ptr) (void)hipHostFree(ptr);
        ptr = dptr = nullptr;
        cap = 0;
        const size_t c = align_up(bytes + bytes / 4, 1 << 16);
        ORB_HIP_TRY(hipHostMalloc((void**)&ptr, c, mapped ? hipHostMallocMapped : hipHostMallocDefault));
        if (mapped) ORB_HIP_TRY(hipHostGetDevicePointer((void**)&dptr, ptr, 0));
        cap = c;
        return ORB_OK;
    }
    ~PinnedBuf() {
        if (ptr) (void)hipHostFree(ptr);
    }
};

// Device-resident LocalBA workspace (one per thread: LocalMapping runs one LocalBA at a time).
struct BAContext {
    HostHelper helper;   // destroyed last (declared first): no job is in flight after a call returns
    int device = -1;
    hipStream_t st = nullptr;
    DevBuf prob, state, structure, sys, ctlbuf;
    DevBuf res_dev;   // the results of a call on a device-resident window (ResultLayout, then pose_R)
    BACtl* h_ctl = nullptr;   // pinned
    BACtl* h_ring = nullptr;  // pinned, device-mapped control snapshots, one per step in flight
    BACtl* d_ring = nullptr;
    int step_seq = 0;         // id of the last enqueued LM step (snapshot sequence)
    int32_t* h_stop = nullptr;   // pinned, device-mapped mirror of the caller's stop flag
    int32_t* d_stop = nullptr;
    PinnedBuf h_prob, h_struct, h_res;   // pinned staging images (one copy each way)
    int next_seq() const { return step_seq == 0x7fffffff ? 1 : step_seq + 1; }   // the id after step_seq
    void release() {   // everything device-bound
        prob.release(); state.release(); structure.release(); sys.release(); ctlbuf.release(); res_dev.release();
        if (st) { (void)hipStreamDestroy(st); st = nullptr; }
        if (h_ring) { (void)hipHostFree(h_ring); h_ring = nullptr; d_ring = nullptr; }
        if (h_stop) { (void)hipHostFree(h_stop); h_stop = nullptr; d_stop = nullptr; }
        if (h_ctl) { (void)hipHostFree(h_ctl); h_ctl = nullptr; }
    }
    // Everything device-bound belongs to `device`: a call on another device from the same thread
    // releases it all (buffers, stream, events) before building the new device's set.
    void reset_device() {
        if (device >= 0) (void)hipSetDevice(device);
        if (st) (void)hipStreamSynchronize(st);
        release();
        device = -1;
    }
    int acquire(int dev) {   // make `dev` the context's and the calling thread's device
        if (device != dev) {
            int ndev = 0;
            ORB_HIP_TRY(hipGetDeviceCount(&ndev));
            ORB_CHECK_ARG(dev >= 0 && dev < ndev, "no such HIP device");
            reset_device();
            ORB_HIP_TRY(hipSetDevice(dev));
            ORB_HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
            ORB_HIP_TRY(hipHostMalloc((void**)&h_ctl, sizeof(BACtl), hipHostMallocDefault));
            ORB_HIP_TRY(hipHostMalloc((void**)&h_ring, 2 * sizeof(BACtl), hipHostMallocMapped));
            ORB_HIP_TRY(hipHostGetDevicePointer((void**)&d_ring, h_ring, 0));
            ORB_HIP_TRY(hipHostMalloc((void**)&h_stop, 64, hipHostMallocMapped));
            ORB_HIP_TRY(hipHostGetDevicePointer((void**)&d_stop, h_stop, 0));
            for (int k = 0; k < 2; k++) h_ring[k].seq = -1;
            device = dev;
        }
        ORB_HIP_TRY(hipSetDevice(dev));
        return ORB_OK;
    }
    ~BAContext() { release(); }
};
thread_local BAContext g_ba;

// The call's buffer initialisations as ONE launch per batch (ba_fill_kernel) instead of a hipMemsetAsync
// each (round 6: 11 memsets per call ran as 16 fill kernels of ~4.4 us, ~70 us of the call's GPU time in
// rocprofv3).
struct FillQueue {
    BAFill f{};
    unsigned long long bytes = 0;
    int add(void* p, size_t n, int v, hipStream_t st) {
        if (!n) return ORB_OK;
        if (f.cnt == BA_FILL_MAX) {
            if (int rc = flush(st)) return rc;
        }
        f.p[f.cnt] = p;
        f.n[f.cnt] = n;
        f.v[f.cnt] = (unsigned)v;
        f.cnt++;
        bytes += n;
        return ORB_OK;
    }
    void set_ctl(BACtl* c, const BACtl& init) {
        f.ctl = c;
        f.ctl_init = init;
    }
    int flush(hipStream_t st) {
        if (!f.cnt && !f.ctl) return ORB_OK;
        const unsigned nb = (unsigned)std::max<unsigned long long>(1, std::min<unsigned long long>(1024, bytes / (16 * 256 * 2)));
        hipLaunchKernelGGL(ba_fill_kernel, dim3(nb), dim3(256), 0, st, f);
        f.cnt = 0;
        f.ctl = nullptr;
        bytes = 0;
        ORB_HIP_TRY(hipGetLastError());
        return ORB_OK;
    }
};

// The environment knobs.  Read at the start of every call (tests flip them between
// calls in one process), but for ORBBA_DEBUG_TIMING, read once per process.
struct BAOptions {
    bool timing;         // ORBBA_DEBUG_TIMING: host-side phase times to stderr at the end of the call
    std::string smode;   // ORBBA_STRUCT: "host" = the whole structure build on the host (generic), "sorted" =
                         // the host's point-sorted variant; default: counts on the host, lists on the device
                         // when the edges are point-sorted
    int stop_after;      // ORBBA_DEBUG_STOP_AFTER_TRIALS, test hook (tests/test_ba_gpu.py); -1: off
    int spec_slack;      // ORBBA_DEBUG_SPEC_EARLY=1, test hook: enqueue the loop ends one step too early, so
                         // that each loop's first guesses miss and the fallback paths run
    bool solve256;       // ORBBA_SOLVE_THREADS=256: the LDS solve's round-5 workgroup instead of 1024 threads
    int simd0_helpers;   // ORBBA_SOLVE_SIMD0=1: wavefront 0's SIMD-mates take trailing tiles too
    std::string gba_solve;   // ORBBA_GBA_SOLVE: "grid" / "single" force BundleAdjustment's HBM solve path
    bool try_counts() const { return smode != "host" && smode != "sorted" && smode != "generic"; }
};
BAOptions read_options() {
    static const bool timing = getenv("ORBBA_DEBUG_TIMING") != nullptr;
    auto num = [](const char* name, int unset) {
        const char* e = getenv(name);
        return e ? atoi(e) : unset;
    };
    const char* smode = getenv("ORBBA_STRUCT");
    BAOptions o;
    o.timing = timing;
    o.smode = smode ? smode : "";
    o.stop_after = num("ORBBA_DEBUG_STOP_AFTER_TRIALS", -1);
    o.spec_slack = num("ORBBA_DEBUG_SPEC_EARLY", 0) != 0 ? 1 : 0;
    o.solve256 = num("ORBBA_SOLVE_THREADS", 0) == 256;
    o.simd0_helpers = num("ORBBA_SOLVE_SIMD0", 0) != 0 ? 1 : 0;
    const char* gs = getenv("ORBBA_GBA_SOLVE");
    o.gba_solve = gs ? gs : "";
    return o;
}

// host-side phase timing (ORBBA_DEBUG_TIMING=1: printed to stderr at the end of the call)
struct PhaseTimer {
    bool on;
    std::vector<std::pair<const char*, std::chrono::steady_clock::time_point>> marks;
    void mark(const char* n) {
        if (on) marks.emplace_back(n, std::chrono::steady_clock::now());
    }
    void report() const {
        for (size_t i = 1; i < marks.size(); i++)
            fprintf(stderr, "orbba %-28s %8.1f us\n", marks[i].first,
                    std::chrono::duration<double, std::micro>(marks[i].second - marks[i - 1].second).count());
    }
};

constexpr int LOOKAHEAD = 2;     // LM steps kept enqueued ahead of the host (= control snapshot ring slots)

// What a call runs on the problem: the optimize() calls, the robust kernels they start with, the edge typing
// and whether the outliers are classified (between two optimize() calls and into edge_outlier at the end).
struct BASchedule {
    int loops;          // optimize() calls: 1 or 2
    int iters[2];       // their iterations
    int robust;         // the edges' robust-kernel flag at the start (Huber, delta by edge type)
    int stereo_rule;    // ORBBA_GBA_RULE_LOCAL: ur < 0 => mono (Optimizer.cc:595); _REFERENCE: `if (ur)` (:253)
    bool classify;      // levels + robust kernels off between the loops, edge_outlier at the end
    bool grid_solve;    // a reduced system in HBM may be factored over the grid (ldlt_grid.h; ORBBA_GBA_SOLVE)
};
// Free keyframes from which the grid-wide factorisation is the default (the smallest measured size at
// which it beats the single workgroup by more than the run-to-run spread)
constexpr int GBA_GRID_MIN_FREE_KEYFRAMES = 64;
// LocalBundleAdjustment: optimize(5), classify, optimize(10) (Optimizer.cc:636-672)
constexpr BASchedule LOCAL_BA_SCHEDULE{2, {5, 10}, 1, ORBBA_GBA_RULE_LOCAL, true, false};

// Where a call's results go (orbba_result's and orbba_gba_result's common part).
struct BAOutputs {
    double *pose_R, *pose_t, *pose_q, *points;
    uint8_t* edge_outlier;   // null without a classification
    double* edge_chi2;
    int32_t iterations[2] = {0, 0};
    double chi2[2] = {0, 0};
    int32_t trials = 0;      // LM trials over the whole call
    int32_t ran = 0;
};

// One optimize()'s loop as the host sees it.
struct LoopState {
    int iters;
    bool fresh, last_loop;   // the call's first optimize() / its last
    int enq = 0, seen = 0;   // steps enqueued / snapshots read
    int spec_at = 0;         // steps enqueued ahead of the latest speculative gather / classification
    bool trans_spec = false; // the second loop's ctl_start is enqueued behind the first loop's steps
    int ids[LOOKAHEAD] = {0, 0};
    bool fin = false, stop_sent = false;
    BACtl last{};
    // iterations that can still be needed (the latest snapshot's)
    int remaining() const { return seen ? last.iters_max - last.it : iters; }
};

// The dynamic LDS limit is a process-wide attribute of a solve kernel: raised (a host call) only when a call needs
// more than any call before it on this device, never lowered.  One table for every caller of these kernels (LocalBACall
// and the debug entries at the end of this file).
enum SolveKernel { SOLVE_LDS_1024 = 0, SOLVE_HBM = 1, SOLVE_LDS_256 = 2 };
static int raise_solve_lds_limit(SolveKernel which, int device, size_t ldlt_lds) {
    static std::mutex mu;
    static size_t lim[64][3] = {};
    const void* solve_fn = which == SOLVE_HBM       ? (const void*)ba_solve_global_kernel
                           : which == SOLVE_LDS_256 ? (const void*)ba_solve_kernel<256>
                                                    : (const void*)ba_solve_kernel<1024>;
    const size_t need = std::max<size_t>(ldlt_lds, 1024);
    std::lock_guard<std::mutex> lk(mu);
    size_t& cur = lim[device & 63][which];
    if (need > cur) {
        ORB_HIP_TRY(hipFuncSetAttribute(solve_fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
        cur = need;
    }
    return ORB_OK;
}

// The second staging path: UploadLayout filled in HBM from a gathered window (ba_window.h), the values stage_problem
// copies from the host.  q by the host's quat_from_R on the widened rotation, everything else an exact widening.
__global__ __launch_bounds__(256) void ba_stage_window_kernel(BaWindowRun r, UploadLayout up, int one_cam) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int P = r.n_local + r.n_fixed;
    if (i < P) {
        const int k = r.w.pose_kf[i];
        double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, t[3] = {0, 0, 0};
        if (k >= 0 && k < r.K) {
            for (int j = 0; j < 9; j++) R[j] = (double)r.kf_pose[12 * (size_t)k + j];
            for (int j = 0; j < 3; j++) t[j] = (double)r.kf_pose[12 * (size_t)k + 9 + j];
        }
        quat_from_R(R, up.q + 4 * (size_t)i);
        for (int j = 0; j < 3; j++) up.t[3 * (size_t)i + j] = t[j];
        up.fixed[i] = r.w.pose_fixed[i];
    }
    if (i < r.n_points) {
        const int p = r.w.point[i];
        for (int j = 0; j < 3; j++) up.X[3 * (size_t)i + j] = (p >= 0 && p < r.M) ? (double)r.mp_xw[3 * (size_t)p + j] : 0.0;
    }
    if (i < r.n_edges) {
        up.ep[i] = r.w.edge_point[i];
        up.ek[i] = r.w.edge_pose[i];
        const float ur = r.w.edge_obs[3 * (size_t)i + 2];
        up.stereo[i] = ur < 0 ? 0 : 1;   // ur < 0 => mono (:595)
        for (int j = 0; j < 3; j++) up.obs[3 * (size_t)i + j] = (double)r.w.edge_obs[3 * (size_t)i + j];
        up.info[i] = (double)r.w.edge_inv_sigma2[i];
        if (!one_cam || i == 0)
            for (int j = 0; j < 5; j++) up.cam[5 * (size_t)i + j] = (double)r.w.edge_cam[5 * (size_t)i + j];
    }
}

// toRotationMatrix of the gathered estimates, as finish() does on the host
__global__ __launch_bounds__(256) void ba_result_rotation_kernel(const double* q, double* R, int P) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < P) q_to_R(q + 4 * (size_t)i, R + 9 * (size_t)i);
}

// One orbba_local_ba call.
struct LocalBACall {
    const orbba_problem* pr;
    BAOutputs* res;
    const BASchedule sch;
    const volatile int32_t* stop_flag;
    const int device, P, N, E;
    BAContext& C;
    HostStructure& hs;   // the calling thread's (capacity kept across calls)
    const BAOptions opt = read_options();
    PhaseTimer tm{opt.timing, {}};
    hipStream_t st = nullptr;
    BADev b{};
    FillQueue fills;   // flushed (one launch) before the first kernel that reads them
    ResultLayout dres{};   // the kernels' view of the mapped pinned result region
    int n_gather = 0;
    BaWindowRun* win = nullptr;   // the problem is a gathered window in HBM: the second staging path
    hipStream_t win_stream = nullptr;
    orbba_problem* win_pr = nullptr;   // pr, writable: its three host arrays are set by stage_window
    uint8_t* d_level = nullptr;   // b.level, writable (the classification between the loops sets it)
    // the host half of the structure build, posted to the helper thread
    bool counts_ok = false;
    struct HelperWait {   // every return path waits for a posted job (it writes hs and counts_ok)
        HostHelper& h;
        bool on;
        ~HelperWait() {
            if (on) h.wait();
        }
    } helper_wait{C.helper, false};
    // The structure is built once, for the first optimize() (every edge at level 0).  The second
    // optimize() (initializeOptimization(0) after the outliers went to level 1) reuses it: its active
    // edges are a subset, the kernels skip level-1 edges (their J / W stay 0, so every sum, Schur block
    // and dense factorisation sees exact zeros in their place), and a vertex left without active edges
    // keeps a zero Hessian block (+ lambda), i.e. a zero update, as if it were not in the problem.
    bool have_structure = false;
    bool dev_build = false;         // act / pt_slot / ps_slot / blk_pair filled on the device
    bool have_classified = false;   // the outlier classification ran (second optimize())
    // the solve of this call's system (plan_solve)
    bool glob = false;   // reduced system in HBM (ba_solve_global_kernel)
    bool grid = false;   // ... and factored over the grid (ldlt_grid.h), BundleAdjustment only
    LdltGrid lg{};
    int D = 0, Dp = 0;
    size_t ldlt_lds = 0;
    dim3 gg;                     // the point kernels' grid: 8 lanes per point
    double* d_wgpart = nullptr;  // point-update workgroup partials
    // loop ends enqueued ahead of the host seeing the loop end
    bool leveled = false;         // a speculative classification ran behind the step that ended the first loop
    bool started_ahead = false;   // ... and the second loop's ctl_start
    bool gathered = false;        // a speculative gather ran behind the step that ended the last loop
    bool hook_stopped = false;    // the device ended a loop on the stop flag (or the test hook)
    int spec_launched[2] = {0, 0};   // speculative loop ends enqueued per loop (ORBBA_DEBUG_TIMING report)

    LocalBACall(const orbba_problem* pr_, BAOutputs* res_, const BASchedule& sch_, const volatile int32_t* stop_,
                int device_, BAContext& C_, HostStructure& hs_)
        : pr(pr_), res(res_), sch(sch_), stop_flag(stop_), device(device_), P(pr_->n_poses), N(pr_->n_points), E(pr_->n_edges),
          C(C_), hs(hs_) {}

    bool stopped() const { return stop_flag && *stop_flag; }

    int validate() {
        ORB_CHECK_ARG(P >= 0 && N >= 0 && E >= 0, "negative sizes");
        ORB_CHECK_ARG(win || (res->pose_R && res->pose_t && res->points && (res->edge_outlier || !sch.classify)),
                      "null result buffers");
        tm.mark("entry");
        for (int e = 0; e < E; e++)
            ORB_CHECK_ARG(pr->edge_point[e] >= 0 && pr->edge_point[e] < N && pr->edge_pose[e] >= 0 &&
                              pr->edge_pose[e] < P, "edge references a missing vertex");
        tm.mark("edge checks");
        return ORB_OK;
    }

    // The host half of the structure build: on the helper thread, in parallel with the staging
    // (default path; ORBBA_STRUCT is read per call: tests compare the forms in one process).
    void post_counts() {
        if (!opt.try_counts() || E < 1024) return;
        HostStructure* hsp = &hs;   // (the helper's own thread_local hs is another object)
        bool* ok = &counts_ok;
        const orbba_problem* p = pr;
        C.helper.post([hsp, ok, p] {
            try {   // (an exception must not leave the helper thread: the calling thread's build takes over)
                *ok = build_structure_counts(p->n_poses, p->n_points, p->pose_fixed, p->edge_point, p->edge_pose,
                                             p->n_edges, *hsp);
            } catch (...) {
                *ok = false;
            }
        });
        helper_wait.on = true;
    }

    // ---- device problem + state.  Everything the host provides is laid out in one region, built
    // in pinned staging with the same offsets and uploaded with a single copy.
    int stage_problem() {
        // initial estimates: SE3Quat(R, t) -> Quaterniond(R) normalised (Optimizer.cc:145-150)
        std::vector<double> q0(4 * (size_t)P);
        for (int i = 0; i < P; i++) quat_from_R(pr->pose_R + 9 * i, &q0[4 * i]);
        // One camera for the whole window (every keyframe of a map shares the calibration: the usual case)
        // goes up once instead of 40 B per edge: half the staging copy and the upload (round 6)
        bool one_cam = E > 0;
        for (int e = 1; e < E && one_cam; e++) one_cam = std::memcmp(pr->edge_cam + 5 * (size_t)e, pr->edge_cam, 40) == 0;
        UploadLayout up, h;
        StateLayout s;
        const size_t up_bytes = up.carve(nullptr, P, N, E, one_cam);
        int rc;
        if ((rc = C.prob.reserve(up_bytes))) return rc;
        if ((rc = C.state.reserve(s.carve(nullptr, P, N, E)))) return rc;
        if ((rc = C.ctlbuf.reserve(sizeof(BACtl) + 64))) return rc;
        if ((rc = C.h_prob.ensure(up_bytes))) return rc;
        if ((rc = C.h_res.ensure(dres.carve(nullptr, P, N, E), true))) return rc;   // mapped: the final gather writes it directly
        up.carve(C.prob.as<char>(), P, N, E, one_cam);
        h.carve(C.h_prob.ptr, P, N, E, one_cam);
        s.carve(C.state.as<char>(), P, N, E);
        std::memcpy(h.fixed, pr->pose_fixed, P);
        std::memcpy(h.ep, pr->edge_point, 4 * (size_t)E);
        std::memcpy(h.ek, pr->edge_pose, 4 * (size_t)E);
        if (sch.stereo_rule == ORBBA_GBA_RULE_LOCAL)
            for (int e = 0; e < E; e++) h.stereo[e] = pr->edge_obs[3 * e + 2] < 0 ? 0 : 1;   // ur < 0 => mono (:595)
        else   // `if (ur)` (:253): any non-zero ur, -1 included, is a mono edge; ur == 0 a stereo edge (u, v, 0)
            for (int e = 0; e < E; e++) h.stereo[e] = pr->edge_obs[3 * e + 2] != 0 ? 0 : 1;
        std::memcpy(h.obs, pr->edge_obs, 24 * (size_t)E);
        std::memcpy(h.info, pr->edge_inv_sigma2, 8 * (size_t)E);
        std::memcpy(h.cam, pr->edge_cam, 8 * (one_cam ? 5 : 5 * (size_t)E));
        std::memcpy(h.q, q0.data(), 32 * (size_t)P);
        std::memcpy(h.t, pr->pose_t, 24 * (size_t)P);
        std::memcpy(h.X, pr->points, 24 * (size_t)N);
        ORB_HIP_TRY(hipMemcpyAsync(C.prob.ptr, C.h_prob.ptr, up_bytes, hipMemcpyHostToDevice, st));
        dres.carve(C.h_res.dptr, P, N, E);
        return bind_problem(up, s, one_cam);
    }

    // The window's form of stage_problem: the same region filled by a kernel; pose_fixed, edge_point and edge_pose (the
    // region's first three fields) come back for the structure build, the results stay in HBM.
    int stage_window() {
        const bool one_cam = E > 0 && win->one_cam;
        UploadLayout up, h;
        StateLayout s;
        const size_t up_bytes = up.carve(nullptr, P, N, E, one_cam);
        const size_t res_bytes = dres.carve(nullptr, P, N, E);
        int rc;
        if ((rc = C.prob.reserve(up_bytes))) return rc;
        if ((rc = C.state.reserve(s.carve(nullptr, P, N, E)))) return rc;
        if ((rc = C.ctlbuf.reserve(sizeof(BACtl) + 64))) return rc;
        if ((rc = C.h_prob.ensure(up_bytes))) return rc;
        if ((rc = C.res_dev.reserve(res_bytes + 72 * (size_t)P + 256))) return rc;
        up.carve(C.prob.as<char>(), P, N, E, one_cam);
        h.carve(C.h_prob.ptr, P, N, E, one_cam);
        s.carve(C.state.as<char>(), P, N, E);
        dres.carve(C.res_dev.as<char>(), P, N, E);
        const int n = std::max(E, std::max(N, P));
        if (n) hipLaunchKernelGGL(ba_stage_window_kernel, dim3((n + 255) / 256), dim3(256), 0, st, *win, up, one_cam ? 1 : 0);
        ORB_HIP_TRY(hipGetLastError());
        const size_t back = (size_t)((char*)up.stereo - (char*)up.fixed);   // fixed, ep, ek
        ORB_HIP_TRY(hipMemcpyAsync(C.h_prob.ptr, C.prob.ptr, back, hipMemcpyDeviceToHost, st));
        ORB_HIP_TRY(hipStreamSynchronize(st));
        win_pr->pose_fixed = h.fixed;
        win_pr->edge_point = h.ep;
        win_pr->edge_pose = h.ek;
        if ((rc = validate())) return rc;
        return bind_problem(up, s, one_cam);
    }

    int bind_problem(const UploadLayout& up, const StateLayout& s, bool one_cam) {
        int rc;
        b.P = P; b.N = N; b.E = E;
        b.q = up.q; b.t = up.t; b.X = up.X;
        b.q_sv = s.q_sv; b.t_sv = s.t_sv; b.X_sv = s.X_sv;
        b.fixed = up.fixed; b.ep = up.ep; b.ek = up.ek; b.stereo = up.stereo; b.obs = up.obs; b.info = up.info;
        b.cam = up.cam;
        b.cam_step = one_cam ? 0 : 5;
        b.robust = s.robust; b.level = d_level = s.level; b.err = s.err;
        b.ctl = C.ctlbuf.as<BACtl>();
        b.stop = stop_flag ? C.d_stop : nullptr;
        b.stop_after = opt.stop_after;
        // (the control block is written whole by the first optimize()'s fill: trials / stopped count from 0
        // over the whole call)
        if ((rc = fills.add(s.robust, E, sch.robust ? 1 : 0, st)) || (rc = fills.add(s.level, E, 0, st)) ||
            (rc = fills.add(s.err, 24 * (size_t)E, 0, st)))
            return rc;
        res->iterations[0] = res->iterations[1] = 0;
        res->chi2[0] = res->chi2[1] = 0;
        // the final classification + poses / points are gathered straight into the mapped pinned result
        // region (round 6: no device-to-host copy behind the kernel); a window's stay in HBM
        n_gather = std::max(E, std::max(N, P));
        tm.mark("staging + upload enqueued");
        return ORB_OK;
    }

    // the final classification and gather of the results
    void gather(int only_if_done) {
        hipLaunchKernelGGL(ba_classify_kernel, dim3((n_gather + 255) / 256), dim3(256), 0, st, b, dres.outlier,
                           res->edge_chi2 ? dres.chi2 : (double*)nullptr, (uint8_t*)nullptr, 0, dres.q, dres.t, dres.X,
                           only_if_done);
    }
    // the outlier classification between the loops (Optimizer.cc:644-670): levels + robust kernels off
    void classify_levels(int only_if_done) {
        hipLaunchKernelGGL(ba_classify_kernel, dim3((E + 255) / 256), dim3(256), 0, st, b, (uint8_t*)nullptr,
                           (double*)nullptr, d_level, 1, (double*)nullptr, (double*)nullptr,
                           (double*)nullptr, only_if_done);
    }

    // the structure's host part: the counts posted at entry, or here; else the whole build on the host
    void count_structure() {
        if (helper_wait.on) {
            C.helper.wait();
            helper_wait.on = false;
            dev_build = counts_ok;
        } else {
            dev_build = opt.try_counts() && build_structure_counts(P, N, pr->pose_fixed, pr->edge_point, pr->edge_pose, E, hs);
        }
        if (!dev_build) {
            const std::vector<uint8_t> level(E, 0);
            build_structure(P, N, level, pr->pose_fixed, pr->edge_point, pr->edge_pose, hs, opt.smode == "sorted");
        }
        tm.mark(dev_build ? "build_structure (counts)" : "build_structure");
    }

    int plan_solve() {
        D = 6 * hs.np;
        // reduced system: in LDS up to 21 free keyframes (D <= 128), else in HBM (ba_solve_global_kernel)
        glob = D > 128 || solve_lds_doubles(D) * 8 + 4096 > 160 * 1024;
        if (glob && hs.np > ORBBA_MAX_FREE_KEYFRAMES) {
            set_error("LocalBA: more than ORBBA_MAX_FREE_KEYFRAMES free keyframes in the local window");
            return ORB_EINVAL;
        }
        grid = glob && sch.grid_solve &&
               (opt.gba_solve == "grid" || (opt.gba_solve != "single" && hs.np >= GBA_GRID_MIN_FREE_KEYFRAMES));
        Dp = solve_dp(D);
        ldlt_lds = glob ? (size_t)3 * Dp * 8 : std::max<size_t>(solve_lds_doubles(D) * 8, 16);
        gg = dim3((hs.nl * 8 + 63) / 64);
        return ORB_OK;
    }

    // system buffers (carved before the structure upload, so that their clears and the control
    // block ride on the structure's fill launch)
    int carve_system(bool fresh, int iters) {
        const size_t nblk = hs.blk_i1.size();
        const SystemDims d{(size_t)hs.n_act, (size_t)hs.np, (size_t)hs.nl, nblk,
                           (size_t)(SB_SPLIT + 1) * (glob ? 36 * nblk : (size_t)D * D),   // + Hpp part
                           glob ? (grid ? ldlt_grid_doubles(D) : (size_t)Dp * (Dp + 1)) : 0};
        SystemLayout y;
        int rc;
        if ((rc = C.sys.reserve(y.carve(nullptr, d)))) return rc;
        y.carve(C.sys.as<char>(), d);
        b.J = y.J; b.W = y.W; b.Hll = y.Hll; b.Dinv = y.Dinv; b.bl = y.bl; b.Hpp = y.Hpp; b.bp = y.bp;
        b.S = y.S; b.Spart = y.Spart; b.blk_done = y.blk_done; b.bs = y.bs; b.x = y.x; b.rchi = y.rchi;
        b.part = y.part; b.Sg = y.Sg;
        d_wgpart = y.wgpart;
        if (grid) lg = ldlt_grid_carve(b.Sg, D, &b.ctl->done);
        if (!fresh) return ORB_OK;
        // (J needs no clearing: every linearising trial writes the entries that are read -- those of the
        // edges to free poses, zeros for a level-1 edge.  S / the part matrices are zero where no pose
        // pair block is, and the second optimize() keeps the structure, so they are cleared once.)
        if ((rc = glob ? fills.add(b.S, (size_t)D * D * 8, 0, st) : fills.add(b.Spart, d.spart_n * 8, 0, st)) ||
            (rc = fills.add(b.blk_done, nblk * 4, 0, st)))
            return rc;
        BACtl init{};   // the first optimize()'s control block (ba_ctl_start_kernel(iters, 0) on a zeroed block)
        init.done = iters <= 0 ? 1 : 0;
        init.need_lin = 1;
        init.iters_max = iters;
        fills.set_ctl(b.ctl, init);
        return ORB_OK;
    }

    // structure upload: the host-built arrays, then the four lists from the host or built on the device
    int upload_structure() {
        const int Ea = hs.n_act, np = hs.np, nl = hs.nl, nblk = (int)hs.blk_i1.size();
        const size_t nps = (size_t)hs.n_ps, npairs = (size_t)hs.n_pairs;
        const StructDims d{(size_t)P, (size_t)N, (size_t)Ea, (size_t)np, (size_t)nl, (size_t)nblk, nps, npairs, dev_build};
        StructLayout s, h;
        const size_t sbytes = s.carve(nullptr, d);
        int rc;
        if ((rc = C.structure.reserve(sbytes))) return rc;
        if ((rc = C.h_struct.ensure(sbytes))) return rc;
        s.carve(C.structure.as<char>(), d);
        h.carve(C.h_struct.ptr, d);
        auto put = [](int* dst, const std::vector<int>& src, size_t n) {
            if (n) std::memcpy(dst, src.data(), 4 * n);
        };
        put(h.hp, hs.hp, P);
        put(h.hl, hs.hl, N);
        put(h.pt_beg, hs.pt_beg, (size_t)nl + 1);
        put(h.pt_id, hs.pt_id, nl);
        put(h.ps_beg, hs.ps_beg, (size_t)np + 1);
        put(h.ps_id, hs.ps_id, np);
        put(h.blk_i1, hs.blk_i1, nblk);
        put(h.blk_i2, hs.blk_i2, nblk);
        put(h.blk_beg, hs.blk_beg, (size_t)nblk + 1);
        for (int k = 0; k < nblk; k++)
            if (hs.blk_i1[k] == hs.blk_i2[k]) h.blk_diag[hs.blk_i1[k]] = k;
        int4* const d_rec = reinterpret_cast<int4*>(s.pt_rec);
        int2* const d_bp = reinterpret_cast<int2*>(s.blk_pair);
        if (dev_build) {
            ORB_HIP_TRY(hipMemcpyAsync(C.structure.ptr, C.h_struct.ptr, s.small_bytes, hipMemcpyHostToDevice, st));
            if ((rc = fills.add(s.slot, 4 * (size_t)np * nl, 0xff, st)) || (rc = fills.flush(st))) return rc;
            if (Ea)
                hipLaunchKernelGGL(ba_struct_slots_kernel, dim3((Ea + 255) / 256), dim3(256), 0, st, b.ep, b.ek, s.hp, s.hl,
                                   Ea, nl, s.act, s.pt_slot, s.slot, d_rec);
            if (nblk && nl)
                hipLaunchKernelGGL(ba_struct_pairs_kernel, dim3(nblk), dim3(1024), 0, st, s.blk_i1, s.blk_i2, s.blk_beg,
                                   s.ps_beg, s.slot, nl, d_bp, s.ps_slot);
            ORB_HIP_TRY(hipGetLastError());
        } else {
            put(h.act, hs.act, Ea);
            put(h.pt_slot, hs.pt_slot, Ea);
            put(h.ps_slot, hs.ps_slot, nps);
            if (npairs) std::memcpy(h.blk_pair, hs.blk_pair.data(), 8 * npairs);
            ORB_HIP_TRY(hipMemcpyAsync(C.structure.ptr, C.h_struct.ptr, s.list_bytes, hipMemcpyHostToDevice, st));
        }
        b.Ea = Ea; b.np = np; b.nl = nl; b.nblk = nblk;
        b.act = s.act; b.hp = s.hp; b.hl = s.hl; b.pt_beg = s.pt_beg; b.pt_slot = s.pt_slot; b.pt_id = s.pt_id;
        b.ps_beg = s.ps_beg; b.ps_slot = s.ps_slot; b.ps_id = s.ps_id; b.blk_i1 = s.blk_i1; b.blk_i2 = s.blk_i2;
        b.blk_beg = s.blk_beg; b.blk_pair = d_bp; b.blk_diag = s.blk_diag; b.pt_rec = d_rec;
        if (Ea && !dev_build) hipLaunchKernelGGL(ba_rec_kernel, dim3((Ea + 255) / 256), dim3(256), 0, st, b);
        ORB_HIP_TRY(hipGetLastError());
        have_structure = true;
        return ORB_OK;
    }

    int raise_lds_limit() {
        return raise_solve_lds_limit(glob ? SOLVE_HBM : opt.solve256 ? SOLVE_LDS_256 : SOLVE_LDS_1024, device, ldlt_lds);
    }

    // the launches of one LM trial
    int enqueue_trial(LoopState& L) {
        hipLaunchKernelGGL(ba_iter_kernel, gg, dim3(64), 0, st, b);
        if (L.enq == 0) {   // first trial: computeLambdaInit needs Hpp before the Schur step
            hipLaunchKernelGGL(ba_pose_accum_kernel, dim3(b.np + 1), dim3(1024), 0, st, b);
            hipLaunchKernelGGL(ba_schur_point_kernel, gg, dim3(64), 0, st, b);
        }
        hipLaunchKernelGGL(ba_schur_block_kernel, dim3(b.nblk + 1 + b.np, SB_SPLIT), dim3(1024), 0, st, b, D,
                           L.enq == 0 ? 0 : 1, glob ? 0 : 1);
        if (grid) {
            ldlt_grid_enqueue_stage(lg, b.S, b.bs, st);
            ldlt_grid_enqueue_factor(lg, st);
            hipLaunchKernelGGL(ba_solve_grid_finish_kernel, dim3(1), dim3(1024), (size_t)lg.Dg * 8, st, b, lg, D);
        } else if (glob) hipLaunchKernelGGL(ba_solve_global_kernel, dim3(1), dim3(1024), ldlt_lds, st, b, D);
        else if (opt.solve256) hipLaunchKernelGGL(ba_solve_kernel<256>, dim3(1), dim3(256), ldlt_lds, st, b, D, 1);
        else hipLaunchKernelGGL(ba_solve_kernel<1024>, dim3(1), dim3(1024), ldlt_lds, st, b, D, opt.simd0_helpers);
        const int slot = L.enq % LOOKAHEAD;
        C.step_seq = C.next_seq();
        L.ids[slot] = C.step_seq;
        hipLaunchKernelGGL(ba_point_update_kernel, gg, dim3(64), 0, st, b, D, d_wgpart);
        hipLaunchKernelGGL(ba_decide_kernel, dim3(1), dim3(256), 0, st, b, C.d_ring + slot, L.ids[slot],
                           (const double*)d_wgpart, (int)gg.x);
        ORB_HIP_TRY(hipGetLastError());
        L.enq++;
        return ORB_OK;
    }

    // the call's last loop: once the steps in flight are all that can be needed (no retry),
    // the final gather goes right behind them, guarded on `done` -- the GPU need not wait for
    // the host to see the last snapshot (round 6: ~15 us per call)
    // (the first loop: the classification, which leaves the control block as it is, so steps
    // enqueued after it still run as the first loop's; loop 2's ctl_start stays host-driven)
    // Without a stop flag or test hook, the first loop also gets the second's ctl_start behind
    // its classification: then no step of the first loop is enqueued after them until every
    // step before them has reported (trans_spec), since a step run after a ctl_start that did
    // start the second loop would be taken for the second loop's.
    void enqueue_loop_end(LoopState& L) {
        if (!((L.last_loop ? n_gather : E) && L.enq > L.spec_at && !L.stop_sent &&
              L.enq - L.seen >= L.remaining() - opt.spec_slack))
            return;
        spec_launched[L.last_loop ? 1 : 0]++;
        if (L.last_loop) {
            gather(1);
        } else {
            classify_levels(1);
            if (!stop_flag && opt.stop_after < 0) {
                // (seq: the second loop's step 0)
                hipLaunchKernelGGL(ba_ctl_start_kernel, dim3(1), dim3(1), 0, st, b, sch.iters[1], 1, C.d_ring + 0,
                                   C.next_seq(), 1);
                L.trans_spec = true;
            }
        }
        L.spec_at = L.enq;
    }

    // wait for step `seen`'s snapshot (a step that runs always writes one), mirroring the
    // caller's stop flag into the device-visible word the decide kernel polls after every
    // trial; the stream is queried now and then so a failed launch cannot hang the host
    int wait_snapshot(LoopState& L) {
        const int slot = L.seen % LOOKAHEAD;
        auto t_q = std::chrono::steady_clock::now();
        while (__atomic_load_n(&C.h_ring[slot].seq, __ATOMIC_ACQUIRE) != L.ids[slot]) {
            if (stop_flag) __atomic_store_n(C.h_stop, *stop_flag ? 1 : 0, __ATOMIC_RELEASE);
            const auto now = std::chrono::steady_clock::now();
            if (now - t_q > std::chrono::microseconds(200)) {
                t_q = now;
                const hipError_t q = hipStreamQuery(st);
                if (q != hipSuccess && q != hipErrorNotReady) ORB_HIP_TRY(q);
                if (q == hipSuccess && __atomic_load_n(&C.h_ring[slot].seq, __ATOMIC_ACQUIRE) != L.ids[slot]) {
                    set_error("LocalBA: LM step finished without a control snapshot");
                    return ORB_EHIP;
                }
            }
        }
        L.last = C.h_ring[slot];
        L.seen++;
        L.fin = L.last.done != 0;
        return ORB_OK;
    }

    // The LM loop runs on the device (ba_decide_step advances it); the host keeps LOOKAHEAD
    // steps enqueued and reads each step's control snapshot from a pinned ring, so no trial
    // waits for a host round trip.  Steps enqueued past the end return immediately.
    int run_loop(LoopState& L) {
        if (!L.fresh && !started_ahead)   // (the first optimize()'s control block came with the fill launch; the
                                          // second's ctl_start may have been enqueued behind the first loop)
            hipLaunchKernelGGL(ba_ctl_start_kernel, dim3(1), dim3(1), 0, st, b, L.iters, have_classified ? 1 : 0,
                               C.d_ring + 0, C.next_seq(), 0);   // (seq: step 0's id, slot 0)
        const int max_steps = L.iters * 10;
        int rc;
        while (!L.fin) {
            // no trial past the ones that can still be needed: each completes at most one iteration, so
            // with as many in flight as iterations remain (the latest snapshot's), the next is enqueued
            // only if one of those turns out a retry (round 6: the call used to end behind up to
            // LOOKAHEAD no-op trials of 5 launches each)
            const int remaining = L.remaining();
            while (L.enq < max_steps && L.enq - L.seen < LOOKAHEAD && L.enq - L.seen < remaining &&
                   !(L.trans_spec && L.seen < L.spec_at))
                if ((rc = enqueue_trial(L))) return rc;
            enqueue_loop_end(L);
            if (L.seen == L.enq || L.stop_sent) break;
            if ((rc = wait_snapshot(L))) return rc;
            if (L.trans_spec && !L.fin && L.seen == L.spec_at) L.trans_spec = false;   // it did nothing: go on
            if (!L.fin && stopped() && !L.stop_sent) {   // force stop: end the loop after the steps in flight
                hipLaunchKernelGGL(ba_ctl_stop_kernel, dim3(1), dim3(1), 0, st, b);
                L.stop_sent = true;
            }
        }
        tm.mark("LM loop done");
        if (!L.fin) {   // loop cut short (step cap or force stop): the device state is authoritative
            ORB_HIP_TRY(hipStreamSynchronize(st));
            ORB_HIP_TRY(hipMemcpy(&L.last, b.ctl, sizeof(BACtl), hipMemcpyDeviceToHost));
        }
        // else: `last` is the final snapshot; the steps still queued return at once, stream-ordered
        // before anything the caller enqueues next.  The step that ended the loop is step `seen` - 1:
        // a speculative gather enqueued after it ran on the final state.
        if (L.fin && L.seen <= L.spec_at) {
            (L.last_loop ? gathered : leveled) = true;
            if (L.trans_spec) started_ahead = true;
        }
        return ORB_OK;
    }

    // ------------------------------------------------------------------ one optimize(iters)
    int optimize(int iters, int which, bool last_loop) {
        LoopState L{iters, !have_structure, last_loop};
        if (L.fresh) count_structure();
        res->iterations[which] = 0;
        res->chi2[which] = 0;
        // (the second optimize()'s level-0 edge count is on the device: ba_ctl_start_kernel ends the
        // loop at once when the classification left none)
        if (hs.n_act == 0 || hs.np + hs.nl == 0) return ORB_OK;
        int rc;
        if ((rc = plan_solve()) || (rc = carve_system(L.fresh, iters))) return rc;
        if (L.fresh && (rc = upload_structure())) return rc;
        if ((rc = fills.flush(st)) || (rc = raise_lds_limit())) return rc;
        tm.mark("structure upload enqueued");
        if ((rc = run_loop(L))) return rc;
        res->iterations[which] = L.last.iters_done;
        res->chi2[which] = L.last.chi_out;
        res->trials = L.last.trials;
        hook_stopped = hook_stopped || L.last.stopped;
        return ORB_OK;
    }

    // final gather, copy-out, scratch release, timing report
    int finish(bool ran) {
        int rc;
        if ((rc = fills.flush(st))) return rc;   // (a call that optimised nothing still classifies)
        if (n_gather && !gathered) {
            gather(0);
            ORB_HIP_TRY(hipGetLastError());
        }
        if (win) return finish_window(ran);
        ORB_HIP_TRY(hipStreamSynchronize(st));
        tm.mark("results copied");
        ResultLayout h;
        h.carve(C.h_res.ptr, P, N, E);
        std::memcpy(res->pose_t, h.t, 24 * (size_t)P);
        std::memcpy(res->points, h.X, 24 * (size_t)N);
        if (res->edge_outlier) {
            if (ran) std::memcpy(res->edge_outlier, h.outlier, E);
            else std::memset(res->edge_outlier, 0, E);
        }
        if (res->edge_chi2) std::memcpy(res->edge_chi2, h.chi2, 8 * (size_t)E);
        for (int i = 0; i < P; i++) {
            q_to_R(&h.q[4 * i], res->pose_R + 9 * i);
            if (res->pose_q) std::memcpy(res->pose_q + 4 * i, &h.q[4 * i], 32);
        }
        if (helper_wait.on) {   // (a call that optimised nothing never waited for the counts)
            C.helper.wait();
            helper_wait.on = false;
        }
        // the dense pair-block scratch (slot_of: nl x np ints, col: np x nl/64 words) of a very large window
        // is released rather than kept with the thread (C4 keeps its 0.3 MB)
        if (hs.slot_of.capacity() * sizeof(int) + hs.col.capacity() * sizeof(unsigned long long) > (8u << 20)) {
            std::vector<int>().swap(hs.slot_of);
            std::vector<unsigned long long>().swap(hs.col);
        }
        tm.mark("end");
        if (tm.on) {
            fprintf(stderr, "orbba loop ends enqueued ahead: first loop %d (used %d, ctl_start %d), second %d (used %d)\n",
                    spec_launched[0], leveled ? 1 : 0, started_ahead ? 1 : 0, spec_launched[1], gathered ? 1 : 0);
            tm.report();
        }
        return ORB_OK;
    }

    // a window's results: the gather's region and the rotations behind it, for the write-back enqueued next
    int finish_window(bool ran) {
        ResultLayout size;
        double* R = reinterpret_cast<double*>(C.res_dev.as<char>() + align_up(size.carve(nullptr, P, N, E), 256));
        if (ran && P) hipLaunchKernelGGL(ba_result_rotation_kernel, dim3((P + 255) / 256), dim3(256), 0, st, dres.q, R, P);
        ORB_HIP_TRY(hipGetLastError());
        win->outlier = dres.outlier;
        win->pose_R = R;
        win->pose_t = dres.t;
        win->points = dres.X;
        if (helper_wait.on) {
            C.helper.wait();
            helper_wait.on = false;
        }
        tm.mark("end");
        if (tm.on) tm.report();
        return ORB_OK;
    }

    int run() {
        int rc;
        if (!win && (rc = validate())) return rc;
        if ((rc = C.acquire(device))) return rc;
        st = win ? win_stream : C.st;
        *C.h_stop = stopped() ? 1 : 0;
        tm.mark("context");
        if (!win) post_counts();
        if ((rc = win ? stage_window() : stage_problem())) return rc;
        const bool ran = !stopped() && opt.stop_after != 0;   // Optimizer.cc:633-634: stop before optimising => nothing done
        res->ran = ran ? 1 : 0;
        if (ran) {
            if ((rc = optimize(sch.iters[0], 0, sch.loops == 1))) return rc;
            if (sch.loops == 2 && !stopped() && !hook_stopped) {   // doMore (:639-642)
                // tag outliers (level 1) and drop the robust kernels (:644-670)
                // (no host copy of the levels: the structure is not rebuilt and the device counts the
                // level-0 edges for ba_ctl_start_kernel)
                if (E && sch.classify) {
                    if (!leveled) classify_levels(0);
                    ORB_HIP_TRY(hipGetLastError());
                    have_classified = true;
                }
                tm.mark("classify enqueued");
                if ((rc = optimize(sch.iters[1], 1, true))) return rc;
            }
        }
        return finish(ran);
    }
};

thread_local HostStructure g_hs;   // capacity kept across calls


}  // namespace

// orbba_local_ba on a window gathered in HBM (orbbamap.hip calls it between its gather and its write-back): the call
// runs on `stream`, on the calling thread's current device.
int orbamd::orbba_run_window(BaWindowRun& r, const volatile int32_t* stop_flag, void* stream) {
    int dev = 0;
    ORB_HIP_TRY(hipGetDevice(&dev));
    orbba_problem pr{};
    pr.n_poses = r.n_local + r.n_fixed;
    pr.n_points = r.n_points;
    pr.n_edges = r.n_edges;
    BAOutputs o{};
    LocalBACall call(&pr, &o, LOCAL_BA_SCHEDULE, stop_flag, dev, g_ba, g_hs);
    call.win = &r;
    call.win_stream = (hipStream_t)stream;
    call.win_pr = &pr;
    const int rc = call.run();
    for (int k = 0; k < 2; k++) {
        r.iterations[k] = o.iterations[k];
        r.chi2[k] = o.chi2[k];
    }
    r.ran = o.ran;
    return rc;
}

extern "C" int orbba_local_ba(const orbba_problem* pr, orbba_result* res, const volatile int32_t* stop_flag,
                              int device) {
    ORB_CHECK_ARG(pr && res, "null argument");
    BAOutputs o{res->pose_R, res->pose_t, res->pose_q, res->points, res->edge_outlier, res->edge_chi2};
    const int rc = LocalBACall(pr, &o, LOCAL_BA_SCHEDULE, stop_flag, device, g_ba, g_hs).run();
    for (int k = 0; k < 2; k++) {
        res->iterations[k] = o.iterations[k];
        res->chi2[k] = o.chi2[k];
    }
    res->ran = o.ran;
    return rc;
}

// Optimizer::BundleAdjustment (Optimizer.cc:197-343): one optimize(n_iterations) over every edge, no
// classification; the same call, context and kernels as LocalBA under another schedule.
extern "C" int orbba_bundle_adjustment(const orbba_problem* pr, const orbba_gba_options* op, orbba_gba_result* res,
                                       const volatile int32_t* stop_flag, int device) {
    ORB_CHECK_ARG(pr && op && res, "null argument");
    ORB_CHECK_ARG(op->n_iterations >= 0 && op->n_iterations <= 1000, "n_iterations out of range");
    ORB_CHECK_ARG(op->stereo_rule == ORBBA_GBA_RULE_REFERENCE || op->stereo_rule == ORBBA_GBA_RULE_LOCAL,
                  "unknown stereo_rule");
    ORB_CHECK_ARG(res->pose_f && res->points_f && res->point_included, "null result buffers");
    ORB_CHECK_ARG(pr->n_edges <= 0 || pr->edge_point, "null edge_point");
    const BASchedule sch{1, {op->n_iterations, 0}, op->robust ? 1 : 0, op->stereo_rule, false, true};
    BAOutputs o{res->pose_R, res->pose_t, res->pose_q, res->points, nullptr, res->edge_chi2};
    res->iterations = res->trials = res->ran = 0;
    res->chi2 = 0;
    if (int rc = LocalBACall(pr, &o, sch, stop_flag, device, g_ba, g_hs).run()) return rc;
    res->iterations = o.iterations[0];
    res->trials = o.trials;
    res->chi2 = o.chi2[0];
    res->ran = o.ran;
    // FromSE3Quat / FromVector3d (Optimizer.cc:157-181): the estimates narrowed element by element
    const int P = pr->n_poses, N = pr->n_points;
    for (int i = 0; i < P; i++) {
        for (int k = 0; k < 9; k++) res->pose_f[12 * i + k] = (float)res->pose_R[9 * i + k];
        for (int k = 0; k < 3; k++) res->pose_f[12 * i + 9 + k] = (float)res->pose_t[3 * i + k];
    }
    for (size_t k = 0; k < 3 * (size_t)N; k++) res->points_f[k] = (float)res->points[k];
    // notIncludedMP (:285-289): a point without an edge never enters the system and keeps its position
    std::memset(res->point_included, 0, N);
    for (int e = 0; e < pr->n_edges; e++) res->point_included[pr->edge_point[e]] = 1;
    return ORB_OK;
}

extern "C" int orbba_debug_stamps(unsigned long long* out) {
#ifdef ORB_BA_STAMPS
    ORB_HIP_TRY(hipDeviceSynchronize());
    ORB_HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ba_stamps), 64 * 8));
    return ORB_OK;
#else
    (void)out;
    set_error("built without ORB_BA_STAMPS");
    return ORB_EINVAL;
#endif
}

// ldlt_grid.h alone: (A + 0) x = b for a dense symmetric A (D x D, row-major; the lower triangle is read), host
// memory, synchronous.  *ok = 0: a zero or non-finite pivot, x is not written.
extern "C" int orbba_debug_ldlt_grid(const double* A, const double* b, int D, double* x, int32_t* ok, int device) {
    ORB_CHECK_ARG(A && b && x && ok, "null argument");
    ORB_CHECK_ARG(D >= 1 && D <= 6 * ORBBA_MAX_FREE_KEYFRAMES, "D out of range");
    ORB_HIP_TRY(hipSetDevice(device));
    DevBuf in, ws;
    struct Free {
        DevBuf &a, &b;
        ~Free() { a.release(); b.release(); }
    } fr{in, ws};
    int rc;
    const size_t nA = (size_t)D * D;
    if ((rc = in.reserve((nA + D) * 8)) || (rc = ws.reserve(ldlt_grid_doubles(D) * 8))) return rc;
    ORB_HIP_TRY(hipMemcpy(in.ptr, A, nA * 8, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(in.as<double>() + nA, b, (size_t)D * 8, hipMemcpyHostToDevice));
    const LdltGrid g = ldlt_grid_carve(ws.as<double>(), D, nullptr);
    ldlt_grid_enqueue_stage(g, in.as<double>(), in.as<double>() + nA, nullptr);
    ldlt_grid_enqueue_factor(g, nullptr);
    hipLaunchKernelGGL(ldlt_grid_solve_kernel, dim3(1), dim3(1024), (size_t)g.Dg * 8, nullptr, g);
    ORB_HIP_TRY(hipGetLastError());
    int okv = 0;
    ORB_HIP_TRY(hipMemcpy(&okv, g.ok, 4, hipMemcpyDeviceToHost));
    *ok = okv;
    if (okv) ORB_HIP_TRY(hipMemcpy(x, g.y, (size_t)D * 8, hipMemcpyDeviceToHost));
    return ORB_OK;
}

namespace {

// What both solve debug entries share: device buffers of their own (freed on every return path) and a control block
// that lets the kernel run (done = 0) with the given lambda.
struct SolveDebug {
    DevBuf sys, ctl;
    ~SolveDebug() { sys.release(); ctl.release(); }
    int control(double lambda) {
        if (int rc = ctl.reserve(sizeof(BACtl))) return rc;
        BACtl c{};
        c.lambda = lambda;
        c.ok2 = -1;
        ORB_HIP_TRY(hipMemcpy(ctl.ptr, &c, sizeof c, hipMemcpyHostToDevice));
        return ORB_OK;
    }
    int result(const double* d_x, int D, double* x, int32_t* ok) {
        ORB_HIP_TRY(hipGetLastError());
        ORB_HIP_TRY(hipDeviceSynchronize());
        BACtl c;
        ORB_HIP_TRY(hipMemcpy(&c, ctl.ptr, sizeof c, hipMemcpyDeviceToHost));
        ORB_HIP_TRY(hipMemcpy(x, d_x, (size_t)D * 8, hipMemcpyDeviceToHost));
        *ok = c.ok2;
        return ORB_OK;
    }
};

// s_piece's sum of one entry's parts (orbba_solve.h), restated on the host in its order: part 0 + the Hpp part +
// lambda on the diagonal, then parts 1 ..
double s_piece_host(const double* part, double h, bool diag, double lam) {
    double v = 0.0;
    for (int k = 0; k < SB_SPLIT; k++) {
        double pk = part[k];
        if (k == 0) pk = (pk + h) + (diag ? lam : 0.0);
        v += pk;
    }
    return v;
}

// the lowest `bits` mantissa bits of a finite double cleared: a and a - chop(a) add up to a without rounding
double chop(double a, int bits) {
    uint64_t u;
    std::memcpy(&u, &a, 8);
    u &= ~((1ull << bits) - 1);
    std::memcpy(&a, &u, 8);
    return a;
}

}  // namespace

// ba_solve_kernel<1024> / <256> alone, the kernel LocalBA launches for D <= 128: A x = b for a dense symmetric A on a
// fabricated BADev without poses or points (the pose update behind the solve does nothing).  The kernel stages S from
// the part matrices, so A - lambda I is split here into SB_SPLIT + 1 of them that s_piece sums back to A bit for bit:
//   * small integers in the Hpp part (diagonal 6 x 6 pose blocks only) and in parts 1 .., part 0 taking the rest,
//     wherever that sum is exact (integer and other short-mantissa entries: every term of s_piece then matters);
//   * else the entry's mantissa cut in three (high bits in the Hpp part on a diagonal pose block, or in part 0; middle
//     bits in part 1; low bits in part 0), which is exact for lambda = 0;
//   * a non-finite entry goes to part 0 as it is.
// An entry neither split reproduces (a lambda that cannot be taken off the diagonal exactly) is an ORB_EINVAL.
extern "C" int orbba_debug_ldlt_lds(const double* A, const double* b, int D, double lambda, int threads,
                                    int simd0_helpers, double* x, int32_t* ok, int device) {
    ORB_CHECK_ARG(A && b && x && ok, "null argument");
    ORB_CHECK_ARG(D >= 2 && D <= 128 && D % 2 == 0, "D must be even, 2 .. 128");
    ORB_CHECK_ARG(threads == 1024 || threads == 256, "threads must be 1024 or 256");
    ORB_CHECK_ARG(simd0_helpers == 0 || simd0_helpers == 1, "simd0_helpers must be 0 or 1");
    ORB_CHECK_ARG(std::isfinite(lambda), "lambda must be finite");
    const size_t nA = (size_t)D * D;
    std::vector<double> parts((SB_SPLIT + 1) * nA, 0.0);
    for (int r = 0; r < D; r++)
        for (int c = 0; c < D; c++) {
            const size_t e = (size_t)r * D + c;
            const double want = A[e];
            const bool blk = r / 6 == c / 6, dg = r == c;
            double p[SB_SPLIT + 1] = {};   // p[SB_SPLIT]: the Hpp part
            auto good = [&] { return s_piece_host(p, p[SB_SPLIT], dg, lambda) == want; };
            if (!std::isfinite(want)) {
                p[0] = want;
            } else {
                const double a = dg ? want - lambda : want;
                // integers in [-4, 4] that depend on the position and on the part, nonzero on the diagonal
                auto noise = [&](int k) { return (double)((r * 7 + c * 13 + k * 5) % 9 - 4) + (dg ? 5.0 : 0.0); };
                double rest = a;
                if (blk) rest -= (p[SB_SPLIT] = noise(0));
                for (int k = 1; k < SB_SPLIT; k++) rest -= (p[k] = noise(k));
                p[0] = rest;
                if (!good()) {
                    for (int k = 0; k <= SB_SPLIT; k++) p[k] = 0.0;
                    const double hi = chop(a, 36), mid = chop(a - hi, 18), lo = (a - hi) - mid;
                    p[blk ? SB_SPLIT : 0] = hi;
                    p[0] += lo;
                    if (SB_SPLIT > 1) p[1] = mid;
                    else p[0] += mid;
                }
                if (!good()) {
                    set_error("orbba_debug_ldlt_lds: lambda cannot be taken off A's diagonal exactly");
                    return ORB_EINVAL;
                }
            }
            for (int k = 0; k <= SB_SPLIT; k++) parts[k * nA + e] = p[k];
        }
    ORB_HIP_TRY(hipSetDevice(device));
    SolveDebug dbg;
    int rc;
    if ((rc = dbg.control(lambda)) || (rc = dbg.sys.reserve((parts.size() + 2 * (size_t)D) * 8))) return rc;
    double* const d_parts = dbg.sys.as<double>();
    ORB_HIP_TRY(hipMemcpy(d_parts, parts.data(), parts.size() * 8, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(d_parts + parts.size(), b, (size_t)D * 8, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemset(d_parts + parts.size() + D, 0xff, (size_t)D * 8));
    BADev bd{};   // np = nl = 0: no pose is read or written
    bd.Spart = d_parts;
    bd.bs = d_parts + parts.size();
    bd.x = bd.bs + D;
    bd.ctl = dbg.ctl.as<BACtl>();
    const size_t lds = std::max<size_t>(solve_lds_doubles(D) * 8, 16);   // LocalBACall::plan_solve's
    if ((rc = raise_solve_lds_limit(threads == 256 ? SOLVE_LDS_256 : SOLVE_LDS_1024, device, lds))) return rc;
    if (threads == 256) hipLaunchKernelGGL(ba_solve_kernel<256>, dim3(1), dim3(256), lds, nullptr, bd, D, simd0_helpers);
    else hipLaunchKernelGGL(ba_solve_kernel<1024>, dim3(1), dim3(1024), lds, nullptr, bd, D, simd0_helpers);
    return dbg.result(bd.x, D, x, ok);
}

// ba_solve_global_kernel alone, LocalBA's kernel for D > 128, which reaches ldlt_hbm_solve as OptimizeEssentialGraph's
// eg_solve_kernel does (the padded system staged in HBM, y / dinv / vz in LDS): S = A, any D up to the pose graph's.
extern "C" int orbba_debug_ldlt_hbm(const double* A, const double* b, int D, double* x, int32_t* ok, int device) {
    ORB_CHECK_ARG(A && b && x && ok, "null argument");
    ORB_CHECK_ARG(D >= 1 && D <= 7 * (ORBBA_EG_MAX_KEYFRAMES - 1), "D out of range");
    ORB_HIP_TRY(hipSetDevice(device));
    const size_t nA = (size_t)D * D, Dp = solve_dp(D);
    SolveDebug dbg;
    int rc;
    if ((rc = dbg.control(0.0)) || (rc = dbg.sys.reserve((nA + 2 * (size_t)D + Dp * (Dp + 1)) * 8))) return rc;
    BADev bd{};
    bd.S = dbg.sys.as<double>();
    bd.bs = bd.S + nA;
    bd.x = bd.bs + D;
    bd.Sg = bd.x + D;
    bd.ctl = dbg.ctl.as<BACtl>();
    ORB_HIP_TRY(hipMemcpy(bd.S, A, nA * 8, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(bd.bs, b, (size_t)D * 8, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemset(bd.x, 0xff, (size_t)D * 8));
    const size_t lds = 3 * Dp * 8;   // LocalBACall::plan_solve's
    if ((rc = raise_solve_lds_limit(SOLVE_HBM, device, lds))) return rc;
    hipLaunchKernelGGL(ba_solve_global_kernel, dim3(1), dim3(1024), lds, nullptr, bd, D);
    return dbg.result(bd.x, D, x, ok);
}
