// LocalBA, the rest of an LM trial and the loop's control: point update, decide (with the control
// snapshot to the host), loop start / stop, and the outlier classification.
#pragma once

#include "orbba_solve.h"

namespace orbamd {

// A point-update workgroup's chi2 / scale partials: its 8 points (group leaders, lanes 0, 8, .., 56)
// summed in order; ba_decide_kernel sums the workgroups' partials in a fixed order.
__device__ __forceinline__ void ba_point_update_partials(double* wgpart, double chi, double part) {
    double pc = 0, pp = 0;
#pragma unroll
    for (int g = 0; g < 64; g += GRP) {
        pc += readlane_d(chi, g);
        pp += readlane_d(part, g);
    }
    if (threadIdx.x == 0) {
        wgpart[2 * blockIdx.x] = pc;
        wgpart[2 * blockIdx.x + 1] = pp;
    }
}

// Back-substitution xl = Dinv (bl - Hpl^T xp), push(), point +=, scale term, then the errors and
// robust chi2 of the point's edges at the new estimate (computeActiveErrors after update()).
// The workgroups' chi2 / scale partials go to wgpart (ba_decide_kernel sums them).
__global__ __launch_bounds__(64) void ba_point_update_kernel(BADev b, int D, double* wgpart) {
    BA_RETURN_IF_DONE(b);
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int l = t / GRP, sub = t % GRP;
    const bool live = l < b.nl;
    double cl[3] = {0, 0, 0};
    if (live)
        for (int u = b.pt_beg[l] + sub; u < b.pt_beg[l + 1]; u += GRP) {
            const int4 rc = b.pt_rec[u];
            const int k = rc.x, ip = rc.w;
            if (ip < 0) continue;
            const double* Hpl = b.J + (long long)k * 72 + 54;
            for (int c = 0; c < 3; c++) {
                double s = 0;
                for (int r = 0; r < 6; r++) s += Hpl[3 * r + c] * b.x[6 * ip + r];
                cl[c] += s;
            }
        }
    for (int c = 0; c < 3; c++) cl[c] = grp_sum(cl[c]);
    double chi = 0, part = 0;   // every lane of a group ends with the same part
    if (live) {
        const double lam = b.ctl->lambda;
        double bl[3], xl[3];
        for (int c = 0; c < 3; c++) bl[c] = b.bl[3 * l + c];
        const double* Di = b.Dinv + 9 * l;
        for (int c = 0; c < 3; c++) cl[c] = bl[c] - cl[c];
        const int id = b.pt_id[l];
        double Xn[3];
        for (int i = 0; i < 3; i++) {
            xl[i] = Di[3 * i] * cl[0] + Di[3 * i + 1] * cl[1] + Di[3 * i + 2] * cl[2];
            Xn[i] = b.X[3 * id + i] + xl[i];
            part += xl[i] * (lam * xl[i] + bl[i]);
        }
        // every lane of the group read X before lane 0 overwrites it below (same wavefront, in order)
        __builtin_amdgcn_wave_barrier();
        if (sub == 0) {
            for (int i = 0; i < 3; i++) {
                b.x[D + 3 * l + i] = xl[i];
                b.X_sv[3 * id + i] = b.X[3 * id + i];
                b.X[3 * id + i] = Xn[i];
            }
            b.part[l] = part;
        }
        for (int u = b.pt_beg[l] + sub; u < b.pt_beg[l + 1]; u += GRP) {
            const int4 rc = b.pt_rec[u];
            const int e = rc.y;
            if (b.level[e]) continue;   // g2o computes active errors only: a level-1 edge keeps its _error
            const int pi = rc.z;
            double Xc[3];
            se3_map(b.q + 4 * pi, b.t + 3 * pi, Xn, Xc);
            chi += edge_error(b, e, Xc);
        }
    }
    // group partial (lanes of a group are contiguous; sum in fixed order via shuffles)
    chi += __shfl_xor(chi, 1, 64);
    chi += __shfl_xor(chi, 2, 64);
    chi += __shfl_xor(chi, 4, 64);
    if (live && sub == 0) b.rchi[l] = chi;
    ba_point_update_partials(wgpart, chi, part);
}

// The control snapshot into pinned host memory: the body as relaxed system-scope stores (write-through
// to the host), then the sequence id the host polls for as a system-scope RELEASE store, so the host's
// acquire load of `seq` (the host ring poll, wait_snapshot in orbba.hip) orders every body word before it by the
// memory model, not by the gfx9 rule that vmcnt(0) retires earlier stores (What's weak 8).
// On gfx950 the release compiles to `buffer_wbl2 sc0 sc1; s_waitcnt vmcnt(0)` before the seq store, a
// write-back of the whole L2 once per LM trial; against the relaxed round-3 form it cost nothing above
// the noise.
__device__ __forceinline__ void snapshot_to_host(const BACtl& snap, int seq, BACtl* host_snap) {
    static_assert(sizeof(BACtl) % 8 == 0, "snapshot copied as 8-byte words");
    const unsigned long long* src = reinterpret_cast<const unsigned long long*>(&snap);
    unsigned long long* dst = reinterpret_cast<unsigned long long*>(host_snap);
#pragma unroll
    for (int k = 0; k < (int)(sizeof(BACtl) / 8); k++)
        __hip_atomic_store(dst + k, src[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __hip_atomic_store(&host_snap->seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}

// levenberg.cpp:120-147 — accept / reject, lambda / nu update, then the trial / iteration bookkeeping
// of g2o's solve() / optimize(); one thread.  Returns whether the step was accepted.
__device__ bool ba_decide_step(const BADev& b, BACtl* host_snap, int seq, double tmp_sum, double scale_sum) {
    BACtl* c = b.ctl;
    c->tmp = tmp_sum;
    c->scale = scale_sum;
    double tmp = tmp_sum;
    if (!c->ok2) tmp = 1.7976931348623157e308;   // std::numeric_limits<double>::max()
    double rho = c->cur - tmp;
    rho /= (scale_sum + 1e-3);
    c->rho = rho;
    if (rho > 0 && isfinite(tmp)) {
        double alpha = 1. - pow((2 * rho - 1), 3);
        alpha = fmin(alpha, 2. / 3.);
        c->lambda *= fmax(1. / 3., alpha);
        c->ni = 2;
        c->cur = tmp;
        c->accepted = 1;
    } else {
        c->lambda *= c->ni;
        c->ni *= 2;
        c->accepted = 0;
    }
    // trial / iteration bookkeeping (host loop of levenberg solve + SparseOptimizer::optimize)
    c->q += 1;
    c->trials += 1;
    // g2o polls terminate() after every trial (levenberg.cpp:149) and before every iteration
    // (sparse_optimizer.cpp:376): a raised flag ends the loop once this trial is done
    const bool stop = (b.stop && __atomic_load_n(b.stop, __ATOMIC_RELAXED) != 0) ||
                      (b.stop_after >= 0 && c->trials >= b.stop_after);
    if (rho < 0 && c->q < 10 && !stop) {
        c->need_lin = 0;   // retry with the new lambda
    } else {
        c->iters_done += 1;
        c->chi_out = c->cur;
        bool term = c->q == 10 || rho == 0;
        if (!term) {
            if ((c->ini - c->cur) * 1e3 < c->ini) c->nbad++;
            else c->nbad = 0;
            term = c->nbad >= 3;
        }
        c->it += 1;
        if (c->it >= c->iters_max) term = true;
        if (stop) {
            term = true;
            c->stopped = 1;
        }
        if (term) c->done = 1;
        else {
            c->need_lin = 1;
            c->q = 0;
        }
    }
    // control snapshot straight into pinned host memory (no copy on the stream, no event).  (A
    // forwarder kernel on a side stream, so the decide kernel would not wait for the PCIe writes,
    // was slower: 1.73 -> 1.92 ms per C4 call.)
    BACtl snap = *c;
    snap.seq = -1;
    snapshot_to_host(snap, seq, host_snap);
    return c->accepted != 0;
}

// The decide step after a trial: fixed-order sums of the point-update workgroups' partials (thread-
// strided, then a fixed tree) + the pose scale terms of the solve, ba_decide_step on one thread, and
// pop() (restore the pushed estimates) on a rejected step.
__global__ __launch_bounds__(256) void ba_decide_kernel(BADev b, BACtl* host_snap, int seq, const double* wgpart,
                                                        int G) {
    BA_RETURN_IF_DONE(b);
    __shared__ double sc[256], sp[256];
    __shared__ int s_acc;
    const int tid = threadIdx.x;
    double c0 = 0, p0 = 0;
    for (int w = tid; w < G; w += 256) {
        c0 += wgpart[2 * w];
        p0 += wgpart[2 * w + 1];
    }
    for (int i = tid; i < b.np; i += 256) p0 += b.part[b.nl + i];
    sc[tid] = c0;
    sp[tid] = p0;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            sc[tid] += sc[tid + o];
            sp[tid] += sp[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) s_acc = ba_decide_step(b, host_snap, seq, sc[0], sp[0]);
    __syncthreads();
    if (s_acc) return;
    for (int t = tid; t < b.nl + b.np; t += 256) {   // pop(): restore the pushed estimates
        if (t < b.nl) {
            const int id = b.pt_id[t];
            for (int i = 0; i < 3; i++) b.X[3 * id + i] = b.X_sv[3 * id + i];
        } else {
            const int id = b.ps_id[t - b.nl];
            for (int j = 0; j < 4; j++) b.q[4 * id + j] = b.q_sv[4 * id + j];
            for (int j = 0; j < 3; j++) b.t[3 * id + j] = b.t_sv[3 * id + j];
        }
    }
}

// check_active (the second optimize()): with no level-0 edge left, g2o's optimize() has nothing to do
// (initializeOptimization(0) finds no active edge); the loop ends here and the snapshot the host waits
// for as step 0's (`seq` in ring slot `host_snap`) is written by this kernel, so the host never needs the
// classification on its side.
// only_if_done: enqueued speculatively behind the first loop (after its guarded classification); it
// starts the second loop only if the first has ended by then.
__global__ void ba_ctl_start_kernel(BADev b, int iters, int check_active, BACtl* host_snap, int seq, int only_if_done) {
    BACtl* c = b.ctl;
    if (only_if_done && !c->done) return;
    c->it = 0;
    c->q = 0;
    c->nbad = 0;
    const bool idle = check_active && c->n_active == 0;
    c->done = (iters <= 0 || idle) ? 1 : 0;
    c->maxdiag_bits = 0;
    c->need_lin = 1;
    c->iters_max = iters;
    c->iters_done = 0;
    c->chi_out = 0;
    c->rho = 0;
    if (idle) {
        BACtl snap = *c;
        snap.seq = -1;
        snapshot_to_host(snap, seq, host_snap);
    }
}

__global__ void ba_ctl_stop_kernel(BADev b) { b.ctl->done = 1; }

// final outlier classification (Optimizer.cc:644-670, :686-699) + chi2 out
// With rq / rt / rX (the final call) it also gathers the poses and points into the result region,
// so the results come back in one copy.
// only_if_done: the final gather enqueued speculatively behind the LM step the host expects to be the
// last; it does nothing unless the loop has ended by then (the host then enqueues another).
__global__ void ba_classify_kernel(BADev b, uint8_t* outlier, double* chi2o, uint8_t* level, int set_level,
                                   double* rq, double* rt, double* rX, int only_if_done) {
    if (only_if_done && !b.ctl->done) return;
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (rq && e < b.P) {
        for (int j = 0; j < 4; j++) rq[4 * e + j] = b.q[4 * e + j];
        for (int j = 0; j < 3; j++) rt[3 * e + j] = b.t[3 * e + j];
    }
    if (rX && e < b.N)
        for (int j = 0; j < 3; j++) rX[3 * e + j] = b.X[3 * e + j];
    uint8_t bad = 1;
    if (e < b.E) {
        const double maxc = b.stereo[e] ? 7.815 : 5.991;
        const double c = edge_chi2(b, e);
        double Xc[3];
        const int pi = b.ek[e];
        se3_map(b.q + 4 * pi, b.t + 3 * pi, b.X + 3 * b.ep[e], Xc);
        bad = (c > maxc || !(Xc[2] > 0.0)) ? 1 : 0;
        if (outlier) outlier[e] = bad;
        if (chi2o) chi2o[e] = c;
        if (set_level) {
            if (bad) level[e] = 1;
            b.robust[e] = 0;
        }
    }
    if (set_level) {   // the edges left at level 0 (the set_level launch covers E only: no early return above)
        const int n = __syncthreads_count(!bad);
        if (threadIdx.x == 0 && n) atomicAdd(&b.ctl->n_active, n);
    }
}

}  // namespace orbamd
