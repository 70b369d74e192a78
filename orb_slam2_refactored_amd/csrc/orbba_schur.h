// LocalBA, the reduced camera system's blocks S(i1, i2) and b_schur.
#pragma once

#include "orbba_linearize.h"

namespace orbamd {

// Reduced camera system block (i1, i2): 36 entries x 28 partial groups (two accumulators each),
// fixed-order combine.
// The pair list of a block is split into SB_SPLIT contiguous parts, one workgroup each (blockIdx.y),
// each storing its partial block (device-coherent stores, completed before it counts in); the last
// part of a block to count in adds the partials in part order and writes the block of S.
// Per free pose one more workgroup (blockIdx.x = nblk + 1 + i, part 0): with `accum` (every step but
// an optimize() call's first) on a linearising trial the Hpp / b_p sums of its pose (what
// ba_pose_accum_kernel would do), then b_schur = b_p - sum Hpp D^-1 b_l; it counts in on the pose's
// diagonal block as one more part, so the diagonal block's last arriver finds Hpp published and forms
// part 0 + Hpp + lambda I exactly as part 0 itself used to (same rounding).  Workgroup nblk: the chi2
// total.  (Round 3: the pose sums and b_schur ran inside the diagonal blocks' part 0, after its pair
// loop, on the kernel's critical path.)
constexpr int SB_G = 28;

// count in on block blk (expect arrivals in all); the last arriver forms the block of S
__device__ __forceinline__ void schur_block_count_in(const BADev& b, int blk, int D, int expect) {
    __shared__ int s_last;
    // Hand-off by the memory model: the partials' stores happen before thread 0's agent-scope
    // release (workgroup barrier), and the last part's agent-scope acquire happens before its loads
    // (the same barrier pattern on the consumer side).  Callers publish the partial from threads of
    // wavefront 0 only (the wavefront of the counting thread).
    __syncthreads();
    if (threadIdx.x == 0) {
        s_last = __hip_atomic_fetch_add(&b.blk_done[blk], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)expect - 1;
        if (s_last) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    if (s_last && threadIdx.x < 36) {
        const int i1 = b.blk_i1[blk], i2 = b.blk_i2[blk];
        const int r = threadIdx.x / 6, cc = threadIdx.x % 6;
        double v = 0;
        for (int k = 0; k < SB_SPLIT; k++) {
            double pk = b.Spart[((long long)k * b.nblk + blk) * 36 + threadIdx.x];
            if (k == 0 && i1 == i2) {   // part 0 + Hpp (the pose workgroup's part) + lambda I, in that order
                pk += b.Spart[((long long)SB_SPLIT * b.nblk + blk) * 36 + threadIdx.x];
                if (r == cc) pk += b.ctl->lambda;
            }
            v += pk;
        }
        b.S[(long long)(6 * i1 + r) * D + 6 * i2 + cc] = v;
        if (i1 != i2) b.S[(long long)(6 * i2 + cc) * D + 6 * i1 + r] = v;
        if (threadIdx.x == 0) __hip_atomic_store(&b.blk_done[blk], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ __launch_bounds__(1024) void ba_schur_block_kernel(BADev b, int D, int accum, int direct) {
    BA_RETURN_IF_DONE(b);
    __shared__ double sh[1024];
    __shared__ int sslot[PA_SLOTS];
    const int blk = blockIdx.x, part = blockIdx.y;
    const bool acc = accum && b.ctl->need_lin;
    if (blk == b.nblk) {
        if (acc && part == 0) chi_total(b, sh);
        return;
    }
    if (blk > b.nblk) {   // pose workgroup
        if (part != 0) return;
        const int i1 = blk - b.nblk - 1;
        stage_pose_slots(b, i1, sslot);   // the pose's edge slots (no dependent HBM loads below)
        __syncthreads();
        if (acc) {
            pose_accum(b, i1, sh, sslot);
            __syncthreads();   // b_p of this trial (global, this workgroup's stores) before b_schur
        }
        // b_schur for pose i1: 6 entries x 168 partial groups
        const int g2 = threadIdx.x / 6, c2 = threadIdx.x % 6;
        double s = 0;
        {
            const int beg = b.ps_beg[i1], end = b.ps_beg[i1 + 1];
            if (g2 < 168) {
                if (end - beg <= PA_SLOTS)
                    for (int u = beg + g2; u < end; u += 168) s += b.W[(long long)sslot[u - beg] * 24 + 18 + c2];
                else
                    for (int u = beg + g2; u < end; u += 168) s += b.W[(long long)b.ps_slot[u] * 24 + 18 + c2];
            }
        }
        sh[threadIdx.x] = g2 < 168 ? s : 0.0;
        __syncthreads();
        // two-level fixed-order sum of the 168 partials per entry (8 runs of 21, then the 8 run sums)
        // instead of one 168-long dependent chain on 6 threads
        double run = 0;
        if (threadIdx.x < 48) {
            const int e = threadIdx.x % 6, h = threadIdx.x / 6;
            for (int q = 21 * h; q < 21 * h + 21; q++) run += sh[q * 6 + e];
        }
        __syncthreads();
        if (threadIdx.x < 48) sh[threadIdx.x] = run;
        __syncthreads();
        if (threadIdx.x < 6) {
            double tot = 0;
            for (int h = 0; h < 8; h++) tot += sh[6 * h + threadIdx.x];
            b.bs[6 * i1 + threadIdx.x] = b.bp[6 * i1 + threadIdx.x] - tot;
        }
        // Hpp (this trial's or the kept one) as the diagonal block's extra part, republished by
        // wavefront 0 so that the counting wavefront's own release orders it
        if (direct) {   // the LDS solve sums the parts itself (no count-in)
            if (threadIdx.x < 36)
                b.Spart[((long long)SB_SPLIT * D + 6 * i1 + threadIdx.x / 6) * D + 6 * i1 + threadIdx.x % 6] =
                    b.Hpp[36 * i1 + threadIdx.x];
            return;
        }
        const int dblk = b.blk_diag[i1];
        if (threadIdx.x < 36) b.Spart[((long long)SB_SPLIT * b.nblk + dblk) * 36 + threadIdx.x] = b.Hpp[36 * i1 + threadIdx.x];
        schur_block_count_in(b, dblk, D, SB_SPLIT + 1);
        return;
    }
    const int i1 = b.blk_i1[blk], i2 = b.blk_i2[blk];
    const int g = threadIdx.x / 36, c = threadIdx.x % 36;
    const int r = c / 6, cc = c % 6;
    if (g < SB_G) {
        double s0 = 0, s1 = 0;
        const int pb = b.blk_beg[blk], pn = b.blk_beg[blk + 1] - pb;
        const int end = pb + (int)(((long long)pn * (part + 1)) / SB_SPLIT);
        int u = pb + (int)(((long long)pn * part) / SB_SPLIT) + g;
        for (; u + SB_G < end; u += 2 * SB_G) {
            const int2 p0 = b.blk_pair[u], p1 = b.blk_pair[u + SB_G];
            const double* W0 = b.W + (long long)p0.x * 24 + 3 * r;
            const double* H0 = b.J + (long long)p0.y * 72 + 54 + 3 * cc;
            const double* W1 = b.W + (long long)p1.x * 24 + 3 * r;
            const double* H1 = b.J + (long long)p1.y * 72 + 54 + 3 * cc;
            s0 += W0[0] * H0[0] + W0[1] * H0[1] + W0[2] * H0[2];
            s1 += W1[0] * H1[0] + W1[1] * H1[1] + W1[2] * H1[2];
        }
        if (u < end) {
            const int2 p0 = b.blk_pair[u];
            const double* W0 = b.W + (long long)p0.x * 24 + 3 * r;
            const double* H0 = b.J + (long long)p0.y * 72 + 54 + 3 * cc;
            s0 += W0[0] * H0[0] + W0[1] * H0[1] + W0[2] * H0[2];
        }
        sh[g * 36 + c] = s0 + s1;
    }
    __syncthreads();
    if (threadIdx.x < 36) {
        double s = 0;
        for (int q = 0; q < SB_G; q++) s += sh[q * 36 + threadIdx.x];
        if (direct) {   // part matrix `part`, both orientations (as S itself)
            double* Sp = b.Spart + (long long)part * D * D;
            Sp[(long long)(6 * i1 + r) * D + 6 * i2 + cc] = -s;
            if (i1 != i2) Sp[(long long)(6 * i2 + cc) * D + 6 * i1 + r] = -s;
        } else {
            b.Spart[((long long)part * b.nblk + blk) * 36 + threadIdx.x] = -s;
        }
    }
    if (!direct) schur_block_count_in(b, blk, D, i1 == i2 ? SB_SPLIT + 1 : SB_SPLIT);
}

}  // namespace orbamd
