// LocalBA, once per call: the device half of the structure build, the point lists' entry records and
// the batched buffer fill.
#pragma once

#include "orbba_dev.h"

namespace orbamd {

// The point lists' entry records (once per call, after the structure): one 16-byte load per entry in
// the per-trial point kernels instead of the pt_slot -> act -> ek -> hp chain of dependent loads.  The
// host-built structure only; the device build writes them in ba_struct_slots_kernel.
__global__ __launch_bounds__(256) void ba_rec_kernel(BADev b) {
    const int u = blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= b.Ea) return;
    const int k = b.pt_slot[u], e = b.act[k], pi = b.ek[e];
    b.pt_rec[u] = make_int4(k, e, pi, b.hp[pi]);
}

// ---- Device half of the structure build (round 6; host half: ba_structure.h build_structure_counts).
// The (free pose, point) slot table, pose-major (row i: the edge of pose i at each point, -1 where
// none; memset to -1 first), the identity lists of the point-sorted case and their entry records.
__global__ void ba_struct_slots_kernel(const int* __restrict__ ep, const int* __restrict__ ek,
                                       const int* __restrict__ hp, const int* __restrict__ hl, int E, int nl,
                                       int* __restrict__ act, int* __restrict__ pt_slot, int* __restrict__ slot_of,
                                       int4* __restrict__ rec) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    act[e] = e;
    pt_slot[e] = e;
    const int pi = ek[e], h = hp[pi];
    rec[e] = make_int4(e, e, pi, h);
    if (h >= 0) slot_of[(long long)h * nl + hl[ep[e]]] = e;
}
// One workgroup per pose-pair block (i1, i2): the points with an edge to both, ascending, as (edge of
// i1, edge of i2) pairs -- build_structure's order; a diagonal block's first members are also the
// pose's edge list (ps_slot).  Ordered compaction 1024 points at a time (wave ballots + an LDS scan).
__global__ __launch_bounds__(1024) void ba_struct_pairs_kernel(const int* __restrict__ blk_i1,
                                                                const int* __restrict__ blk_i2,
                                                                const int* __restrict__ blk_beg,
                                                                const int* __restrict__ ps_beg,
                                                                const int* __restrict__ slot_of, int nl,
                                                                int2* __restrict__ blk_pair, int* __restrict__ ps_slot) {
    __shared__ int wsum[16];
    const int blk = blockIdx.x, i1 = blk_i1[blk], i2 = blk_i2[blk];
    const int* r1 = slot_of + (long long)i1 * nl;
    const int* r2 = slot_of + (long long)i2 * nl;
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    const int psd = i1 == i2 ? ps_beg[i1] - blk_beg[blk] : 0;   // ps_slot index - pair index
    int base = blk_beg[blk];
    for (int l0 = 0; l0 < nl; l0 += 1024) {
        const int l = l0 + threadIdx.x;
        int a = -1, c = -1;
        if (l < nl) {
            a = r1[l];
            c = r2[l];
        }
        const bool keep = a >= 0 && c >= 0;
        const unsigned long long bm = __ballot(keep);
        if (lane == 0) wsum[wv] = __popcll(bm);
        __syncthreads();
        int off = 0, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            const int v = wsum[w];
            off += w < wv ? v : 0;
            tot += v;
        }
        if (keep) {
            const int pos = base + off + __popcll(bm & below);
            blk_pair[pos] = make_int2(a, c);
            if (i1 == i2) ps_slot[pos + psd] = a;
        }
        base += tot;
        __syncthreads();
    }
}

// The call's buffer initialisations as ONE launch per batch instead of a hipMemsetAsync each (round 6:
// 11 memsets per call ran as 16 fill kernels of ~4.4 us, ~70 us of the call's GPU time in rocprofv3).
// Segments start 16-byte aligned (carve offsets are multiples of 256); a byte value replicated.
constexpr int BA_FILL_MAX = 8;
struct BAFill {
    void* p[BA_FILL_MAX];
    unsigned long long n[BA_FILL_MAX];
    unsigned v[BA_FILL_MAX];
    int cnt;
    BACtl* ctl;       // when set: the first optimize()'s control block, written whole (ba_ctl_start_kernel's
    BACtl ctl_init;   // job for that call, one launch earlier)
};
__global__ __launch_bounds__(256) void ba_fill_kernel(BAFill f) {
    const unsigned long long gt = blockIdx.x * 256ull + threadIdx.x, gs = gridDim.x * 256ull;
    if (f.ctl && gt < sizeof(BACtl) / 8)
        reinterpret_cast<unsigned long long*>(f.ctl)[gt] = reinterpret_cast<const unsigned long long*>(&f.ctl_init)[gt];
    for (int s = 0; s < f.cnt; s++) {
        uint8_t* p = static_cast<uint8_t*>(f.p[s]);
        const unsigned b = f.v[s] & 0xffu, w = b * 0x01010101u;
        const uint4 v4 = make_uint4(w, w, w, w);
        const unsigned long long nv = f.n[s] >> 4;
        for (unsigned long long i = gt; i < nv; i += gs) reinterpret_cast<uint4*>(p)[i] = v4;
        for (unsigned long long i = (nv << 4) + gt; i < f.n[s]; i += gs) p[i] = (uint8_t)b;
    }
}

}  // namespace orbamd
