// orbx_geom.h — what every extractor stage shares: the capacity constants, the per-level geometry the
// host builds once per image size (LevelDev / Geom / CellDev, passed to every kernel by value), and the
// lane / DPP / scan / XCD-swizzle helpers.  Part of orbx.hip's single translation unit.
#pragma once
#include <cstdint>

#include "common.h"

namespace orbamd {

constexpr int MAX_LEVELS = 16;
constexpr int MAX_ZONE = 64;            // max FAST detection-zone side (cellw <= 59 always)
constexpr int MAX_ROOTS = 32;
constexpr int PATCH = 43;               // raw neighbourhood: +-21 (rBRIEF reach 18 + blur 3)

__constant__ int c_umax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
constexpr int c_umax_h[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};   // compile-time copy
__constant__ int c_gauss[7] = {18, 34, 48, 56, 48, 34, 18};   // OpenCV 4.x bit-exact Q8 taps
// FAST circle (cv::FAST makeOffsets, pattern 16): compile-time so LDS reads use immediate offsets
constexpr int c_circle_dx_h[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
constexpr int c_circle_dy_h[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};

struct LevelDev {
    int w, h, stride;
    long long off;          // byte offset of this level in a frame's pyramid slab (l >= 1)
    int rx, ry, rw, rh;     // ROI = level inset by BORDER 16 (:755-760)
    int ncells, cell_base;
    long long cand_base;    // offset of this level's candidate array in a frame's slab
    int cand_cap;
    int quota, out_cap, out_base;
    int nroots;
    double hx;
    float scale, size;
    int xtab_off, ytab_off;         // resize coefficient tables (l >= 1)
    int tail_x;                     // first column of VResizeLinear's scalar tail (l >= 1; w: none)
    int mt_off;                     // first 16-column block in the matrix-core resize tables (-1: none)
    double ssx, ssy;                // (double)w[l-1] / w[l], (double)h[l-1] / h[l] (l >= 1)
};
// 128 bytes: g.lv[l] is a shift, and the kernels' scalar registers stay where round 4 had them (a
// 136-byte LevelDev made fast_cells' level indexing a multiply and moved its SGPR spills: +3.7 %)
static_assert(sizeof(LevelDev) == 128, "LevelDev stays 128 bytes");

struct Geom {
    int nlevels;
    int ncells_total;
    long long pyr_frame_bytes;
    long long slot_frame;     // candidate slots per frame (sum of per-cell capacities)
    long long cand_frame;     // contiguous candidate entries per frame
    int out_frame;            // selected keypoints per frame (sum of out_cap)
    unsigned of_m;            // n / out_frame = (t + ((n - t) >> of_s1)) >> of_s2, t = mulhi(n, of_m)
    int of_s1, of_s2;         // (round-up magic, exact for every n < 2^31; divmod_of)
    // describe's slot -> level: level q's first slot as u16 field q (q = 0 and unused levels 0x7fff);
    // the level of slot s is the number of fields <= s (SWAR, describe_level)
    unsigned lv_start[MAX_LEVELS / 2];
    LevelDev lv[MAX_LEVELS];
};

// n / g.out_frame for 0 <= n < 2^31 by the host's round-up magic (scalar multiply-high, no
// reciprocal round trip): the describe grid is out_frame selection slots per frame.
__device__ __forceinline__ int divmod_of(const Geom& g, int n) {
    const unsigned t = __umulhi((unsigned)n, g.of_m);
    return (int)((t + (((unsigned)n - t) >> g.of_s1)) >> g.of_s2);
}

// cell_cnt entries: the cell's kept corner count, plus a hint bit for fast_cells' next launch
constexpr int CELL_CNT_MASK = 0xffff, CELL_CNT_INI = 1 << 30;

struct CellDev {
    int level;
    int x0y0;     // x0 | y0 << 16 (crop origin, level coords)
    int zwzh;     // detection zone width | height << 16
    int slot;     // first slot (per-frame candidate-slot index)
};

// ------------------------------------------------------------------------------------------
// small device helpers
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int lane_id() { return threadIdx.x & 63; }
__device__ __forceinline__ unsigned long long lanemask_lt() {
    const int l = lane_id();
    return l == 0 ? 0ull : (~0ull >> (64 - l));
}
__device__ __forceinline__ int popc64(unsigned long long m) { return __popcll(m); }
// popc(m & lanemask_lt) without a lane mask held in VGPRs: v_mbcnt_lo / v_mbcnt_hi
__device__ __forceinline__ int rank64(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

__device__ __forceinline__ const uint8_t* level_base(const Geom& g, int l, int f, const uint8_t* in,
                                                      long long in_fstride, int in_step, const uint8_t* pyr,
                                                      int* step) {
    if (l == 0) {
        *step = in_step;
        return in + (long long)f * in_fstride;
    }
    *step = g.lv[l].stride;
    return pyr + (long long)f * g.pyr_frame_bytes + g.lv[l].off;
}

// Orders this wavefront's LDS accesses across lanes (LDS ops of one wave complete in order).
// XCD-aware block order: workgroups are dealt round-robin over the 8 XCDs (linear id % 8), each
// with its own 4 MiB L2.  Remap so XCD x runs one contiguous 1/8 of the logical blocks: neighbouring
// cells / tiles / keypoints of a frame then share that XCD's L2 for their overlapping rows instead
// of fetching the same 128-B lines from the fabric on several XCDs.  Bijective for any nb.
__device__ __forceinline__ int xcd_swizzle(int b, int nb) {
    const int q = nb >> 3, r = nb & 7, x = b & 7, k = b >> 3;
    return x < r ? x * (q + 1) + k : r * (q + 1) + (x - r) * q + k;
}

// Sum of an int over the 64 lanes, wave-uniform result: DPP within each row of 16 (quad xor 1, xor 2,
// row rotate 4, 8), then the four row sums by v_readlane.
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false); }
__device__ __forceinline__ int wave_sum_i32(int v) {
    v += dpp_i32<0xB1>(v);    // quad_perm [1,0,3,2]
    v += dpp_i32<0x4E>(v);    // quad_perm [2,3,0,1]
    v += dpp_i32<0x124>(v);   // row_ror:4
    v += dpp_i32<0x128>(v);   // row_ror:8
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) +
           __builtin_amdgcn_readlane(v, 48);
}

// v_writelane_b32 (the LLVM intrinsic; this clang has no builtin for it): a wave-uniform value into
// one lane of a register, with the compiler's own hazard handling
extern "C" __device__ uint32_t writelane_u32(uint32_t v, uint32_t lane, uint32_t old) __asm("llvm.amdgcn.writelane.i32");

__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// Wave-inclusive scan of ints (64 lanes) on DPP: Hillis-Steele inside each row of 16 (row_shr 1, 2,
// 4, 8 with zero fill), then row 1 / 3 add lane 15 of the row before (row_bcast:15) and rows 2 / 3
// add lane 31 (row_bcast:31).  No LDS round trips (a ds_bpermute scan costs six).
__device__ __forceinline__ int wave_incl_scan(int v) {
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);   // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);   // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);   // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);   // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 -> rows 1, 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 -> rows 2, 3
    return v;
}

// Block-wide exclusive scan for any blockDim.x that is a multiple of 64 (<= 8 waves). `tmp` >= 8 ints of LDS.
__device__ __forceinline__ int block_excl_scan(int v, int* tmp, int* total) {
    const int w = threadIdx.x >> 6, l = lane_id();
    const int inc = wave_incl_scan(v);
    if (l == 63) tmp[w] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    const int nw = blockDim.x >> 6;
    for (int i = 0; i < nw; i++) {
        if (i < w) base += tmp[i];
        tot += tmp[i];
    }
    __syncthreads();
    *total = tot;
    return base + inc - v;
}

// The quadtree's group primitives for its two forms: WV = false, the whole workgroup on one tree
// (workgroup barrier, block scan); WV = true (round 6), one wavefront per tree (no barrier: a wavefront
// runs in lockstep, so an LDS / global write is visible to the wavefront's next read once issued and
// the compiler is kept from reordering across the point; the fence orders global memory as the
// workgroup barrier's does).
template <bool WV>
__device__ __forceinline__ void qt_sync() {
    if constexpr (WV) {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    } else {
        __syncthreads();
    }
}
template <bool WV>
__device__ __forceinline__ int grp_excl_scan(int v, int* tmp, int* total) {
    if constexpr (WV) {
        const int inc = wave_incl_scan(v);
        *total = __builtin_amdgcn_readlane(inc, 63);
        return inc - v;
    } else {
        return block_excl_scan(v, tmp, total);
    }
}

}  // namespace orbamd
