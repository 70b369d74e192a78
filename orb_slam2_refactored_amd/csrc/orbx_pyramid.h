// orbx_pyramid.h — stage 1 of orbx.hip: cascaded cv::resize INTER_LINEAR 8U (src/ORBextractor.cc:455-470),
// level 0 being the caller's image.  pyramid_level_kernel builds one level, pyramid_pair_kernel two
// cascaded levels per launch (the default for the pairs that fit), pyramid_pair_mfma_kernel the pair with
// the horizontal pass on the matrix cores (ORBX_PYR_MFMA=1); with them the host-side table builders and
// capacity checks of the pair kernels.
#pragma once
#include <cmath>
#include <type_traits>
#include <vector>

#include "orbx_geom.h"
#include "orbx_pyr_rect.h"

namespace orbamd {

// cv::resize INTER_LINEAR CV_8UC1 [ext]: horizontal 11-bit fixed point (exact int32), vertical
// with the universal-intrinsics rounding ((b0*(S0>>4))>>16 + (b1*(S1>>4))>>16 + 2) >> 2 up to the
// level's tail_x and (S0*b0 + S1*b1 + 2^21) >> 22 from there.  Default tail mode 0: tail_x = w, the
// vector rounding on every column (OpenCV's uchar VResizeLinear specialisation uses it in its scalar
// tail too); the other modes are sensitivity switches (orbx_set_opencv_compat, oracle resize_tail_x).
// xtab[dx] = {sx0 | sx1 << 16, a0 | a1 << 16}; ytab[dy] = {sy0 | sy1 << 16, b0 | b1 << 16}.
// One workgroup = a 64 x 16 tile of level l (256 threads, 4 output pixels each).  The source
// rectangle of level l-1 it needs is staged in LDS with dword loads; coefficients come from the
// per-level tables.
typedef unsigned short us2 __attribute__((ext_vector_type(2)));   // packed u16 pair

// Vertical taps ((h >> 4) * b) >> 16 on the full-rate 24-bit multiplier: with h4 = (h >> 4) << 4
// (h < 2^20) and b12 = b << 12 (b <= 2048), mulhi(h4, b12) = ((h >> 4) * b * 2^16) >> 32, and the
// masks tell the compiler both operands fit in 24 bits (v_mul_hi_u32_u24 instead of the
// quarter-rate v_mul_hi_u32).
__device__ __forceinline__ uint32_t htap24(uint32_t h) { return h & 0xffff0u; }
// v_mul_hi_u32_u24 on operands the compiler cannot see are < 2^24 (table coefficients b << 12, the
// matrix-core pass's sums): no mask instruction to prove it
__device__ __forceinline__ uint32_t mulhi24(uint32_t a, uint32_t b) {
    uint32_t r;
    asm("v_mul_hi_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ uint32_t vcoef24(int b) { return ((uint32_t)b & 0xfffu) << 12; }
// VResizeLinear's scalar loop, FixedPtCast<int, uchar, 22>: (S0*b0 + S1*b1 + 2^21) >> 22 on the full
// horizontal sums (S < 2^20, b <= 2048: both products and the sum fit 32 bits); b24 = b << 12
__device__ __forceinline__ uint32_t vtail(uint32_t h0, uint32_t h1, uint32_t b0_24, uint32_t b1_24) {
    return (__umul24(h0, b0_24 >> 12) + __umul24(h1, b1_24 >> 12) + (1u << 21)) >> 22;
}

// two u8 taps of the 8-byte window (hi:lo) picked by a v_perm selector, as a packed u16 pair
__device__ __forceinline__ us2 pyr_tap(uint32_t hi, uint32_t lo, uint32_t sel) {
    const uint32_t r = __builtin_amdgcn_perm(hi, lo, sel);
    return *reinterpret_cast<const us2*>(&r);
}

// (tile and LDS capacities: orbx_pyr_rect.h)
// pyr_recip20 as a table: a workgroup's divisions by its piece / quad counts are one scalar load each
struct PyrRecipTab { unsigned m[PYR_RECIP_N]; };
constexpr PyrRecipTab pyr_recip_tab() {
    PyrRecipTab t{};
    for (int n = 1; n < PYR_RECIP_N; n++) t.m[n] = pyr_recip20(n);
    return t;
}
__constant__ PyrRecipTab c_pyr_recip = pyr_recip_tab();
static_assert(PYR_SW / 16 < PYR_RECIP_N, "the staging piece counts are in the table");

// A tile row's vertical taps, built once per workgroup (round 4): the byte offsets of its two source rows
// in the staged rectangle (first row sy_lo, row stride PYR_SW) and the two coefficients in mulhi24 form
// (b << 12), so a row costs one ds_read_b128 and the address adds instead of ~11 VALU of decoding.
__device__ __forceinline__ int4 pyr_row_taps(int2 yv, int sy_lo) {
    return make_int4(((yv.x & 0xffff) - sy_lo) * PYR_SW, ((yv.x >> 16) - sy_lo) * PYR_SW, (int)vcoef24(yv.y),
                     (int)vcoef24(yv.y >> 16));
}

// Level-l output tile (tx0, ty0, tw x th) from the staged source rectangle S (row stride PYR_SW,
// first byte column xa), the tile's column taps xs_t and its row taps ys_t (pyr_row_taps).  Every
// thread of the workgroup must call it (block-wide vote inside); no barrier follows the vote.
__device__ __forceinline__ void pyr_tile_compute(const Geom& g, const LevelDev& L, int f, uint8_t* pyr,
                                                 const uint8_t* S, const int2* xs_t, const int4* ys_t, int tx0,
                                                 int ty0, int tw, int th, int xa) {
    {
        // 16 threads per 64-px output row (4 px each: two pairs), 16 rows per pass (round 4: the row's
        // table read, address and loop control once per 4 pixels instead of 2).  Both pixels of a pair
        // have their four taps in the 8 LDS bytes from the pair's dword wd (scale <= ~3), so a pair costs
        // two dword reads per source row; v_perm packs a pixel's taps as u16 (S0, S1) and v_dot2_u32_u16
        // with the packed (a0, a1) gives S0*a0 + S1*a1 exactly.  (h >> 4 <= 32640 and the result <= 255:
        // OpenCV's saturations cannot trigger for coefficients summing to 2048.)
        const int q0 = (threadIdx.x & 15) * 4;
        uint32_t sel0[2], sel1[2];
        int wdb[2];
        us2 a0[2], a1[2];
        bool fits = true;
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int2 xv0 = xs_t[min(q0 + 2 * j, tw - 1)], xv1 = xs_t[min(q0 + 2 * j + 1, tw - 1)];
            const int s00 = (xv0.x & 0xffff) - xa, s01 = (xv0.x >> 16) - xa;
            const int s10 = (xv1.x & 0xffff) - xa, s11 = (xv1.x >> 16) - xa;
            const int wd = s00 >> 2;
            const int e00 = s00 - 4 * wd, e01 = s01 - 4 * wd, e10 = s10 - 4 * wd, e11 = s11 - 4 * wd;
            fits = fits && max(e01, e11) <= 7 && min(e00, e10) >= 0;
            sel0[j] = (uint32_t)e00 | 0x0c00u | ((uint32_t)e01 << 16) | 0x0c000000u;
            sel1[j] = (uint32_t)e10 | 0x0c00u | ((uint32_t)e11 << 16) | 0x0c000000u;
            wdb[j] = 4 * wd;
            a0[j] = *reinterpret_cast<const us2*>(&xv0.y);
            a1[j] = *reinterpret_cast<const us2*>(&xv1.y);
        }
        if (!__syncthreads_or(!fits)) {   // block-uniform: every thread's taps fit its 8-byte windows
            if (q0 >= tw) return;   // after the block-wide vote: no barrier follows
            const bool full = q0 + 3 < tw;
            uint8_t* dst = pyr + (long long)f * g.pyr_frame_bytes + L.off + tx0 + q0 +
                           (long long)(ty0 + (int)(threadIdx.x >> 4)) * L.stride;
            const long long dstep = 16ll * L.stride;
            // this thread's first column in the scalar tail (<= 0: all four, >= 4: none); the tail
            // loop is a separate instantiation, so columns left of tail_x run the plain loop
            const int tcol = L.tail_x - (tx0 + q0);
            auto rows = [&](auto tail_c) {
                constexpr bool TAIL = decltype(tail_c)::value;
                for (int ty = threadIdx.x >> 4; ty < th; ty += 16, dst += dstep) {
                    const int4 yv = ys_t[ty];
                    const uint32_t b0 = (uint32_t)yv.z, b1 = (uint32_t)yv.w;   // b << 12 (pyr_row_taps)
                    uint32_t out = 0;
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        const uint32_t* s0 = reinterpret_cast<const uint32_t*>(S + yv.x + wdb[j]);
                        const uint32_t* s1 = reinterpret_cast<const uint32_t*>(S + yv.y + wdb[j]);
                        const uint32_t w00 = s0[0], w01 = s0[1], w10 = s1[0], w11 = s1[1];
                        const uint32_t r0a = __builtin_amdgcn_udot2(pyr_tap(w01, w00, sel0[j]), a0[j], 0u, false);
                        const uint32_t r1a = __builtin_amdgcn_udot2(pyr_tap(w11, w10, sel0[j]), a0[j], 0u, false);
                        const uint32_t r0b = __builtin_amdgcn_udot2(pyr_tap(w01, w00, sel1[j]), a1[j], 0u, false);
                        const uint32_t r1b = __builtin_amdgcn_udot2(pyr_tap(w11, w10, sel1[j]), a1[j], 0u, false);
                        uint32_t va = (mulhi24(htap24(r0a), b0) + mulhi24(htap24(r1a), b1) + 2) >> 2;
                        uint32_t vb = (mulhi24(htap24(r0b), b0) + mulhi24(htap24(r1b), b1) + 2) >> 2;
                        if (TAIL) {
                            va = 2 * j >= tcol ? vtail(r0a, r1a, b0, b1) : va;
                            vb = 2 * j + 1 >= tcol ? vtail(r0b, r1b, b0, b1) : vb;
                        }
                        out |= (va | (vb << 8)) << (16 * j);
                    }
                    if (full) {
                        *reinterpret_cast<uint32_t*>(dst) = out;   // tx0 + q0 and the row stride: multiples of 4
                    } else {
                        for (int k = 0; k < 3; k++)
                            if (q0 + k < tw) dst[k] = (uint8_t)(out >> (8 * k));
                    }
                }
            };
            // block-uniform: only the tiles that reach the tail run the selecting loop (a per-thread choice
            // made the waves holding both kinds of lane run both loops)
            if (tx0 + tw > L.tail_x) rows(std::true_type{});
            else
                rows(std::false_type{});
            return;
        }
    }
    // generic path: 16 threads per 64-px output row segment (4 px each), 16 rows per pass
    const int q0 = (threadIdx.x & 15) * 4;
    if (q0 >= tw) return;
    // (cold path: the column coefficients are re-read from LDS per row to keep registers free for
    // pyramid_tiles_kernel's prefetch)
    uint8_t* dbase = pyr + (long long)f * g.pyr_frame_bytes + L.off + tx0 + q0;
#pragma nounroll
    for (int ty = threadIdx.x >> 4; ty < th; ty += 16) {
        const int4 yv = ys_t[ty];
        const int r0 = yv.x, r1 = yv.y;
        const int b0 = yv.z >> 12, b1 = yv.w >> 12;
        uint32_t packed = 0;
#pragma nounroll
        for (int k = 0; k < 4; k++) {
            const int2 xv = xs_t[min(q0 + k, tw - 1)];
            const int sx0 = (xv.x & 0xffff) - xa, sx1 = (xv.x >> 16) - xa, a0 = xv.y & 0xffff, a1 = xv.y >> 16;
            const int h0 = S[r0 + sx0] * a0 + S[r0 + sx1] * a1;
            const int h1 = S[r1 + sx0] * a0 + S[r1 + sx1] * a1;
            const int s0 = min(h0 >> 4, 32767), s1 = min(h1 >> 4, 32767);
            int v = (((s0 * b0) >> 16) + ((s1 * b1) >> 16) + 2) >> 2;
            if (tx0 + q0 + k >= L.tail_x) v = (h0 * b0 + h1 * b1 + (1 << 21)) >> 22;
            packed |= (uint32_t)(v > 255 ? 255 : v) << (8 * k);
        }
        uint8_t* dst = dbase + (long long)(ty0 + ty) * L.stride;
        if (q0 + 3 < tw) *reinterpret_cast<uint32_t*>(dst) = packed;   // stride % 16 == 0, tx0+q0 % 4 == 0
        else {   // q0 < tw <= q0 + 3
            dst[0] = (uint8_t)packed;
            if (q0 + 1 < tw) dst[1] = (uint8_t)(packed >> 8);
            if (q0 + 2 < tw) dst[2] = (uint8_t)(packed >> 16);
        }
    }
}

// 16-byte staging (every pyramid level; level 0 when the caller's base and step are multiples of
// 16): the source rectangle is fetched as 16-byte pieces with (row, piece) flattened over the 256
// threads, i.e. ~3 loads per thread instead of one dword load per source row.
// (PYR_PF 16-byte pieces per thread: rows x pieces <= 5 x 256)

struct PyrTile {
    int f, tx0, ty0, tw, th, sy_lo, xa, nc, items, mul;   // mul = ceil(2^20 / nc): row = item * mul >> 20
    const uint8_t* src;
    int sstep;
};

// (sx, sy: the source spans the tile's taps cover, pyr_tap_span)
__device__ __forceinline__ PyrTile pyr_tile_geom(const Geom& g, int l, int t, int ntx, int nty, PyrSpan sx, PyrSpan sy,
                                                 const uint8_t* in, long long in_fstride, int in_step, uint8_t* pyr) {
    const LevelDev& L = g.lv[l];
    PyrTile T;
    const int per = ntx * nty;
    T.f = t / per;
    const int r = t - T.f * per;
    T.ty0 = (r / ntx) * PYR_TH;
    T.tx0 = (r - (r / ntx) * ntx) * PYR_TW;
    T.tw = min(PYR_TW, L.w - T.tx0);
    T.th = min(PYR_TH, L.h - T.ty0);
    T.sy_lo = sy.lo;
    T.xa = sx.lo & ~15;
    T.nc = ((sx.hi - T.xa) >> 4) + 1;
    T.items = (sy.hi - sy.lo + 1) * T.nc;
    T.mul = (int)c_pyr_recip.m[T.nc];
    T.src = level_base(g, l - 1, T.f, in, in_fstride, in_step, pyr, &T.sstep);
    // workgroup-uniform by construction: keep the tile in SGPRs, not in VGPRs across the compute
    auto u = [](int x) { return __builtin_amdgcn_readfirstlane(x); };
    T.f = u(T.f), T.tx0 = u(T.tx0), T.ty0 = u(T.ty0), T.tw = u(T.tw), T.th = u(T.th), T.sy_lo = u(T.sy_lo);
    T.xa = u(T.xa), T.nc = u(T.nc), T.items = u(T.items), T.mul = u(T.mul), T.sstep = u(T.sstep);
    const unsigned long long sp = (unsigned long long)(uintptr_t)T.src;
    T.src = (const uint8_t*)(uintptr_t)(((unsigned long long)(unsigned)u((int)(sp >> 32)) << 32) |
                                        (unsigned)u((int)(unsigned)sp));
    return T;
}

// piece i -> (row, 16-byte column): rr = (i * mul) >> 20 as a 24-bit high product (i < 2^11,
// mul <= 2^20), c = i - rr * nc as a 24-bit product (full-rate multipliers)
__device__ __forceinline__ int pyr_piece_row(const PyrTile& T, int i) {
    return (int)(__umulhi(((unsigned)i & 0x7ffu) << 12, (unsigned)T.mul & 0xffffffu) & 0x7ffu);
}
__device__ __forceinline__ int mul12(int a, int b) {   // a, b in [0, 4096): one v_mul_u32_u24
    return (int)(((unsigned)a & 0xfffu) * ((unsigned)b & 0xfffu));
}
__device__ __forceinline__ void pyr_piece_load(const PyrTile& T, int i, uint4& v) {
    if (i < T.items) {
        const int rr = pyr_piece_row(T, i), c = i - mul12(rr, T.nc);
        v = *reinterpret_cast<const uint4*>(T.src + __mul24(T.sy_lo + rr, T.sstep) + T.xa + 16 * c);
    }
}

__device__ __forceinline__ void pyr_fetch(const PyrTile& T, int tid, uint4& v0, uint4& v1, uint4& v2, uint4& v3,
                                          uint4& v4) {
    static_assert(PYR_PF == 5, "five pieces per thread");
    pyr_piece_load(T, tid, v0);
    pyr_piece_load(T, tid + 256, v1);
    pyr_piece_load(T, tid + 512, v2);
    pyr_piece_load(T, tid + 768, v3);
    pyr_piece_load(T, tid + 1024, v4);
}

__device__ __forceinline__ void pyr_stage(const PyrTile& T, int tid, uint8_t* S, const uint4& v, int k) {
    const int i = tid + 256 * k;
    if (i < T.items) {
        const int rr = pyr_piece_row(T, i), c = i - mul12(rr, T.nc);
        *reinterpret_cast<uint4*>(&S[mul12(rr, PYR_SW) + 16 * c]) = v;
    }
}

__global__ __launch_bounds__(256) void pyramid_level_kernel(Geom g, int l, const uint8_t* __restrict__ in,
                                                            long long in_fstride, int in_step, uint8_t* pyr,
                                                            const int2* __restrict__ xtab,
                                                            const int2* __restrict__ ytab) {
    __shared__ __attribute__((aligned(16))) uint8_t S[PYR_SH * PYR_SW + 16];   // +16: the 8-byte windows may read past the last row
    __shared__ int2 xs_t[PYR_TW];
    __shared__ int4 ys_t[PYR_TH];
    const LevelDev& L = g.lv[l];
    const LevelDev& Ls = g.lv[l - 1];
    const int gx = gridDim.x, gxy = gridDim.x * gridDim.y;
    const int lb = xcd_swizzle(blockIdx.x + gx * blockIdx.y + gxy * blockIdx.z, gxy * gridDim.z);
    const int f = lb / gxy;
    const int tx0 = (lb % gx) * PYR_TW, ty0 = ((lb % gxy) / gx) * PYR_TH;
    const int tw = min(PYR_TW, L.w - tx0), th = min(PYR_TH, L.h - ty0);
    int sstep;
    const uint8_t* src = level_base(g, l - 1, f, in, in_fstride, in_step, pyr, &sstep);
    const int2* xt = xtab + L.xtab_off;
    const int2* yt = ytab + L.ytab_off;
    // the source rectangle the tile's taps cover, from the first and last entries of its table rows
    // (workgroup-uniform reads)
    const int sw = Ls.w;
    const PyrSpan sx = pyr_tap_span(xt, tx0, tx0 + tw - 1), sy = pyr_tap_span(yt, ty0, ty0 + th - 1);
    const int sx_lo = __builtin_amdgcn_readfirstlane(sx.lo), sx_hi = __builtin_amdgcn_readfirstlane(sx.hi);
    const int sy_lo = __builtin_amdgcn_readfirstlane(sy.lo), sy_hi = __builtin_amdgcn_readfirstlane(sy.hi);
    // coefficient tables -> LDS
    if ((int)threadIdx.x < tw) xs_t[threadIdx.x] = xt[tx0 + threadIdx.x];
    if ((int)threadIdx.x >= 64 && (int)threadIdx.x - 64 < th)
        ys_t[threadIdx.x - 64] = pyr_row_taps(yt[ty0 + threadIdx.x - 64], sy_lo);
    const int xa = sx_lo & ~3;
    const int nd = (sx_hi - xa + 4) >> 2;   // dwords per source row (<= PYR_SW / 4 < 64)
    const int nr = sy_hi - sy_lo + 1;
    const bool aligned = ((reinterpret_cast<uintptr_t>(src) | (uintptr_t)sstep) & 3) == 0;
    if (((reinterpret_cast<uintptr_t>(src) | (uintptr_t)sstep) & 15) == 0 && sx_hi - (sx_lo & ~15) < PYR_SW) {
        const PyrTile T = pyr_tile_geom(g, l, lb, gx, gridDim.y, PyrSpan{sx_lo, sx_hi}, PyrSpan{sy_lo, sy_hi}, in,
                                        in_fstride, in_step, pyr);
        uint4 v0, v1, v2, v3, v4;
        pyr_fetch(T, threadIdx.x, v0, v1, v2, v3, v4);
        pyr_stage(T, threadIdx.x, S, v0, 0);
        pyr_stage(T, threadIdx.x, S, v1, 1);
        pyr_stage(T, threadIdx.x, S, v2, 2);
        pyr_stage(T, threadIdx.x, S, v3, 3);
        pyr_stage(T, threadIdx.x, S, v4, 4);
        __syncthreads();
        pyr_tile_compute(g, L, f, pyr, S, xs_t, ys_t, tx0, ty0, tw, th, T.xa);
        return;
    }
    if (aligned) {
        // wavefront w stages rows w, w + 4, ...; lane = dword of the row.  The row address is
        // wave-uniform (SGPR base + a per-lane column offset), so a load costs no VALU; all of a
        // lane's loads are issued before the LDS stores.
        constexpr int RPW = PYR_SH / 4;
        const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
        const int ln = threadIdx.x & 63;
        const int col = min(xa + 4 * ln, (sw - 1) & ~3);   // in-row dword (row stride >= align4(w))
        const uint8_t* rbase = src + (long long)sy_lo * sstep + col;
        uint32_t v[RPW];
#pragma unroll
        for (int k = 0; k < RPW; k++) {   // unconditional (row clamped): straight-line loads
            const int rk = min(wv + 4 * k, nr - 1);
            v[k] = *reinterpret_cast<const uint32_t*>(rbase + (long long)rk * sstep);
        }
        if (ln < nd) {
            uint32_t* drow = reinterpret_cast<uint32_t*>(S) + wv * (PYR_SW / 4) + ln;
#pragma unroll
            for (int k = 0; k < RPW; k++)
                if (wv + 4 * k < nr) drow[k * PYR_SW] = v[k];   // row wv + 4k: (wv + 4k) * PYR_SW / 4 dwords
        }
    } else {   // unaligned caller image (level 0 with an odd base / step): byte loads
        for (int i = threadIdx.x; i < nd * nr; i += blockDim.x) {
            const int r = i / nd, d = i - r * nd;
            const uint8_t* rowp = src + (long long)(sy_lo + r) * sstep;
            const int x = xa + 4 * d;
            uint32_t v = 0;
            for (int q = 0; q < 4; q++)
                if (x + q < sw) v |= (uint32_t)rowp[x + q] << (8 * q);
            *reinterpret_cast<uint32_t*>(&S[r * PYR_SW + 4 * d]) = v;
        }
    }
    __syncthreads();
    pyr_tile_compute(g, L, f, pyr, S, xs_t, ys_t, tx0, ty0, tw, th, xa);
}

// Two cascaded levels in one launch: level l (from level l-1, both in the pyramid slab) and level
// l+1, one workgroup per 64x64 tile of level l+1.  The workgroup computes the level-l rectangle
// its tile's taps cover (pyr_pair_rect: read from the tap tables, columns from a dword boundary)
// from a staged level-(l-1) rectangle, keeps it in LDS for the level-(l+1) tile and writes it to
// the slab.  Neighbouring workgroups' rectangles overlap where both tiles tap a pixel; they write
// the same bytes there.  Removes the launch boundary between the two levels and the level-l
// re-read.  NP: the level-l row passes the host found over every tile of the pair (pyr_pair_fits).

__device__ __forceinline__ uint32_t pyr_px_generic(const uint8_t* S, int2 xv, int4 yv, int xa, bool tail) {
    const int r0 = yv.x, r1 = yv.y;
    const int sx0 = (xv.x & 0xffff) - xa, sx1 = (xv.x >> 16) - xa, a0 = xv.y & 0xffff, a1 = xv.y >> 16;
    const int b0 = yv.z >> 12, b1 = yv.w >> 12;
    const int h0 = S[r0 + sx0] * a0 + S[r0 + sx1] * a1;
    const int h1 = S[r1 + sx0] * a0 + S[r1 + sx1] * a1;
    const int s0 = min(h0 >> 4, 32767), s1 = min(h1 >> 4, 32767);
    int v = (((s0 * b0) >> 16) + ((s1 * b1) >> 16) + 2) >> 2;
    if (tail) v = (h0 * b0 + h1 * b1 + (1 << 21)) >> 22;
    return (uint32_t)(v > 255 ? 255 : v);
}

template <int NP>
__global__ __launch_bounds__(256) void pyramid_pair_kernel(Geom g, int l, const uint8_t* __restrict__ in,
                                                           long long in_fstride, int in_step, uint8_t* pyr,
                                                           const int2* __restrict__ xtab,
                                                           const int2* __restrict__ ytab) {
    __shared__ __attribute__((aligned(16))) uint8_t S[PYR_SH * PYR_SW + 16];
    __shared__ int2 xs1[PP_MAXC], xs2[PYR_TW];
    __shared__ int4 ys1[PP_MAXR], ys2[PYR_TH];
    const LevelDev& L1 = g.lv[l];
    const LevelDev& L2 = g.lv[l + 1];
    const int tid = threadIdx.x;
    const int gx = gridDim.x, gxy = gridDim.x * gridDim.y;
    const int lb = xcd_swizzle(blockIdx.x + gx * blockIdx.y + gxy * blockIdx.z, gxy * gridDim.z);
    const int f = lb / gxy;
    const int tx0 = (lb % gx) * PYR_TW, ty0 = ((lb % gxy) / gx) * PYR_TH;
    const int tw = min(PYR_TW, L2.w - tx0), th = min(PYR_TH, L2.h - ty0);
    auto u = [](int x) { return __builtin_amdgcn_readfirstlane(x); };
    // level-l rectangle [c0, c1] x [ay0, ay1] (c0 dword aligned) and the level-(l-1) rectangle for it,
    // staged as 16-byte pieces: workgroup-uniform reads of the tables' first / last entries
    const PyrPairRect R = pyr_pair_rect(xtab + L1.xtab_off, ytab + L1.ytab_off, xtab + L2.xtab_off,
                                        ytab + L2.ytab_off, tx0, ty0, tw, th);
    const int c0 = u(R.c0), c1 = u(R.c1), ay0 = u(R.ay0), ay1 = u(R.ay1);
    const int ncol = c1 - c0 + 1, nrow = ay1 - ay0 + 1;
    PyrTile T;
    T.sy_lo = u(R.by0);
    T.xa = u(R.xa);
    T.nc = u(((R.bx1 - R.xa) >> 4) + 1);
    T.items = u((R.by1 - R.by0 + 1) * T.nc);
    T.mul = u((int)c_pyr_recip.m[T.nc]);
    T.src = level_base(g, l - 1, f, in, in_fstride, in_step, pyr, &T.sstep);   // 16-byte aligned (host)
    {
        uint4 v0, v1, v2, v3, v4;
        pyr_fetch(T, tid, v0, v1, v2, v3, v4);
        if (tid < ncol) xs1[tid] = xtab[L1.xtab_off + c0 + tid];
        if (tid < nrow) ys1[tid] = pyr_row_taps(ytab[L1.ytab_off + ay0 + tid], T.sy_lo);
        if (tid < tw) xs2[tid] = xtab[L2.xtab_off + tx0 + tid];
        if (tid < th) ys2[tid] = pyr_row_taps(ytab[L2.ytab_off + ty0 + tid], ay0);
        pyr_stage(T, tid, S, v0, 0);
        pyr_stage(T, tid, S, v1, 1);
        pyr_stage(T, tid, S, v2, 2);
        pyr_stage(T, tid, S, v3, 3);
        pyr_stage(T, tid, S, v4, 4);
    }
    __syncthreads();
    // level l: thread = (quad q of 4 columns, first row r0), rows r0 + p * rpp; tid / ncq by the
    // table's reciprocal (exact for tid <= 2048), rpp = 256 / ncq likewise
    const int ncq = (ncol + 3) >> 2;
    const unsigned m20 = (unsigned)u((int)c_pyr_recip.m[ncq]);
    const int rpp = (int)(m20 >> 12);
    const int r0 = (int)(__umul24((unsigned)tid, m20) >> 20), q = tid - __mul24(r0, ncq);
    const bool act = r0 < rpp;
    uint32_t out[NP];
    if (act) {
        uint32_t sel0[2], sel1[2], wdv[2];
        us2 a0[2], a1[2];
        int2 xv[4];
        bool fits = true;
#pragma unroll
        for (int k = 0; k < 4; k++) xv[k] = xs1[min(4 * q + k, ncol - 1)];
#pragma unroll
        for (int j = 0; j < 2; j++) {
            const int2 xv0 = xv[2 * j], xv1 = xv[2 * j + 1];
            const int s00 = (xv0.x & 0xffff) - T.xa, s01 = (xv0.x >> 16) - T.xa;
            const int s10 = (xv1.x & 0xffff) - T.xa, s11 = (xv1.x >> 16) - T.xa;
            const int wd = s00 >> 2;
            const int e00 = s00 - 4 * wd, e01 = s01 - 4 * wd, e10 = s10 - 4 * wd, e11 = s11 - 4 * wd;
            fits = fits && max(e01, e11) <= 7 && min(e00, e10) >= 0;
            sel0[j] = (uint32_t)e00 | 0x0c00u | ((uint32_t)e01 << 16) | 0x0c000000u;
            sel1[j] = (uint32_t)e10 | 0x0c00u | ((uint32_t)e11 << 16) | 0x0c000000u;
            wdv[j] = (uint32_t)wd;
            a0[j] = *reinterpret_cast<const us2*>(&xv0.y);
            a1[j] = *reinterpret_cast<const us2*>(&xv1.y);
        }
        // this thread's first level-l column in the scalar tail (<= 0: all four, >= 4: none)
        const int tcol = L1.tail_x - (c0 + 4 * q);
        auto rows = [&](auto tail_c) {
            constexpr bool TAIL = decltype(tail_c)::value;
#pragma unroll
            for (int pp = 0; pp < NP; pp++) {
                const int r = r0 + pp * rpp;
                out[pp] = 0;
                // workgroup-uniform: the pass is empty / every row of it exists (the per-thread row
                // test runs on the rectangle's last pass only)
                if (pp * rpp >= nrow) break;
                if ((pp + 1) * rpp > nrow && r >= nrow) break;
                const int4 yv = ys1[r];
                if (fits) {
                    const uint32_t b0 = (uint32_t)yv.z, b1 = (uint32_t)yv.w;   // b << 12 (pyr_row_taps)
#pragma unroll
                    for (int j = 0; j < 2; j++) {
                        const uint32_t* s0 = reinterpret_cast<const uint32_t*>(S + yv.x + 4 * (int)wdv[j]);
                        const uint32_t* s1 = reinterpret_cast<const uint32_t*>(S + yv.y + 4 * (int)wdv[j]);
                        const uint32_t w00 = s0[0], w01 = s0[1], w10 = s1[0], w11 = s1[1];
                        const uint32_t r0a = __builtin_amdgcn_udot2(pyr_tap(w01, w00, sel0[j]), a0[j], 0u, false);
                        const uint32_t r1a = __builtin_amdgcn_udot2(pyr_tap(w11, w10, sel0[j]), a0[j], 0u, false);
                        const uint32_t r0b = __builtin_amdgcn_udot2(pyr_tap(w01, w00, sel1[j]), a1[j], 0u, false);
                        const uint32_t r1b = __builtin_amdgcn_udot2(pyr_tap(w11, w10, sel1[j]), a1[j], 0u, false);
                        uint32_t va = (mulhi24(htap24(r0a), b0) + mulhi24(htap24(r1a), b1) + 2) >> 2;
                        uint32_t vb = (mulhi24(htap24(r0b), b0) + mulhi24(htap24(r1b), b1) + 2) >> 2;
                        if (TAIL) {
                            va = 2 * j >= tcol ? vtail(r0a, r1a, b0, b1) : va;
                            vb = 2 * j + 1 >= tcol ? vtail(r0b, r1b, b0, b1) : vb;
                        }
                        out[pp] |= (va | (vb << 8)) << (16 * j);
                    }
                } else {   // taps outside the 8-byte windows (not at the supported scale factors)
#pragma unroll
                    for (int k = 0; k < 4; k++) out[pp] |= pyr_px_generic(S, xv[k], yv, T.xa, k >= tcol) << (8 * k);
                }
            }
        };
        if (c1 >= L1.tail_x) rows(std::true_type{});   // block-uniform, as in pyr_tile_compute
        else
            rows(std::false_type{});
    }
    __syncthreads();   // every read of the level-(l-1) rectangle done: S now takes the level-l one
    if (act) {
        uint8_t* lrow = pyr + (long long)f * g.pyr_frame_bytes + L1.off + c0 + 4 * q;
        // columns past c1 hold clamped-coefficient values: never written to the slab (a
        // neighbouring workgroup writes the true ones there)
        const bool full = c0 + 4 * q + 3 <= c1;
#pragma unroll
        for (int pp = 0; pp < NP; pp++) {
            const int r = r0 + pp * rpp;
            if (pp * rpp >= nrow) break;
            if ((pp + 1) * rpp > nrow && r >= nrow) break;
            *reinterpret_cast<uint32_t*>(&S[r * PYR_SW + 4 * q]) = out[pp];
            uint8_t* dst = lrow + __mul24(ay0 + r, L1.stride);
            if (full) {
                *reinterpret_cast<uint32_t*>(dst) = out[pp];
            } else {
                for (int k = 0; k < 3; k++)
                    if (c0 + 4 * q + k <= c1) dst[k] = (uint8_t)(out[pp] >> (8 * k));
            }
        }
    }
    __syncthreads();
    pyr_tile_compute(g, L2, f, pyr, S, xs2, ys2, tx0, ty0, tw, th, c0);
}

// Host check of pyramid_pair_kernel for the pair (l, l+1): the kernel's geometry replayed for every
// tile from the host's copy of the tap tables (pyr_pair_plan).  Returns the NP to launch (the pass
// count rounded up to an instantiated one), 0 when a tile exceeds a capacity.
static int pyr_pair_fits(const Geom& g, int l, const std::vector<int2>& xtab, const std::vector<int2>& ytab) {
    const LevelDev &L0 = g.lv[l - 1], &L1 = g.lv[l], &L2 = g.lv[l + 1];
    const PyrPairPlan P = pyr_pair_plan(L0.w, L0.h, L1.w, L1.h, L2.w, L2.h, xtab.data() + L1.xtab_off,
                                        ytab.data() + L1.ytab_off, xtab.data() + L2.xtab_off, ytab.data() + L2.ytab_off);
    if (!P.ok) return 0;
    return P.passes <= 7 ? 7 : PP_MAXP;
}

// ---- the level pair with the horizontal pass on the matrix cores (round 5) ----
// VResizeLinear's horizontal sums for a block of 16 output columns (M) and 16 source rows (N) are
// one v_mfma_f32_16x16x32_f16 over K = 32 source columns from kb (the block's first tap rounded
// down to a dword):
//   A[m][k] = a0 at k = sx0 - kb, a1 at k = sx1 - kb (integers <= 2049: exact in f16),
//   B[k][n] = 1024 + pixel (the byte under an f16 0x64 high byte: one v_perm per two pixels),
//   C[m]    = 2^23 - 1024 (a0 + a1).
// Every partial sum is an integer below 2^24, so D = 2^23 + (S0 a0 + S1 a1) exactly and its float
// bits carry the horizontal sum in bits 0..19 (h < 2^19).  A source row's sums are computed once
// (the VALU form computes them for each of the ~1.7 output rows that read the row) into a
// per-wavefront ring of 48 rows; the vertical taps stay on the VALU (their per-term truncation is
// not a product).  A and C come from a per-level table built on the host (one 2 KiB entry per
// 16-column block); a wavefront owns one block at a time, so the ring needs no workgroup barrier.
typedef _Float16 h8v __attribute__((ext_vector_type(8)));
typedef float pf4v __attribute__((ext_vector_type(4)));
struct PyrMfmaLane { uint32_t a[4]; float c[4]; };   // one lane's A fragment (8 f16) and C (4 f32)
constexpr int PM_MAXB1 = 6;      // level-l rectangle blocks (96 columns)
constexpr int PM_TAB = PYR_SH;   // per-source-row table entries (rows of S)
constexpr int PM_MAXU1 = 12;     // level-l units (block, 15-row group) per wavefront


// One unit: source rows 15 k .. 15 k + 15 of S (16 rows, the last shared with the next group) x a
// 16-column block.  The product leaves lane (n, g) with the horizontal sums of source row 15 k + n,
// columns 4 g .. 4 g + 3; at scale factors >= 1 a source row is the upper tap sy0 of at most one
// output row, so lane n (n < 15) computes that output row from its own sums and lane n + 1's (DPP
// row_shl:1) -- the vertical pass needs no exchange through LDS.  sp: this lane's S address of
// group 0 (kb - S's first column + 8 g + n * PYR_SW); tab[r] = {byte offset of r's output row in the
// output level (-1: none), b0 << 12, b1 << 12, the row in the rectangle}.  Returns the lane's 4 pixels
// (meaningful when tab[15 k + n].x >= 0 and n < 15).
template <bool TAIL>
__device__ __forceinline__ uint32_t pyr_mfma_unit(const uint8_t* sp, int k, const h8v& A, const pf4v& C, const int4& t,
                                                  int tcol) {
    const int g = lane_id() >> 4;
    constexpr uint32_t hmask = TAIL ? 0xfffffu : 0xffff0u;   // the tail's formula needs the full sum
    const uint2 w = *reinterpret_cast<const uint2*>(sp + k * (15 * PYR_SW));
    const uint4 bu = make_uint4(__builtin_amdgcn_perm(0x64646464u, w.x, 0x04010400u),
                                __builtin_amdgcn_perm(0x64646464u, w.x, 0x04030402u),
                                __builtin_amdgcn_perm(0x64646464u, w.y, 0x04010400u),
                                __builtin_amdgcn_perm(0x64646464u, w.y, 0x04030402u));
    const pf4v d = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, __builtin_bit_cast(h8v, bu), C, 0, 0, 0);
    const uint32_t b0 = (uint32_t)t.y, b1 = (uint32_t)t.z;
    uint32_t out = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t h0 = __float_as_uint(d[j]) & hmask;
        const uint32_t h1 = (uint32_t)__builtin_amdgcn_mov_dpp((int)h0, 0x101, 0xf, 0xf, true);   // row_shl:1 (lane 15: 0)
        uint32_t v;
        if (!TAIL) {
            v = (mulhi24(h0, b0) + mulhi24(h1, b1) + 2) >> 2;
        } else {
            v = (mulhi24(h0 & 0xffff0u, b0) + mulhi24(h1 & 0xffff0u, b1) + 2) >> 2;
            v = 4 * g + j >= tcol ? vtail(h0, h1, b0, b1) : v;
        }
        out |= v << (8 * j);
    }
    return out;
}

// A block's A / C fragments from the host table
__device__ __forceinline__ void pyr_mfma_frag(const PyrMfmaLane* tab, h8v& A, pf4v& C) {
    const PyrMfmaLane t = tab[lane_id()];
    A = __builtin_bit_cast(h8v, make_uint4(t.a[0], t.a[1], t.a[2], t.a[3]));
    C = pf4v{t.c[0], t.c[1], t.c[2], t.c[3]};
}

// The per-source-row table of pyr_mfma_unit: output rows [r0, r0 + nrow) of a level (row stride
// ostride) whose source rows start at S row 0 = sy_lo.  Thread y fills source rows sy0(y) ..
// sy0(y + 1) - 1 (thread 0 also the rows above sy0(0), the last thread the rows to PM_TAB).
__device__ __forceinline__ void pyr_mfma_tab(const int2* ytab, int r0, int nrow, int sy_lo, int ostride, int4* tab) {
    const int y = threadIdx.x;
    if (y < nrow) {
        const int2 v = ytab[r0 + y];
        const int s0 = (v.x & 0xffff) - sy_lo;
        const int s0n = y + 1 < nrow ? (ytab[r0 + y + 1].x & 0xffff) - sy_lo : PM_TAB;
        if (y == 0)
            for (int r = 0; r < s0; r++) tab[r] = make_int4(-1, 0, 0, -1);
        tab[s0] = make_int4((r0 + y) * ostride, (int)vcoef24(v.y), (int)vcoef24(v.y >> 16), y);
        for (int r = s0 + 1; r < min(s0n, PM_TAB); r++) tab[r] = make_int4(-1, 0, 0, -1);
    }
}

// 4 output pixels (one dword) at byte column col of a row; partial at the right edge (last: the
// last column that may be written)
__device__ __forceinline__ void pyr_store4(uint8_t* dst, uint32_t o, int col, int last) {
    if (col + 3 <= last) *reinterpret_cast<uint32_t*>(dst) = o;
    else
        for (int k = 0; k < 3; k++)
            if (col + k <= last) dst[k] = (uint8_t)(o >> (8 * k));
}

__global__ __launch_bounds__(256) void pyramid_pair_mfma_kernel(Geom g, int l, const uint8_t* __restrict__ in,
                                                                long long in_fstride, int in_step, uint8_t* pyr,
                                                                const int2* __restrict__ ytab,
                                                                const PyrMfmaLane* __restrict__ mt,
                                                                const int* __restrict__ mkb) {
    __shared__ __attribute__((aligned(16))) uint8_t S[PYR_SH * PYR_SW + 16];
    __shared__ int4 tab1[PM_TAB], tab2[PM_TAB];
    const LevelDev& L0 = g.lv[l - 1];
    const LevelDev& L1 = g.lv[l];
    const LevelDev& L2 = g.lv[l + 1];
    const int tid = threadIdx.x;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int gx = gridDim.x, gxy = gridDim.x * gridDim.y;
    const int lb = xcd_swizzle(blockIdx.x + gx * blockIdx.y + gxy * blockIdx.z, gxy * gridDim.z);
    const int f = lb / gxy;
    const int tx0 = (lb % gx) * PYR_TW, ty0 = ((lb % gxy) / gx) * PYR_TH;
    const int tw = min(PYR_TW, L2.w - tx0), th = min(PYR_TH, L2.h - ty0);
    auto u = [](int x) { return __builtin_amdgcn_readfirstlane(x); };
    // level-l rectangle [c0, c1] x [ay0, ay1], c0 on a 16-column block boundary
    const int ax0 = max(0, (int)floor((tx0 + 0.5) * L2.ssx - 0.5) - 2);
    const int c1 = u(min(L1.w - 1, (int)floor((tx0 + tw - 0.5) * L2.ssx - 0.5) + 2));
    const int ay0 = u(max(0, (int)floor((ty0 + 0.5) * L2.ssy - 0.5) - 2));
    const int ay1 = u(min(L1.h - 1, (int)floor((ty0 + th - 0.5) * L2.ssy - 0.5) + 2));
    const int c0 = u(ax0 & ~15);
    const int ncol = c1 - c0 + 1, nrow = ay1 - ay0 + 1;
    PyrTile T;
    const int bx0 = max(0, (int)floor((c0 + 0.5) * L1.ssx - 0.5) - 2);
    const int bx1 = min(L0.w - 1, (int)floor((c1 + 0.5) * L1.ssx - 0.5) + 2);
    T.sy_lo = u(max(0, (int)floor((ay0 + 0.5) * L1.ssy - 0.5) - 2));
    const int by1 = u(min(L0.h - 1, (int)floor((ay1 + 0.5) * L1.ssy - 0.5) + 2));
    T.xa = u(bx0 & ~15);
    T.nc = u(((bx1 - T.xa) >> 4) + 1);
    T.items = u((by1 - T.sy_lo + 1) * T.nc);
    T.mul = u(((1 << 20) + T.nc - 1) / T.nc);
    T.src = level_base(g, l - 1, f, in, in_fstride, in_step, pyr, &T.sstep);   // 16-byte aligned (host)
    // at the level's last row the lower tap is clipped to the upper one (sy1 = sy0): S row sy0 + 1
    // then holds a copy of the last row, so the lane below always supplies the lower tap
    const int rep1 = by1 == L0.h - 1 ? by1 - T.sy_lo : -1;
    {
        uint4 v0, v1, v2, v3, v4;
        pyr_fetch(T, tid, v0, v1, v2, v3, v4);
        pyr_mfma_tab(ytab + L1.ytab_off, ay0, nrow, T.sy_lo, (int)L1.stride, tab1);
        pyr_mfma_tab(ytab + L2.ytab_off, ty0, th, ay0, (int)L2.stride, tab2);
        auto stage = [&](const uint4& v, int k) {
            const int i = tid + 256 * k;
            if (i < T.items) {
                const int rr = pyr_piece_row(T, i), c = i - mul12(rr, T.nc);
                *reinterpret_cast<uint4*>(&S[mul12(rr, PYR_SW) + 16 * c]) = v;
                if (rr == rep1) *reinterpret_cast<uint4*>(&S[mul12(rr + 1, PYR_SW) + 16 * c]) = v;
            }
        };
        stage(v0, 0);
        stage(v1, 1);
        stage(v2, 2);
        stage(v3, 3);
        stage(v4, 4);
    }
    __syncthreads();
    const int n = tid & 15, q = (tid >> 4) & 3;
    // level l: units (block b, group k) block-major, a contiguous range per wavefront; the rows
    // stay in registers until every wavefront is done reading the level-(l-1) rectangle
    const int nb1 = (ncol + 15) >> 4;
    const int g1 = u(((ytab[L1.ytab_off + ay1].x & 0xffff) - T.sy_lo) / 15 + 1);   // groups to the last output's sy0
    const int nu1 = nb1 * g1;
    const int ub = (nu1 * w) >> 2, ue = (nu1 * (w + 1)) >> 2;
    uint32_t o1[PM_MAXU1];
    uint8_t* lbase = pyr + (long long)f * g.pyr_frame_bytes + L1.off + c0 + 4 * q;
    {
        int cur = -1;
        h8v A;
        pf4v C;
        const uint8_t* sp = S;
        int tcol = 16;
#pragma unroll
        for (int i = 0; i < PM_MAXU1; i++) {
            const int un = ub + i;
            if (un >= ue) break;
            const int b = un / g1, k = un - b * g1;
            if (b != cur) {   // wavefront-uniform
                cur = b;
                const int blk = L1.mt_off + ((c0 >> 4) + b);
                pyr_mfma_frag(mt + (long long)blk * 64, A, C);
                sp = S + (mkb[blk] - T.xa + 8 * q + n * PYR_SW);
                tcol = L1.tail_x - (c0 + 16 * b);
            }
            const int4 t = tab1[15 * k + n];   // < PM_TAB (host check)
            o1[i] = tcol < 16 ? pyr_mfma_unit<true>(sp, k, A, C, t, tcol) : pyr_mfma_unit<false>(sp, k, A, C, t, tcol);
            const int col = c0 + 16 * b + 4 * q;
            if (t.x >= 0 && n < 15 && col <= c1) pyr_store4(lbase + 16 * b + t.x, o1[i], col, c1);
        }
    }
    __syncthreads();   // every read of the level-(l-1) rectangle done: S now takes the level-l one
    const int rep2 = ay1 == L1.h - 1 ? nrow - 1 : -1;
#pragma unroll
    for (int i = 0; i < PM_MAXU1; i++) {
        const int un = ub + i;
        if (un >= ue) break;
        const int b = un / g1, k = un - b * g1;
        const int4 t = tab1[15 * k + n];
        if (t.x >= 0 && n < 15) {
            *reinterpret_cast<uint32_t*>(&S[t.w * PYR_SW + 16 * b + 4 * q]) = o1[i];
            if (t.w == rep2) *reinterpret_cast<uint32_t*>(&S[(t.w + 1) * PYR_SW + 16 * b + 4 * q]) = o1[i];
        }
    }
    __syncthreads();
    // level l+1: wavefront w takes block w of the 64-column tile, all its groups
    if (16 * w < tw) {
        const int bc = tx0 + 16 * w;
        const int blk = L2.mt_off + (bc >> 4);
        h8v A;
        pf4v C;
        pyr_mfma_frag(mt + (long long)blk * 64, A, C);
        const uint8_t* sp = S + (mkb[blk] - c0 + 8 * q + n * PYR_SW);
        const int col = bc + 4 * q;
        const int tcol = L2.tail_x - bc;
        const int g2 = u(((ytab[L2.ytab_off + ty0 + th - 1].x & 0xffff) - ay0) / 15 + 1);
        uint8_t* dbase = pyr + (long long)f * g.pyr_frame_bytes + L2.off + col;
        const int last = tx0 + tw - 1;
        auto run = [&](auto tail_c) {
            constexpr bool TAIL = decltype(tail_c)::value;
            for (int k = 0; k < g2; k++) {
                const int4 t = tab2[15 * k + n];
                const uint32_t o = pyr_mfma_unit<TAIL>(sp, k, A, C, t, tcol);
                if (t.x >= 0 && n < 15 && col <= last) pyr_store4(dbase + t.x, o, col, last);
            }
        };
        if (tcol < 16) run(std::true_type{});
        else run(std::false_type{});
    }
}

// f16 bits of an integer 0 <= v <= 2048 (exact: at most 11 significant bits)
static uint16_t f16_of_int(int v) {
    if (v <= 0) return 0;
    int e = 0;
    while ((2 << e) <= v) e++;   // v in [2^e, 2^(e+1))
    const int m = e >= 10 ? (v - (1 << e)) >> (e - 10) : (v - (1 << e)) << (10 - e);
    return (uint16_t)(((e + 15) << 10) | m);
}

// A / C fragments of pyramid_pair_mfma_kernel for one level's columns (xt: its xtab entries, dw
// columns), appended to mt / mkb; returns the level's first block, or -1 when a block's taps do
// not fit K = 32 from its dword-aligned first tap (scale factors above ~1.7).
static int pyr_mfma_tables(const int2* xt, int dw, std::vector<PyrMfmaLane>& mt, std::vector<int>& mkb) {
    const int nb = (dw + 15) / 16;
    std::vector<PyrMfmaLane> lanes((size_t)nb * 64);
    std::vector<int> kbs(nb);
    for (int j = 0; j < nb; j++) {
        const int kb = (xt[16 * j].x & 0xffff) & ~7;   // 8-byte aligned: the B fragments are ds_read_b64
        kbs[j] = kb;
        for (int ln = 0; ln < 64; ln++) {
            PyrMfmaLane& t = lanes[(size_t)j * 64 + ln];
            const int c = 16 * j + (ln & 15), gq = ln >> 4;
            uint16_t hv[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            if (c < dw) {
                const int sx0 = xt[c].x & 0xffff, sx1 = xt[c].x >> 16, a0 = xt[c].y & 0xffff, a1 = xt[c].y >> 16;
                const int e0 = sx0 - kb, e1 = sx1 - kb;
                if (e0 < 0 || e1 < e0 || e1 > 31 || a0 < 0 || a1 < 0 || a0 + a1 > 4096) return -1;
                for (int k = 0; k < 8; k++) {
                    const int kk = 8 * gq + k;
                    const int wv = (kk == e0 ? a0 : 0) + (kk == e1 ? a1 : 0);
                    if (wv > 2048) return -1;
                    hv[k] = f16_of_int(wv);
                }
            }
            for (int k = 0; k < 4; k++) t.a[k] = (uint32_t)hv[2 * k] | ((uint32_t)hv[2 * k + 1] << 16);
            for (int r = 0; r < 4; r++) {
                const int cm = 16 * j + 4 * gq + r;
                const int sum = cm < dw ? (xt[cm].y & 0xffff) + (xt[cm].y >> 16) : 0;
                t.c[r] = (float)(8388608 - 1024 * sum);
            }
        }
    }
    const int off = (int)mkb.size();
    mt.insert(mt.end(), lanes.begin(), lanes.end());
    mkb.insert(mkb.end(), kbs.begin(), kbs.end());
    return off;
}

// pyramid_pair_mfma_kernel's geometry replayed for every tile of the pair (l, l+1): the staged
// rectangles fit S, every block's K window lies inside S's rows, one output row per source row, and
// the 15-row groups (and their tables) inside S.
static bool pyr_mfma_pair_fits(const Geom& g, int l, const std::vector<int>& mkb, const std::vector<int2>& ytab) {
    const LevelDev &L0 = g.lv[l - 1], &L1 = g.lv[l], &L2 = g.lv[l + 1];
    if (L1.mt_off < 0 || L2.mt_off < 0) return false;
    auto fl = [](double v) { return (int)std::floor(v); };
    int max_rows = 0, max_nc = 0, max_nb1 = 0, max_g1 = 0;
    for (int ty0 = 0; ty0 < L2.h; ty0 += PYR_TH) {
        const int th = std::min(PYR_TH, L2.h - ty0);
        const int ay0 = std::max(0, fl((ty0 + 0.5) * L2.ssy - 0.5) - 2);
        const int ay1 = std::min(L1.h - 1, fl((ty0 + th - 0.5) * L2.ssy - 0.5) + 2);
        const int nrow = ay1 - ay0 + 1;
        const int sy_lo = std::max(0, fl((ay0 + 0.5) * L1.ssy - 0.5) - 2);
        const int by1 = std::min(L0.h - 1, fl((ay1 + 0.5) * L1.ssy - 0.5) + 2);
        if (nrow > PP_MAXR || by1 - sy_lo + 1 > PYR_SH) return false;
        max_rows = std::max(max_rows, by1 - sy_lo + 1);
        max_g1 = std::max(max_g1, ((ytab[L1.ytab_off + ay1].x & 0xffff) - sy_lo) / 15 + 1);
        // per output row: sy0 strictly increasing (one output row per source row), sy1 = sy0 + 1 except
        // at the level's last row (clipped: S holds a copy there); the groups' rows and the copy in S
        auto rows_ok = [&](const LevelDev& L, const LevelDev& Ls, int r0, int nr, int lo, int staged) {
            int prev = -1;
            for (int y = 0; y < nr; y++) {
                const int2 v = ytab[L.ytab_off + r0 + y];
                const int s0 = (v.x & 0xffff) - lo, s1 = (v.x >> 16) - lo;
                if (s0 <= prev || s0 < 0 || !(s1 == s0 + 1 || (s1 == s0 && (v.x >> 16) == Ls.h - 1))) return false;
                if (s1 >= staged) return false;
                prev = s0;
            }
            const int groups = prev / 15 + 1;
            return 15 * groups < PM_TAB && 15 * groups < PYR_SH && staged + 1 <= PYR_SH;
        };
        if (!rows_ok(L1, L0, ay0, nrow, sy_lo, by1 - sy_lo + 1) || !rows_ok(L2, L1, ty0, th, ay0, nrow)) return false;
    }
    for (int tx0 = 0; tx0 < L2.w; tx0 += PYR_TW) {
        const int tw = std::min(PYR_TW, L2.w - tx0);
        const int ax0 = std::max(0, fl((tx0 + 0.5) * L2.ssx - 0.5) - 2);
        const int c1 = std::min(L1.w - 1, fl((tx0 + tw - 0.5) * L2.ssx - 0.5) + 2);
        const int c0 = ax0 & ~15;
        const int ncol = c1 - c0 + 1;
        const int bx0 = std::max(0, fl((c0 + 0.5) * L1.ssx - 0.5) - 2);
        const int bx1 = std::min(L0.w - 1, fl((c1 + 0.5) * L1.ssx - 0.5) + 2);
        const int xa = bx0 & ~15, nc = ((bx1 - xa) >> 4) + 1;
        if (ncol > 16 * PM_MAXB1 || 16 * nc > PYR_SW) return false;
        max_nb1 = std::max(max_nb1, (ncol + 15) / 16);
        max_nc = std::max(max_nc, nc);
        for (int b = 0; b < (ncol + 15) / 16; b++) {
            const int kbrel = mkb[L1.mt_off + (c0 >> 4) + b] - xa;
            if (kbrel < 0 || kbrel + 32 > PYR_SW) return false;
        }
        for (int b = 0; 16 * b < tw; b++) {   // (c0 is a multiple of 16: kb - c0 stays 8-byte aligned)
            const int kbrel = mkb[L2.mt_off + (tx0 >> 4) + b] - c0;
            if (kbrel < 0 || kbrel + 32 > PYR_SW) return false;
        }
    }
    return max_rows * max_nc <= PYR_PF * 256 && max_nb1 * max_g1 <= 4 * PM_MAXU1;
}

}  // namespace orbamd
