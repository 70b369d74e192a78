// orbx_fast.h — stage 2 of orbx.hip: DetectFAST (:489-540, cv::FAST [ext]).  fast_cells_kernel: one
// wavefront per (frame, column strip of cells): crop -> LDS, FAST-9/16 corner score, cell-local 3x3 NMS at
// iniThFAST, retry at minThFAST when the cell is empty.  fast_hint_kernel: the next batch's first-cell
// speculation hints.
#pragma once
#include "orbx_geom.h"
#include "orbx_pyramid.h"   // us2

namespace orbamd {

// Corner strength M = max over the 16 nine-pixel arcs and both polarities of min |I_p - I_c|.
// A pixel is a FAST-9 corner at threshold t iff M > t, and cornerScore<16> == M - 1 for every
// detected corner (threshold-independent), so one M map serves both the iniThFAST pass and the
// minThFAST retry of DetectFAST.
//
// Cost model (PMC, tools/pmc_ab.sh): the kernel is issue-bound -- time follows the total count of
// instructions a wave issues (VALU + SALU + branch + LDS, about 2 cycles each per SIMD) and the VALU
// pipe's occupancy (v_pk_*, v_perm, v_alignbyte, v_mbcnt, v_cmp take 4 cycles, v_add/v_and/v_or/
// v_bitop3 and the unpacked 16-bit forms 2: tools/probe/issue_probe3).  So the tests below use the
// fewest instructions (packed u16, 2 pixels per instruction), not the cheapest ones, and avoid
// per-pixel branches.
template <int IMM>
__device__ __forceinline__ uint32_t bt3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, IMM); }
constexpr int BT_OR3 = 0xFE;   // a | b | c (truth tables over (a, b, c) = (0xF0, 0xCC, 0xAA))

// Two-of-four pre-test on packed u16 lanes.  A dword w of pixels x..x+3 is used as two words of
// u16 lanes: the even pixels (x, x+2) unpacked, w & 0x00ff00ff, and the odd pixels (x+1, x+3) in
// place, i.e. in each lane's high byte with the even pixel as a low byte.  The odd lanes' thresholds
// carry the low byte that makes the comparison depend on the high byte only:
//   p*256 + q > (v + t)*256 + 255  <=>  p > v + t     (saturated at 0xffff when v + t > 255)
//   (v - t)*256 > p*256 + q        <=>  p < v - t     (saturated at 0 when v < t)
// and max / min of such words order by the high byte first, so the same network serves both halves.
// Pass condition for four circle points at 90-degree steps (p1, p3 opposite; p2, p4 opposite): two
// circle-adjacent ones both brighter than v + t or both darker than v - t, which factors to
// (B1 | B3) & (B2 | B4):  min(max(p1, p3), max(p2, p4)) > hi  or  max(min(p1, p3), min(p2, p4)) < lo.
struct PkThr {
    us2 hi_e, lo_e, hi_o, lo_o;
};
__device__ __forceinline__ us2 u2us(uint32_t a) { return __builtin_bit_cast(us2, a); }
__device__ __forceinline__ uint32_t us2u(us2 a) { return __builtin_bit_cast(uint32_t, a); }
__device__ __forceinline__ us2 pk_even(uint32_t w) { return u2us(w & 0x00ff00ffu); }
__device__ __forceinline__ PkThr pk_thresholds(uint32_t wv, int t) {
    const unsigned short tc = (unsigned short)min(max(t, 0), 255);   // cv::FAST clamps the threshold
    const us2 t1 = {tc, tc}, t8 = {(unsigned short)(tc << 8), (unsigned short)(tc << 8)};
    PkThr r;
    const us2 ve = pk_even(wv);
    r.hi_e = ve + t1;                                                        // <= 510: no wrap
    r.lo_e = __builtin_elementwise_sub_sat(ve, t1);
    r.hi_o = __builtin_elementwise_add_sat(u2us(wv | 0x00ff00ffu), t8);      // (v + t)*256 + 255, saturated
    r.lo_o = __builtin_elementwise_sub_sat(u2us(wv & 0xff00ff00u), t8);      // (v - t)*256, saturated
    return r;
}
// non-zero u16 lanes where the pixel passes
__device__ __forceinline__ us2 pk_two_of_four(us2 p1, us2 p3, us2 p2, us2 p4, us2 hi, us2 lo) {
    const us2 bmax = __builtin_elementwise_min(__builtin_elementwise_max(p1, p3), __builtin_elementwise_max(p2, p4));
    const us2 dmin = __builtin_elementwise_max(__builtin_elementwise_min(p1, p3), __builtin_elementwise_min(p2, p4));
    return __builtin_elementwise_sub_sat(bmax, hi) | __builtin_elementwise_sub_sat(lo, dmin);
}

// Corner strength M (cornerScore<16> + 1, or 0 when not a corner at any threshold) on packed u16
// pairs: lane pair k holds circle positions (k, k + 8), so every min / max of the arc network covers
// two arcs at once; position j >= 8 is the swapped pair j - 8.  The network runs on the raw pixels:
// max over arcs of min(p) - v is the bright strength, v - min over arcs of max(p) the dark one.
__device__ __forceinline__ us2 swap2(us2 a) { return __builtin_shufflevector(a, a, 1, 0); }
// The 16 circle bytes as packed pairs (the compiler packs them with v_perm; ds_read_u8_d16_hi cannot
// be used: with SRAM ECC enabled, as on MI355X, d16 loads zero the other half of the register
// instead of preserving it -- a round-4 attempt failed tests/test_extractor_gpu.py exactly so).
template <int CS>
__device__ __forceinline__ void circle_pairs(const uint8_t* c, int cs, us2 (&D)[8]) {
    const int s = CS != 0 ? CS : cs;
#pragma unroll
    for (int k = 0; k < 8; k++)
        D[k] = us2{(unsigned short)c[c_circle_dy_h[k] * s + c_circle_dx_h[k]],
                   (unsigned short)c[c_circle_dy_h[k + 8] * s + c_circle_dx_h[k + 8]]};
}
template <int CS>
__device__ __forceinline__ int corner_strength_pk(const uint8_t* c, int cs) {
    us2 D[8];
    circle_pairs<CS>(c, cs, D);
    us2 l[8], h[8], l2[8], h2[8];
#pragma unroll
    for (int k = 0; k < 8; k++) {   // arcs of 2
        const us2 n = k + 1 < 8 ? D[k + 1] : swap2(D[k - 7]);
        l[k] = __builtin_elementwise_min(D[k], n);
        h[k] = __builtin_elementwise_max(D[k], n);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {   // arcs of 4
        const us2 nl = k + 2 < 8 ? l[k + 2] : swap2(l[k - 6]);
        const us2 nh = k + 2 < 8 ? h[k + 2] : swap2(h[k - 6]);
        l2[k] = __builtin_elementwise_min(l[k], nl);
        h2[k] = __builtin_elementwise_max(h[k], nh);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {   // arcs of 8
        const us2 nl = k + 4 < 8 ? l2[k + 4] : swap2(l2[k - 4]);
        const us2 nh = k + 4 < 8 ? h2[k + 4] : swap2(h2[k - 4]);
        l[k] = __builtin_elementwise_min(l2[k], nl);
        h[k] = __builtin_elementwise_max(h2[k], nh);
    }
    // arcs of 9 = two overlapping arcs of 8, max / min over all 16, two windows at a time by the lattice
    // identities max(min(a, b), min(b, c)) = min(b, max(a, c)) and min(max(a, b), max(b, c)) =
    // max(b, min(a, c)): 22 packed ops instead of 32
    us2 A, B;
#pragma unroll
    for (int j = 0; j < 8; j += 2) {   // windows starting at j and j + 1 (and j + 8, j + 9)
        const us2 cl = j + 2 < 8 ? l[j + 2] : swap2(l[0]);
        const us2 ch = j + 2 < 8 ? h[j + 2] : swap2(h[0]);
        const us2 wl = __builtin_elementwise_min(l[j + 1], __builtin_elementwise_max(l[j], cl));
        const us2 wh = __builtin_elementwise_max(h[j + 1], __builtin_elementwise_min(h[j], ch));
        A = j == 0 ? wl : __builtin_elementwise_max(A, wl);
        B = j == 0 ? wh : __builtin_elementwise_min(B, wh);
    }
    const int v = c[0];
    const int bright = (int)max(A.x, A.y) - v;   // max over arcs of min(p - v)
    const int dark = v - (int)min(B.x, B.y);     // max over arcs of min(v - p)
    return max(0, max(bright, dark));
}

// One wavefront per (cell, frame).  LDS (sized per launch from the largest cell): the crop
// (zone + 3-px apron, stored one byte right so zone column 0 is dword aligned), a zone map of
// corner strengths, a queue of pre-test passers and the ordered list of corners.
//   1. crop -> LDS with aligned dword loads issued together
//   2. compass pre-test, 4 pixels per lane (SWAR), groups with a passer queued in row-major order
//   3. diagonal pre-test on the queued groups' passers (SWAR), survivors queued per pixel; those get
//      the corner strength densely, 64 at a time; corners are appended in row-major order
//   4. corner strength M (cornerScore + 1) for the corner list; NMS at iniThFAST and minThFAST
//      over the list (3x3, cell-local: neighbours outside the zone count as 0)
//   5. emit the iniThFAST set, or the minThFAST set when it is empty (DetectFAST :527-530)
constexpr int GR_RING = 128;   // pre-test group ring (u32 entries; power of two, >= 64 + 64)
constexpr int FQ2_RING = 512;  // diagonal-filter passer ring (u16 entries; power of two, >= 64 + 256)
constexpr int FAST_CLIST_CAP = 256;   // ordered corner list (cells with more take the zone-scan NMS)

struct FastLds {
    int CS, ZS, crop_bytes, mz_bytes, qcap, ccap;
};

#ifdef ORB_FAST_STAMPS
// diagnostic build: phase stamps of every 64th logical wave (8 words each)
#define FAST_NSAMP 8192
__device__ unsigned long long g_fast_stamps[FAST_NSAMP * 8];
#define FAST_STAMP(k, v)                                                                               \
    do {                                                                                             \
        if (lane == 0 && (lb & 63) == 0 && (lb >> 6) < FAST_NSAMP) g_fast_stamps[(lb >> 6) * 8 + (k)] = (v); \
    } while (0)
#else
#define FAST_STAMP(k, v) do {} while (0)
#endif

// Crop staging.  LDS dword mm of crop row r holds crop cols 4mm-1 .. 4mm+2 (col c at byte c+1), i.e.
// the 4 image bytes starting at q = (y0+r)*step + x0 - 1 + 4mm, built with v_alignbyte from the two
// dword-aligned image words around q.  The (row, dword) pairs are walked flat over the wave's 64
// lanes; the first CROP_PF*64 of them are loaded into registers one cell ahead (the loads of cell
// i+1 are in flight while cell i is processed), the rest (cells wider or taller than ~40 px) are
// loaded and stored synchronously.
constexpr int CROP_PF = 8;
typedef uint32_t u32x2a4 __attribute__((ext_vector_type(2), aligned(4)));

struct CropWalk {
    int row, mm, dr, dm, ndl;
    __device__ __forceinline__ CropWalk(int lane, int ndl_) : ndl(ndl_) {
        row = lane / ndl;
        mm = lane - row * ndl;
        dr = 64 / ndl;
        dm = 64 - dr * ndl;
    }
    __device__ __forceinline__ void next() {
        row += dr;
        mm += dm;
        if (mm >= ndl) { mm -= ndl; row++; }
    }
};

struct CropSrc {
    const uint8_t* img;   // level base of the frame (wave-uniform)
    int step, x0, y0, ch, ndl, h;   // h: the level's height
    __device__ __forceinline__ int q(const CropWalk& w) const { return (y0 + w.row) * step + x0 - 1 + 4 * w.mm; }
    __device__ __forceinline__ int mis(int q) const {
        return (int)(((uint32_t)reinterpret_cast<uintptr_t>(img) + (uint32_t)q) & 3u);
    }
    __device__ __forceinline__ u32x2a4 load(int q) const {
        return *reinterpret_cast<const u32x2a4*>(img + (q - mis(q)));
    }
};

__device__ __forceinline__ void crop_prefetch(const CropSrc& c, int lane, u32x2a4 (&v)[CROP_PF]) {
    CropWalk w(lane, c.ndl);
#pragma unroll
    for (int it = 0; it < CROP_PF; it++) {   // unconditional (row clamped): straight-line loads
        CropWalk wc = w;
        wc.row = min(w.row, c.ch - 1);
        v[it] = c.load(c.q(wc));
        w.next();
    }
}

__device__ __forceinline__ void crop_commit(const CropSrc& c, int lane, const u32x2a4 (&v)[CROP_PF], uint8_t* crop,
                                            int CSd) {
    CropWalk w(lane, c.ndl);
#pragma unroll
    for (int it = 0; it < CROP_PF; it++) {
        if (w.row < c.ch) {
            const int q = c.q(w);
            reinterpret_cast<uint32_t*>(crop + w.row * CSd)[w.mm] = __builtin_amdgcn_alignbyte(v[it].y, v[it].x, c.mis(q));
        }
        w.next();
    }
    while (w.row < c.ch) {   // rare: crops larger than CROP_PF*64 dwords
        const int q = c.q(w);
        const u32x2a4 t = c.load(q);
        reinterpret_cast<uint32_t*>(crop + w.row * CSd)[w.mm] = __builtin_amdgcn_alignbyte(t.y, t.x, c.mis(q));
        w.next();
    }
}

// Row-group staging: lanes per crop row LR = 16 (32, 64 for wider crops), row group k covers
// rows RPG*k .. RPG*k + RPG-1.  A group's source address is wave-uniform plus a per-lane constant,
// so a load costs no address VALU; only the realignment (v_alignbyte) and the LDS address remain.
constexpr int CROP_NG = 10;
constexpr int FAST_CROP_SLACK = 3;   // crop rows past the tallest crop: a partial last row group (RPG <= 4)
// groups whose loads are issued together (40 rows at LR = 16)
// LRS = log2(lanes per crop row), a template constant so that with a compile-time crop stride the
// CROP_NG row-group stores share one LDS base address (offset fields) instead of CROP_NG live
// per-lane addresses.
template <int LRS>   // 0: from the crop's row-dword count at run time
__device__ __forceinline__ void crop_stage_rows_t(const CropSrc& c, int lane, uint8_t* crop, int CSd) {
    const int lrs = LRS ? LRS : (c.ndl <= 16 ? 4 : (c.ndl <= 32 ? 5 : 6));   // 0: run time
    const int RPG = 64 >> lrs;
    const int roff = lane >> lrs, d = lane & ((1 << lrs) - 1);
    const bool dok = d < c.ndl;
    const int dd = dok ? d : 0;
    const uint8_t* g0 = c.img + (long long)c.y0 * c.step + (c.x0 - 1);   // wave-uniform
    const int ng = (c.ch + RPG - 1) >> (6 - lrs);
    if ((c.step & 3) == 0) {
        // dword-multiple row step (every pyramid level; level 0 unless the caller's step is odd):
        // the misalignment is one wave-uniform shift, the loads are buffer loads off a scalar
        // resource with a per-lane constant voffset and a per-group soffset (no address VALU),
        // and a partial last group writes into the crop's slack rows (FAST_CROP_SLACK).  The resource
        // ends with the level, so loads of groups past it return 0 instead of needing a clamp, and the
        // first batch stores all CROP_NG groups unconditionally (the crop buffer holds CROP_NG * 4 rows,
        // and groups past the crop only fill rows nothing reads): no per-group scalar control.
        const int m = __builtin_amdgcn_readfirstlane((int)(reinterpret_cast<uintptr_t>(g0) & 3u));
        const int avail = (c.h - c.y0) * c.step - (c.x0 - 1) + m;   // bytes from g0 - m to the level's end
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(g0 - m), 0, avail, 0x00020000);
        const int voff = roff * c.step + 4 * dd;
        uint32_t* lrow = reinterpret_cast<uint32_t*>(crop + roff * CSd) + d;
        const int gstep = RPG * c.step, lstep = RPG * CSd / 4;
        {
            u32x2a4 v[CROP_NG];
#pragma unroll
            for (int k = 0; k < CROP_NG; k++) {
                const auto t = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, k * gstep, 0);
                v[k] = u32x2a4{t[0], t[1]};
            }
            if (dok) {
#pragma unroll
                for (int k = 0; k < CROP_NG; k++) lrow[k * lstep] = __builtin_amdgcn_alignbyte(v[k].y, v[k].x, m);
            }
        }
        for (int k0 = CROP_NG; k0 < ng; k0 += CROP_NG) {   // crops taller than CROP_NG groups (rare)
            u32x2a4 v[CROP_NG];
#pragma unroll
            for (int k = 0; k < CROP_NG; k++) {
                const auto t = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, (k0 + k) * gstep, 0);
                v[k] = u32x2a4{t[0], t[1]};
            }
            if (dok) {
#pragma unroll
                for (int k = 0; k < CROP_NG; k++)
                    if (k0 + k < ng) lrow[(k0 + k) * lstep] = __builtin_amdgcn_alignbyte(v[k].y, v[k].x, m);
            }
        }
        return;
    }
    const int loff = roff * c.step + 4 * dd;                            // per-lane constant
    for (int k0 = 0; k0 < ng; k0 += CROP_NG) {
        u32x2a4 v[CROP_NG];
        int m[CROP_NG];
#pragma unroll
        for (int k = 0; k < CROP_NG; k++) {
            // group k's rows; a partial last group reads up to RPG-1 rows past the crop, which stay
            // inside the level (crops end >= 13 rows above its bottom edge); groups past the crop
            // re-read the last group
            const int gk = min(k0 + k, ng - 1);
            const uint8_t* p = g0 + (long long)(RPG * gk) * c.step + loff;
            m[k] = (int)(reinterpret_cast<uintptr_t>(p) & 3u);
            v[k] = *reinterpret_cast<const u32x2a4*>(p - m[k]);
        }
#pragma unroll
        for (int k = 0; k < CROP_NG; k++) {
            const int r = RPG * (k0 + k) + roff;
            if (dok && r < c.ch)
                reinterpret_cast<uint32_t*>(crop + r * CSd)[d] = __builtin_amdgcn_alignbyte(v[k].y, v[k].x, m[k]);
        }
    }
}

template <int CST>
__device__ __forceinline__ void crop_stage_rows(const CropSrc& c, int lane, uint8_t* crop, int CSd) {
    if (CST == 0) crop_stage_rows_t<0>(c, lane, crop, CSd);   // run-time stride: one generic copy
    else if (c.ndl <= 16) crop_stage_rows_t<4>(c, lane, crop, CSd);
    else if (c.ndl <= 32) crop_stage_rows_t<5>(c, lane, crop, CSd);
    else crop_stage_rows_t<6>(c, lane, crop, CSd);
}

// One wavefront processes `cpw` consecutive (frame, cell) items of the XCD-swizzled order; item
// i = f * ncells + cell.  LDS (sized per launch from the largest cell): the crop (zone + 3-px
// apron), a zone map of corner strengths, a queue of pre-test passers and the ordered corner list.
#ifndef FAST_WAVES_DEF
#define FAST_WAVES_DEF 6
#endif
// CST / ZST: the crop and zone-map row strides when known at compile time (the C1-C3 geometries:
// 48 / 36 and 52 / 40), so every LDS address off a row base folds into the instruction's offset
// field; 0 = read them from FastLds (any other geometry).
// PAIR (round 6, ORBX_FAST_PAIR=1): two vertically consecutive cells of the strip per pass, as one
// merged zone (one crop of zhA + zhB + 6 rows, one zone map with a zero separator row between the
// cells so the 3x3 NMS stays cell-local, one set of rings): the end-of-cell partial drains, partial
// strength batches, NMS chunks and emission loops happen once per pair instead of once per cell.
// Counts, the iniThFAST / minThFAST choice (:527-530), the slot capacity and the output stay per cell;
// a speculative pass is kept only when both cells keep an iniThFAST corner.
template <int CST, int ZST, bool PAIR>
__global__ __launch_bounds__(64, FAST_WAVES_DEF) void fast_cells_kernel(Geom g, const CellDev* __restrict__ cells,
                                                        const int2* __restrict__ strips,
                                                        const uint8_t* __restrict__ in, long long in_fstride,
                                                        int in_step, const uint8_t* __restrict__ pyr, int th_ini,
                                                        int th_min, uint32_t* __restrict__ slots,
                                                        int* __restrict__ cell_cnt, uint32_t* fault, FastLds fl,
                                                        int strip_beg, int nstrips, int spec_arg) {
    extern __shared__ __attribute__((aligned(16))) uint8_t fsm[];
    uint8_t* crop = fsm;                                   // crop col c at byte 1 + c
    uint8_t* Mz = fsm + fl.crop_bytes;
    short* queue = reinterpret_cast<short*>(Mz + fl.mz_bytes);
    short* clist = queue + fl.qcap;
    unsigned long long* bal = reinterpret_cast<unsigned long long*>(clist + fl.ccap);
    const int CSd = CST ? CST : fl.CS, ZSd = ZST ? ZST : fl.ZS;

    const int lane = threadIdx.x;
    const int lb = xcd_swizzle(blockIdx.x, gridDim.x);
    FAST_STAMP(0, __builtin_amdgcn_s_memtime());
    // wavefront = (frame, column strip): up to fast_cpw vertically consecutive cells of one column
    const int f = lb / nstrips;
    const int2 sd = strips[strip_beg + lb - f * nstrips];
    const int i_beg = 0, i_end = sd.y & 255, cstride = (sd.y >> 8) & 0x7fffff;   // bit 31: the first-cell hint
    // every cell of a strip has the same level and zone width (host-checked): the crop's level
    // base, step and row-dword count and every per-lane quantity that depends on the zone width are
    // loop-invariant over the strip
    const CellDev c0 = cells[sd.x];
    const int zw = c0.zwzh & 0xffff;
    int lstep;
    const uint8_t* limg = level_base(g, c0.level, f, in, in_fstride, in_step, pyr, &lstep);
    const int lh = g.lv[c0.level].h;
    const int ndl = (zw + 6 + 1 + 3) >> 2;   // LDS dwords per crop row
    auto source = [&](int item, CellDev& cd, int& ci) {
        ci = sd.x + item * cstride;
        cd = cells[ci];
        CropSrc c;
        c.img = limg;
        c.step = lstep;
        c.x0 = cd.x0y0 & 0xffff;
        c.y0 = cd.x0y0 >> 16;
        c.ch = (cd.zwzh >> 16) + 6;
        c.ndl = ndl;
        c.h = lh;
        return c;
    };
    // Speculative iniThFAST pass: a cell whose predecessor in this wavefront (the cell above it in
    // the same column) kept >= spec_min corners at iniThFAST is first run with the pre-test,
    // the diagonal filter and the corner list at iniThFAST only.  When the NMS keeps one of them
    // that is DetectFAST's answer (:527); otherwise the cell is re-run at min(ini, min).  On
    // texture-rich frames most pixels pass at minThFAST but few at iniThFAST.
    // spec_arg: the threshold (-1: every cell), bit 29 (threshold > 0 only): a strip's first cell, which has
    // no predecessor, speculates when the strip's hint bit (bit 31 of its descriptor, set by
    // fast_hint_kernel from the CELL_CNT_INI bit its cell got in frame 0 of the previous launch) is set.
    // Consecutive batches of a sequence see the same texture there.  The hint costs the cell loop
    // nothing (the descriptor is already in SGPRs; the kernel is at its SGPR limit), and it only decides
    // whether to speculate, never the result.
    const int spec_min = spec_arg < 0 ? spec_arg : spec_arg & 0x1fffffff;
    int prev_ini = (spec_arg > 0 && ((spec_arg >> 29) & 1) && sd.y < 0) ? spec_min : 0;
    for (int item = i_beg; item < i_end; item += PAIR ? 2 : 1) {
    CellDev cell;
    int ci;
    CropSrc src = source(item, cell, ci);
    const int x0 = src.x0, y0 = src.y0;
    const int zhA = cell.zwzh >> 16;
    // PAIR: the second cell (the one below; zhB = 0 when the strip has an odd count) extends the zone
    const bool hasB = PAIR && item + 1 < i_end;
    CellDev cellB = cell;
    int ciB = ci, zhB = 0;
    if (hasB) {
        ciB = ci + cstride;
        cellB = cells[ciB];
        zhB = cellB.zwzh >> 16;
        src.ch += zhB;
    }
    const int zh = zhA + zhB;
    // zone-map row of zone row y: PAIR inserts a zero row between the cells
    auto mrow = [&](int y) { return PAIR ? y + (y >= zhA ? 1 : 0) : y; };
    {
        crop_stage_rows<CST>(src, lane, crop, CSd);
    }
    const int tlo = min(th_ini, th_min);
    bool spec = spec_min != 0 && th_ini > tlo && prev_ini >= spec_min;   // spec_min < 0: every cell
    uint8_t* Mc = Mz + ZSd + 1;   // zone (0, 0); the zero border makes out-of-zone neighbours read 0
    uint32_t* out = slots + (long long)f * g.slot_frame + cell.slot;
    const int cap = ((zw + 1) / 2) * ((zhA + 1) / 2);
    int n_ini = 0, n_min = 0, total = 0;
    int n_iniB = 0, totalB = 0;   // PAIR: the second cell
    for (;;) {   // passes: speculative (iniThFAST) and / or full (min(ini, min))
    for (int i = lane; i < ((zh + 2 + (PAIR ? 1 : 0)) * ZSd + 15) >> 4; i += 64) reinterpret_cast<uint4*>(Mz)[i] = make_uint4(0, 0, 0, 0);
    wave_lds_sync();
    if (item == i_beg) FAST_STAMP(1, __builtin_amdgcn_s_memtime());

    const int tp = spec ? th_ini : tlo;   // threshold of this pass
    // lanes: QR quads per row (8 or 16), 64/QR rows per chunk
    const int qsh = zw <= 32 ? 3 : 4;
    const int QR = 1 << qsh, RPC = 64 >> qsh;
    const int qx = (lane & (QR - 1)) * 4, qy = lane >> qsh;
    // u16-lane masks (1 / 0) of the zone's columns: even lanes hold (qx, qx+2), odd lanes (qx+1, qx+3)
    const us2 pme = {(unsigned short)(qx < zw), (unsigned short)(qx + 2 < zw)};
    const us2 pmo = {(unsigned short)(qx + 1 < zw), (unsigned short)(qx + 3 < zw)};

    // Stage 1 (dense): the compass pre-test (points 0/4/8/12) on 4 pixels per lane; a lane whose group
    // of 4 has a passer appends one entry (pass bits 0, 1, 16, 17 = pixels qx .. qx+3, the group's
    // zone index (y << 8) | qx at bits 2-15) to a ring of GR_RING groups in row-major order.
    // Stage 2, whenever 64 groups are pending: the diagonal pre-test (points 2/6/10/14: a 9-arc also
    // holds two circle-adjacent ones of them) on the passers of 64 groups, survivors appended per pixel
    // to a second ring in row-major order (14 % -> 5 % of the pixels on the synthetic frames).
    // Stage 3, whenever 64 pixels are pending: the corner strength M densely.  Corners (M > the pass
    // threshold) get M in the zone map and are appended to the ordered corner list.
    // (pending groups < 64 + 64 <= GR_RING; pending pixels < 64 + 256 <= FQ2_RING.)
    uint32_t* gring = reinterpret_cast<uint32_t*>(queue);
    short* queue2 = queue + 2 * GR_RING;
    int qn = 0, head = 0, q2n = 0, h2 = 0, nc = 0;
    auto strength = [&](int n) {
        const int i = lane < n ? queue2[(h2 + lane) & (FQ2_RING - 1)] : -1;
        int M = 0;
        if (i >= 0) M = corner_strength_pk<CST>(&crop[__mul24((i >> 8) + 3, CSd) + 4 + (i & 255)], CSd);
        const bool c = M > tp;
        const unsigned long long bm = __ballot(c);
        if (c) {
            const int pos = nc + rank64(bm);
            if (pos < fl.ccap) clist[pos] = (short)i;   // past ccap: the cell takes the zone-scan NMS below
            Mc[__mul24(mrow(i >> 8), ZSd) + (i & 255)] = (uint8_t)min(M, 255);
        }
        nc += popc64(bm);
        h2 += n;
    };
    auto drain = [&](int n) {
        const uint32_t e = lane < n ? gring[(head + lane) & (GR_RING - 1)] : 0u;   // 0: no pass bits
        // zone index (y << 8) | x; PAIR: stored as (y << 6) | x at bits 18-30 (merged zones are taller
        // than the 64 rows bits 2-15 hold)
        const int i0 = PAIR ? (int)(((e >> 24) << 8) | ((e >> 18) & 63u)) : (int)((e >> 2) & 0x3fffu);
        const uint8_t* c = crop + __mul24((i0 >> 8) + 3, CSd) + 4 + (i0 & 255);   // zone (y, x): dword aligned
        const uint32_t* cp = reinterpret_cast<const uint32_t*>(c + 2 * CSd);
        const uint32_t* cm = reinterpret_cast<const uint32_t*>(c - 2 * CSd);
        const uint32_t wv = *reinterpret_cast<const uint32_t*>(c);
        const uint32_t ap = cp[-1], bp = cp[0], dp = cp[1], am = cm[-1], bm_ = cm[0], dm = cm[1];
        const uint32_t Lp = __builtin_amdgcn_alignbyte(bp, ap, 2), Rp = __builtin_amdgcn_alignbyte(dp, bp, 2);
        const uint32_t Lm = __builtin_amdgcn_alignbyte(bm_, am, 2), Rm = __builtin_amdgcn_alignbyte(dm, bm_, 2);
        // position 2 = (+2, +2): Rp, 10 = (-2, -2): Lm, 6 = (+2, -2): Rm, 14 = (-2, +2): Lp
        const PkThr T = pk_thresholds(wv, tp);
        const us2 se = __builtin_elementwise_min(
            pk_two_of_four(pk_even(Rp), pk_even(Lm), pk_even(Rm), pk_even(Lp), T.hi_e, T.lo_e), u2us(e & 0x00010001u));
        const us2 so = __builtin_elementwise_min(pk_two_of_four(u2us(Rp), u2us(Lm), u2us(Rm), u2us(Lp), T.hi_o, T.lo_o),
                                                 u2us((e >> 1) & 0x00010001u));
        // ordered compaction of up to 4 survivors per lane: one ballot per pixel slot, the lane's
        // position = the survivors of the lower lanes (mbcnt) + its own earlier slots
        const bool p0 = se.x != 0, p1 = so.x != 0, p2 = se.y != 0, p3 = so.y != 0;
        const unsigned long long b0 = __ballot(p0), b1 = __ballot(p1), b2 = __ballot(p2), b3 = __ballot(p3);
        unsigned pre = __builtin_amdgcn_mbcnt_hi((unsigned)(b0 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b0, 0u));
        pre = __builtin_amdgcn_mbcnt_hi((unsigned)(b1 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b1, pre));
        pre = __builtin_amdgcn_mbcnt_hi((unsigned)(b2 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b2, pre));
        pre = __builtin_amdgcn_mbcnt_hi((unsigned)(b3 >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b3, pre));
        int pos = q2n + (int)pre;
        if (p0) queue2[pos++ & (FQ2_RING - 1)] = (short)i0;
        if (p1) queue2[pos++ & (FQ2_RING - 1)] = (short)(i0 + 1);
        if (p2) queue2[pos++ & (FQ2_RING - 1)] = (short)(i0 + 2);
        if (p3) queue2[pos & (FQ2_RING - 1)] = (short)(i0 + 3);
        q2n += popc64(b0) + popc64(b1) + popc64(b2) + popc64(b3);
        head += n;
        wave_lds_sync();
        while (q2n - h2 >= 64) strength(64);
    };
    // per-lane LDS address of zone (qy, qx) = crop (qy+3, qx+3) at byte qx+4 and the group's zone index
    // (qy << 8) | qx at bits 2-15, both stepped by a wave-uniform amount per chunk of RPC rows
    const uint8_t* rowq = crop + __mul24(qy + 3, CSd) + 4 + qx;
    const uint32_t e0s = PAIR ? (uint32_t)((qy << 6) | qx) << 18 : (uint32_t)((qy << 8) | qx) << 2;
    const bool qxin = qx < zw;
    for (int yb = 0, yoff = 0; yb < zh; yb += RPC, yoff += RPC * CSd) {
        const int y = yb + qy;
        us2 pe = {0, 0}, po = {0, 0};
        if (y < zh && qxin) {
            const uint8_t* rowc = rowq + yoff;   // zone (y, qx)
            const uint32_t wv = *reinterpret_cast<const uint32_t*>(rowc);
            const uint32_t wl = *reinterpret_cast<const uint32_t*>(rowc - 4);
            const uint32_t wr = *reinterpret_cast<const uint32_t*>(rowc + 4);
            const uint32_t wn = *reinterpret_cast<const uint32_t*>(rowc + 3 * CSd);   // (0,+3)
            const uint32_t ws = *reinterpret_cast<const uint32_t*>(rowc - 3 * CSd);   // (0,-3)
            const uint32_t we = __builtin_amdgcn_alignbyte(wr, wv, 3);   // (+3, 0): bytes qx+3..qx+6
            const uint32_t ww = __builtin_amdgcn_alignbyte(wv, wl, 1);   // (-3, 0): bytes qx-3..qx
            const PkThr T = pk_thresholds(wv, tp);
            pe = __builtin_elementwise_min(
                pk_two_of_four(pk_even(wn), pk_even(ws), pk_even(we), pk_even(ww), T.hi_e, T.lo_e), pme);
            po = __builtin_elementwise_min(pk_two_of_four(u2us(wn), u2us(ws), u2us(we), u2us(ww), T.hi_o, T.lo_o), pmo);
        }
        const bool any = (us2u(pe) | us2u(po)) != 0;
        const unsigned long long bm = __ballot(any);
        if (any) {
            // ring slot = qn + the passers of the lower lanes (mbcnt accumulates qn)
            const unsigned pos = __builtin_amdgcn_mbcnt_hi((unsigned)(bm >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bm, (unsigned)qn));
            gring[pos & (GR_RING - 1)] = bt3<BT_OR3>(us2u(pe), us2u(po) + us2u(po), e0s + ((uint32_t)yb << (PAIR ? 24 : 10)));
        }
        qn += popc64(bm);
        wave_lds_sync();
        if (qn - head >= 64) drain(64);
    }
    if (qn > head) drain(qn - head);
    if (q2n > h2) strength(q2n - h2);
    wave_lds_sync();
    if (item == i_beg) FAST_STAMP(3, __builtin_amdgcn_s_memtime());

    n_ini = 0;
    n_min = 0;
    n_iniB = 0;   // (a speculative pass that fell through left its counts)
    if constexpr (PAIR) {
        // Both cells' NMS in one walk (the list, or the zone map row by row for dense pairs), with a
        // third ballot per chunk marking the first cell's entries (row-major: a prefix), then each
        // cell's emission from its own threshold's ballots.  Ballots: 3 words per chunk / pass.
        const bool dense = nc > fl.ccap;
        const int rsh = zw <= 32 ? 5 : 6, RP = 64 >> rsh;
        const int zx = lane & ((1 << rsh) - 1), zr = lane >> rsh;
        unsigned long long* pb = dense ? reinterpret_cast<unsigned long long*>(queue) : bal;
        int nm_b = 0, nch = 0;
        const int nsteps = dense ? (zh + RP - 1) / RP : (nc + 63) >> 6;
        for (; nch < nsteps; nch++) {
            bool ki = false, km = false, inA = false;
            int y = -1, x = 0;
            if (dense) {
                if (zx < zw && zr + nch * RP < zh) { y = zr + nch * RP; x = zx; }
            } else if (nch * 64 + lane < nc) {
                const int i = clist[nch * 64 + lane];
                y = i >> 8;
                x = i & 255;
            }
            if (y >= 0) {
                inA = y < zhA;
                const uint8_t* c0 = Mc + __mul24(mrow(y), ZSd) + x;
                const int m = c0[0];
                if (m) {
                    const int n0 = max(max((int)c0[-ZSd - 1], (int)c0[-ZSd]), (int)c0[-ZSd + 1]);
                    const int n1 = max((int)c0[-1], (int)c0[1]);
                    const int n2 = max(max((int)c0[ZSd - 1], (int)c0[ZSd]), (int)c0[ZSd + 1]);
                    const bool top = max(max(n0, n1), n2) < m;
                    ki = top && m > th_ini;
                    km = top && m > th_min;
                }
            }
            const unsigned long long bi = __ballot(ki), bmn = __ballot(km), ba = __ballot(inA);
            if (lane == 0) { pb[3 * nch] = bi; pb[3 * nch + 1] = bmn; pb[3 * nch + 2] = ba; }
            n_ini += popc64(bi & ba);
            n_min += popc64(bmn & ba);
            n_iniB += popc64(bi & ~ba);
            nm_b += popc64(bmn & ~ba);
        }
        wave_lds_sync();
        if (spec && (n_ini == 0 || (hasB && n_iniB == 0))) goto full_pass;
        const int wA = n_ini > 0 ? 0 : 1, wB = n_iniB > 0 ? 0 : 1;
        total = wA == 0 ? n_ini : n_min;
        totalB = wB == 0 ? n_iniB : nm_b;
        uint32_t* outB = slots + (long long)f * g.slot_frame + cellB.slot;
        const int capB = ((zw + 1) / 2) * ((zhB + 1) / 2);
        const unsigned long long below = lanemask_lt();
        int runA = 0, runB = 0;
        for (int p = 0; p < nch; p++) {
            const unsigned long long ba = pb[3 * p + 2];
            const unsigned long long kA = pb[3 * p + wA] & ba, kB = pb[3 * p + wB] & ~ba;
            if (((kA | kB) >> lane) & 1) {
                const bool a = (kA >> lane) & 1;
                const int r = a ? runA + popc64(kA & below) : runB + popc64(kB & below);
                int y, x;
                if (dense) { y = zr + p * RP; x = zx; }
                else { const int i = clist[p * 64 + lane]; y = i >> 8; x = i & 255; }
                if (r < (a ? cap : capB))
                    (a ? out : outB)[r] = (uint32_t)(x0 + 3 + x) | ((uint32_t)(y0 + 3 + y) << 12) |
                                          ((uint32_t)(Mc[__mul24(mrow(y), ZSd) + x] - 1) << 24);
            }
            runA += popc64(kA);
            runB += popc64(kB);
        }
    } else if (nc > fl.ccap) {
        // Dense cell (more corners than the list holds, e.g. pure noise): NMS over the zone map in
        // row-major order, one zone row per pass (zw <= 64), the same keep rule: a corner is kept
        // at threshold t iff M > t and every neighbour is < M (for M > t, a neighbour q >= M is
        // also > t), so both thresholds share the neighbourhood maximum.  (The speculative pass's
        // map holds only the corners at iniThFAST: a neighbour with M <= ini < m never suppresses
        // at iniThFAST, so its iniThFAST set is the full pass's.)
        // Rows per pass: two 32-lane rows when the zone is at most 32 wide (every C1-C3 cell but the
        // widest cells of the smallest levels), else one 64-lane row.  The keep ballots of both
        // thresholds are computed once and kept in the (drained) passer ring for the emission pass;
        // lane order within a pass is row-major, so the emission order is the reference's.
        const int rsh = zw <= 32 ? 5 : 6, RP = 64 >> rsh;
        const int zx = lane & ((1 << rsh) - 1), zr = lane >> rsh;
        unsigned long long* dbal = reinterpret_cast<unsigned long long*>(queue);   // 2 per pass, <= 160
        int npass = 0;
        for (int yb = 0; yb < zh; yb += RP, npass++) {
            const int y = yb + zr;
            bool ki = false, km = false;
            if (zx < zw && y < zh) {
                const uint8_t* c0 = Mc + __mul24(y, ZSd) + zx;
                const int m = c0[0];
                if (m) {
                    const int n0 = max(max((int)c0[-ZSd - 1], (int)c0[-ZSd]), (int)c0[-ZSd + 1]);
                    const int n1 = max((int)c0[-1], (int)c0[1]);
                    const int n2 = max(max((int)c0[ZSd - 1], (int)c0[ZSd]), (int)c0[ZSd + 1]);
                    const int nmax = max(max(n0, n1), n2);
                    ki = m > th_ini && nmax < m;
                    km = m > th_min && nmax < m;
                }
            }
            const unsigned long long bi = __ballot(ki), bmn = __ballot(km);
            if (lane == 0) { dbal[2 * npass] = bi; dbal[2 * npass + 1] = bmn; }
            n_ini += popc64(bi);
            n_min += popc64(bmn);
        }
        wave_lds_sync();
        if (spec && n_ini == 0) goto full_pass;
        const int which = n_ini > 0 ? 0 : 1;
        total = which == 0 ? n_ini : n_min;
        int running = 0;
        for (int pp = 0; pp < npass; pp++) {
            const unsigned long long bm = dbal[2 * pp + which];
            if (bm & (1ull << lane)) {
                const int r = running + rank64(bm);
                const int y = pp * RP + zr;
                if (r < cap)
                    out[r] = (uint32_t)(x0 + 3 + zx) | ((uint32_t)(y0 + 3 + y) << 12) |
                             ((uint32_t)(Mc[__mul24(y, ZSd) + zx] - 1) << 24);
            }
            running += popc64(bm);
        }
    } else {
    for (int jb = 0, ch2 = 0; jb < nc; jb += 64, ch2++) {
        const int j = jb + lane;
        bool ki = false, km = false;
        if (j < nc) {   // 3x3 NMS at both thresholds from one read of the 8 neighbours: for M > t a
                        // neighbour q >= M is also > t, so both keep rules are M > t && max(q) < M
            const int i = clist[j];
            const uint8_t* c0 = Mc + __mul24(i >> 8, ZSd) + (i & 255);
            const int m = c0[0];
            const int n0 = max(max((int)c0[-ZSd - 1], (int)c0[-ZSd]), (int)c0[-ZSd + 1]);
            const int n1 = max((int)c0[-1], (int)c0[1]);
            const int n2 = max(max((int)c0[ZSd - 1], (int)c0[ZSd]), (int)c0[ZSd + 1]);
            const bool top = max(max(n0, n1), n2) < m;
            ki = top && m > th_ini;
            km = top && m > th_min;
        }
        const unsigned long long bi = __ballot(ki), bmn = __ballot(km);
        if (lane == 0) { bal[2 * ch2] = bi; bal[2 * ch2 + 1] = bmn; }
        n_ini += popc64(bi);
        n_min += popc64(bmn);
    }
    wave_lds_sync();
    if (spec && n_ini == 0) goto full_pass;

    const int which = n_ini > 0 ? 0 : 1;
    total = which == 0 ? n_ini : n_min;
    int running = 0;
    for (int jb = 0, ch2 = 0; jb < nc; jb += 64, ch2++) {
        const unsigned long long bm = bal[2 * ch2 + which];
        if (bm & (1ull << lane)) {
            const int r = running + rank64(bm);
            const int i = clist[jb + lane];
            if (r < cap) {
                const int zy = i >> 8, zx = i & 255;
                const uint32_t x = (uint32_t)(x0 + 3 + zx), yy = (uint32_t)(y0 + 3 + zy);
                out[r] = x | (yy << 12) | ((uint32_t)(Mc[__mul24(zy, ZSd) + zx] - 1) << 24);
            }
        }
        running += popc64(bm);
    }
    }   // list NMS
    break;
full_pass:   // the speculative pass kept no corner at iniThFAST: the full pass decides
    spec = false;
    }   // passes
    prev_ini = hasB ? n_iniB : n_ini;
    if (item == i_beg) FAST_STAMP(4, __builtin_amdgcn_s_memtime());
    if (lane == 0) {
        if (total > cap) atomicOr(fault, FAULT_CELL_CAP);
        // bit 30: this cell kept >= spec_min corners at iniThFAST (the next strips' first-cell hint;
        // the quadtree masks the count with CELL_CNT_MASK)
        cell_cnt[(long long)f * g.ncells_total + ci] = min(total, cap) | (n_ini >= spec_min ? CELL_CNT_INI : 0);
        if (hasB) {
            const int capB = ((zw + 1) / 2) * ((zhB + 1) / 2);
            if (totalB > capB) atomicOr(fault, FAULT_CELL_CAP);
            cell_cnt[(long long)f * g.ncells_total + ciB] = min(totalB, capB) | (n_iniB >= spec_min ? CELL_CNT_INI : 0);
        }
    }
    if (item == i_beg) {
        FAST_STAMP(2, __builtin_amdgcn_s_memtime());
        FAST_STAMP(6, ((unsigned long long)cell.level << 48) | ((unsigned long long)n_min << 16) | (unsigned)total);
    }
    wave_lds_sync();
    }   // items
    FAST_STAMP(5, __builtin_amdgcn_s_memtime());
    FAST_STAMP(7, (unsigned long long)(i_end - i_beg));
}

// FAST's first-cell hint for the next launch: bit 31 of every strip descriptor = the CELL_CNT_INI bit of
// its first cell in frame 0 (cell_cnt's frame-0 slots).  One thread per strip, once per batch after every
// stage of it (launch_fast_hint).
__global__ void fast_hint_kernel(int2* __restrict__ strips, const int* __restrict__ cell_cnt, int nstrips) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nstrips) return;
    const int2 sd = strips[s];
    const unsigned bit = (cell_cnt[sd.x] & CELL_CNT_INI) ? 0x80000000u : 0u;
    strips[s].y = (int)(((unsigned)sd.y & 0x7fffffffu) | bit);
}

}  // namespace orbamd
