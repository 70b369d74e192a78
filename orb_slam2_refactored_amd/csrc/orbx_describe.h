// orbx_describe.h — stage 4 of orbx.hip: one wavefront per kept keypoint: IC_Angle on the raw level
// (:74-101), GaussianBlur 7x7 s2 Q8 REFLECT_101 of the 43x43 neighbourhood in LDS (:799), rotated rBRIEF
// (:103-140) packed with wave ballots; octave / size / scale written in the reference's output order.
// describe_prefix_kernel: the per-frame level prefix; describe_kernel: the slot-table grid or the dense
// grid (ORBX_DESC_DENSE=1) with describe_overflow_kernel.
#pragma once
#include <cfloat>

#include "orbx_fast.h"   // us2, u2us
#include "orbx_geom.h"
#include "sincos_f.h"

namespace orbamd {

__device__ __forceinline__ float fast_atan2_dev(float y, float x) {
    const float k = (float)(180 / M_PI);
    const float p1 = 0.9997878412794807f * k, p3 = -0.3258083974640975f * k;
    const float p5 = 0.1555786518463281f * k, p7 = -0.04432655554792128f * k;
    // the reference's two branches (ax >= ay: ay / ax, else 90 - f(ax / ay)) with one division:
    // the same operations on the same operands
    const float ax = fabsf(x), ay = fabsf(y);
    const bool xm = ax >= ay;
    const float c = (xm ? ay : ax) / ((xm ? ax : ay) + (float)DBL_EPSILON);
    const float c2 = c * c;
    float a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    if (!xm) a = 90.f - a;
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

__device__ __forceinline__ int reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) {
        if (i < 0) i = -i;
        if (i >= n) i = 2 * n - 2 - i;
    }
    return i;
}

constexpr int RS = 48;   // LDS raw-patch row stride (16-byte aligned rows for the blur's b128 reads)

// Horizontal Q8 blur as v_mfma_i32_16x16x64_i8 products C[m][n] = sum_k A[m][k] B[k][n]: m = blurred
// column, n = patch row, k = raw column; A = the 7-tap Toeplitz band A[m][k] = K[k - m]
// (K = 18 34 48 56 48 34 18), B = raw pixels as i8 (p - 128; sum K = 256, so the accumulator starts
// at 128 * 256).  Lane l holds A rows m = l % 16 (+16 mt), k = 16 (l / 16) .. +15 — the same k
// split as its B bytes, so the hardware's k order inside a lane group does not matter.
struct HBlurA { uint32_t v[3][64][4]; };   // [m tile][lane][dword]
constexpr HBlurA make_hblur_a() {
    HBlurA t{};
    const int K[7] = {18, 34, 48, 56, 48, 34, 18};
    for (int mt = 0; mt < 3; mt++)
        for (int l = 0; l < 64; l++)
            for (int d = 0; d < 4; d++) {
                uint32_t w = 0;
                for (int b = 0; b < 4; b++) {
                    const int o = 16 * (l >> 4) + 4 * d + b - (l & 15) - 16 * mt;
                    if (o >= 0 && o < 7) w |= (uint32_t)K[o] << (8 * b);
                }
                t.v[mt][l][d] = w;
            }
    return t;
}

// IC_Angle (:74-101) as the same i8 products on the blur's B fragments: D_t = A_t B_nt chained over
// the three row tiles, with A_t[m][k] = the disk weight of patch pixel (row m + 16 nt, column k) —
// u = k - 21 for m_10, v = m + 16 nt - 21 for m_01, 0 outside the disk |v| <= 15, |u| <= umax[|v|].
// The diagonal D[n][n] is then the weighted sum of patch row n (+16 nt), and its trace the moment.
// The disk is symmetric in u and in v, so sum(weights) = 0 and the i8 offset (p - 128) cancels.
struct AngleA { uint32_t v[3][2][64][4]; };   // [row tile][m_10, m_01][lane][dword]
constexpr AngleA make_angle_a() {
    AngleA t{};
    for (int nt = 0; nt < 3; nt++)
        for (int l = 0; l < 64; l++)
            for (int d = 0; d < 4; d++)
                for (int b = 0; b < 4; b++) {
                    const int v = (l & 15) + 16 * nt - 21, u = 16 * (l >> 4) + 4 * d + b - 21;
                    const int av = v < 0 ? -v : v, au = u < 0 ? -u : u;
                    if (av > 15 || au > c_umax_h[av]) continue;
                    t.v[nt][0][l][d] |= (uint32_t)(uint8_t)(int8_t)u << (8 * b);
                    t.v[nt][1][l][d] |= (uint32_t)(uint8_t)(int8_t)v << (8 * b);
                }
    return t;
}
// describe's constant tables in ONE symbol, read through one buffer resource (a lane's 16 bytes at
// lane * 16 + a compile-time offset): one address materialisation instead of one s_getpc + 64-bit add per
// table load (13 loads, ~39 SALU instructions per keypoint wave, in a kernel bound by SALU issue; round 6)
struct DescTabs {
    HBlurA hb;                              // 3 KiB
    AngleA an;                              // 6 KiB
    float pat[1024];                        // bit_pattern_31_ (:142-400) as floats (the samples' operands), 4 KiB
};
__constant__ __attribute__((aligned(16))) DescTabs c_desc_tabs = {make_hblur_a(), make_angle_a(), {
#include "orb_pattern31.inc"
}};
constexpr int DT_HB = 0, DT_AN = 3 * 1024, DT_PAT = 9 * 1024;
// the fdlibm sincos constants as a __constant__ copy: scalar loads instead of two s_mov_b32 per double
__constant__ __attribute__((aligned(16))) SincosK c_sincos_k = kSincosK;
static_assert(sizeof(HBlurA) == 3 * 1024 && sizeof(AngleA) == 6 * 1024, "table offsets");
typedef int i4v __attribute__((ext_vector_type(4)));

#ifdef ORB_DESC_STAMPS
// diagnostic build: phase stamps of every 16th describe wavefront (8 words each)
__device__ unsigned long long g_desc_stamps[1024 * 8];
#define DESC_STAMP(k)                                                                              \
    do {                                                                                           \
        if (lane == 0 && (lb & 15) == 0 && (lb >> 4) < 1024) g_desc_stamps[(lb >> 4) * 8 + (k)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define DESC_STAMP(k) do {} while (0)
#endif

// One workgroup = one wavefront = one selection slot (a kept keypoint or an empty slot).
constexpr int PATCH_DW = (PATCH + 3) / 4;                 // dwords staged per raw-patch row
#ifndef DESC_ANGLE_MFMA
#define DESC_ANGLE_MFMA 1   // IC_Angle as i8 products on the blur's B fragments (0: LDS disk reads; A/B)
#endif
// column-major blurred patch: column c (0..39) holds rows 0..47 at u16 c * HCS; 26 dwords per column
// put the 16 columns of one b64 store group on distinct bank pairs
constexpr int HCS = 52;
static_assert(HCS % 4 == 0 && HCS >= 48, "8-byte aligned columns of 48 rows (the tiles' slack rows)");
constexpr int HB_ELEMS = 40 * HCS;

// One kept keypoint (level l, selection word k, output row o of the frame's slots): the raw 43x43 patch,
// IC_Angle, the 7x7 Q8 blur and the rBRIEF samples, written to kps / desc at row o.  One wavefront.
template <int TRIG>
__device__ __forceinline__ void describe_keypoint(const Geom& g, int l, int f, uint32_t k, long long o,
                                                  const uint8_t* __restrict__ in, long long in_fstride, int in_step,
                                                  const uint8_t* __restrict__ pyr, orbx_keypoint* __restrict__ kps,
                                                  uint8_t* __restrict__ desc, uint16_t* Hb, int lb) {
    const int lane = threadIdx.x;
    uint8_t* R = reinterpret_cast<uint8_t*>(Hb);
    const LevelDev& L = g.lv[l];
    const __amdgpu_buffer_rsrc_t trs =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<DescTabs*>(&c_desc_tabs), 0, (int)sizeof(DescTabs), 0x00020000);
    // a lane's 16 bytes of 1 KiB table row `row` (hb: mt; an: 2 nt + moment; pat: r), constant offsets
    auto tab16 = [&](int off) -> i4v {
        return __builtin_bit_cast(i4v, __builtin_amdgcn_raw_buffer_load_b128(trs, off + 16 * lane, 0, 0));
    };
    DESC_STAMP(0);
    // the blur's constant A fragments, in flight under the patch load
    i4v afr[3];
#pragma unroll
    for (int mt = 0; mt < 3; mt++) afr[mt] = tab16(DT_HB + 1024 * mt);

    const int kx = kp_x(k), ky = kp_y(k), score = kp_s(k);
    // the level's base and row step: both candidates' operands come with the kernel arguments' first
    // scalar round trip, and the selection is an s_cselect (no branch to a second round trip)
    const uint8_t* img0 = in + (long long)f * in_fstride;
    const uint8_t* imgl = pyr + (long long)f * g.pyr_frame_bytes + L.off;
    const uint8_t* img = l == 0 ? img0 : imgl;
    const int step = l == 0 ? in_step : L.stride;
    // 43x43 neighbourhood (reflect-101 outside the level, as the blur's BORDER_REFLECT_101)
    if (kx >= 21 && ky >= 21 && kx + 21 + 8 < L.w && ky + 21 < L.h) {
        // interior: 16 lanes per row (dword d of row 4k + lane/16), 11 row groups; all loads in
        // flight before the LDS stores
        constexpr int NG = (PATCH + 3) / 4;
        const uint8_t* base = img + (long long)(ky - 21) * step + (kx - 21);
        const int roff = lane >> 4, d = min(lane & 15, PATCH_DW - 1);
        uint32_t v[NG];
        if ((step & 3) == 0) {
            // dword-multiple row step (every pyramid level; level 0 unless the caller's step is
            // odd): one wave-uniform realignment, buffer loads off a scalar resource with a per-lane
            // constant voffset and a per-group soffset (no address VALU).  The resource ends at the
            // level's last pixel: row 43 of the last group (never stored) may lie past it and reads 0.
            const int m = __builtin_amdgcn_readfirstlane((int)(reinterpret_cast<uintptr_t>(base) & 3u));
            const int nrec = (L.h - 1 - (ky - 21)) * step + L.w - (kx - 21) + m;
            const __amdgpu_buffer_rsrc_t rs =
                __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t*>(base - m), 0, nrec, 0x00020000);
            const int voff = roff * step + 4 * d;
#pragma unroll
            for (int k = 0; k < NG; k++) {
                const auto t = __builtin_amdgcn_raw_buffer_load_b64(rs, voff, 4 * k * step, 0);
                v[k] = __builtin_amdgcn_alignbyte(t[1], t[0], m);
            }
        } else {
            // odd caller step: a per-lane realignment (v_alignbyte of the aligned dword pair)
            const int loff = roff * step + 4 * d;
            uint32_t lo[NG], hi[NG];
            int sh[NG];
#pragma unroll
            for (int k = 0; k < NG; k++) {
                const uint8_t* gb = base + (long long)min(4 * k, PATCH - 1 - roff) * step;   // rows <= 42
                const uint8_t* pbyte = gb + loff;
                const int m = (int)(reinterpret_cast<uintptr_t>(pbyte) & 3);
                const uint32_t* pw = reinterpret_cast<const uint32_t*>(pbyte - m);
                lo[k] = pw[0];
                hi[k] = pw[1];
                sh[k] = m;
            }
#pragma unroll
            for (int k = 0; k < NG; k++) v[k] = __builtin_amdgcn_alignbyte(hi[k], lo[k], sh[k]);
        }
        static_assert(4 * (NG - 1) + 3 == PATCH, "the last row group holds three patch rows");
        if ((lane & 15) < PATCH_DW) {
            uint32_t* rrow = reinterpret_cast<uint32_t*>(&R[roff * RS + 4 * d]);
#pragma unroll
            for (int k = 0; k < NG - 1; k++) rrow[k * RS] = v[k];   // row 4k + roff: (4k + roff) * RS / 4 dwords
            if (roff < 3) rrow[(NG - 1) * RS] = v[NG - 1];
        }
    } else if (lane < PATCH) {
        const int xx = reflect101(kx - 21 + lane, L.w);
        uint8_t v[PATCH];
#pragma unroll
        for (int r = 0; r < PATCH; r++) v[r] = img[(long long)reflect101(ky - 21 + r, L.h) * step + xx];
#pragma unroll
        for (int r = 0; r < PATCH; r++) R[r * RS + lane] = v[r];
    }
    __syncthreads();
    DESC_STAMP(1);

#if !DESC_ANGLE_MFMA   // the round-3 IC_Angle (LDS disk reads), for A/B builds
    // IC_Angle on the unblurred level, patch centre (21, 21).  Lane = (row parity, u + 15): lanes
    // 0-31 take rows +-v for odd v, lanes 32-63 for v + 1, so the 15 row pairs take 8 steps.
    int m10 = 0, m01 = 0;
    {
        const int hv = lane >> 5, u = (lane & 31) - 15;   // u = 16 on lanes 31 / 63: outside every umax
        const uint8_t* cp = R + 21 * RS + 21 + u + hv * RS;
        // every read unconditional (all inside the 43x43 patch) and issued together; the disk mask
        // is applied to the products
        int vp[8], vm[8];
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const int vv = 2 * t + 1;
            vp[t] = cp[vv * RS];
            vm[t] = cp[-(vv + 2 * hv) * RS];
        }
        const int c0 = R[21 * RS + 21 + u];
        m10 = (hv == 0 && u <= 15) ? u * c0 : 0;
        // the disk mask as lane-constant multipliers (branch-free multiply-adds)
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const int vv = 2 * t + 1;
            const int v = vv + hv;
            const int um = hv ? (vv + 1 <= 15 ? c_umax_h[vv + 1] : -1) : c_umax_h[vv];
            const bool in = u >= -um && u <= um;
            const int vin = in ? v : 0, uin = in ? u : 0;
            m01 += vin * (vp[t] - vm[t]);
            m10 += uin * (vp[t] + vm[t]);
        }
    }
    m10 = wave_sum_i32(m10);
    m01 = wave_sum_i32(m01);
#endif
    // The raw rows as i8 B fragments (p - 128), shared by the angle and the blur products: lane
    // (n, g) holds columns 16 g .. +15 of patch row n + 16 nt.  Every read of R is issued before the
    // first Hb write (R aliases Hb; one wavefront's LDS operations complete in order).
    const int n = lane & 15, lg = lane >> 4;
    i4v bfr[3];
#pragma unroll
    for (int nt = 0; nt < 3; nt++) {
        bfr[nt] = *reinterpret_cast<const i4v*>(&R[(n + 16 * nt) * RS + 16 * lg]);
        bfr[nt] ^= (int)0x80808080u;
    }

#if DESC_ANGLE_MFMA
    // IC_Angle on the unblurred patch, centre (21, 21), as six more products (c_angle_a) chained
    // over the row tiles; the diagonal element D[n][n] sits in lane 20 (n / 4) + n % 4, register
    // n % 4: each lane takes register lane % 4, and the quads at row offset 4 (lane / 16) are summed.
    int m10 = 0, m01 = 0;
    auto angle_products = [&](const i4v (&au)[3], const i4v (&av)[3]) {
        i4v du = {0, 0, 0, 0}, dv = {0, 0, 0, 0};
#pragma unroll
        for (int nt = 0; nt < 3; nt++) {
            du = __builtin_amdgcn_mfma_i32_16x16x64_i8(au[nt], bfr[nt], du, 0, 0, 0);
            dv = __builtin_amdgcn_mfma_i32_16x16x64_i8(av[nt], bfr[nt], dv, 0, 0, 0);
        }
        const bool q1 = lane & 1, q2 = lane & 2;
        int tu = q2 ? (q1 ? du.w : du.z) : (q1 ? du.y : du.x);
        int tv = q2 ? (q1 ? dv.w : dv.z) : (q1 ? dv.y : dv.x);
        tu += dpp_i32<0xB1>(tu);   // quad_perm [1,0,3,2]
        tv += dpp_i32<0xB1>(tv);
        tu += dpp_i32<0x4E>(tu);   // quad_perm [2,3,0,1]
        tv += dpp_i32<0x4E>(tv);
        m10 = __builtin_amdgcn_readlane(tu, 0) + __builtin_amdgcn_readlane(tu, 20) +
              __builtin_amdgcn_readlane(tu, 40) + __builtin_amdgcn_readlane(tu, 60);
        m01 = __builtin_amdgcn_readlane(tv, 0) + __builtin_amdgcn_readlane(tv, 20) +
              __builtin_amdgcn_readlane(tv, 40) + __builtin_amdgcn_readlane(tv, 60);
    };
#endif

    // horizontal Q8 blur on the matrix cores (c_hblur_a): 3 x 3 tiles of 16 blurred columns x 16
    // rows; lane (n, g) of tile (mt, nt) gets columns 16 mt + 4 g .. +3 of row 16 nt + n.  Rows past
    // 42 (stored into slack rows) and columns past 36 are computed from neighbouring bytes and never
    // read; columns past 39 are not stored.
    {
        const i4v cinit = {128 * 256, 128 * 256, 128 * 256, 128 * 256};
        i4v acc[3][3];   // all nine products first: their results are not waited on one at a time
#pragma unroll
        for (int nt = 0; nt < 3; nt++)
#pragma unroll
            for (int mt = 0; mt < 3; mt++)
                // the transposed product (patch rows as A, the blur band as B: the same k pairing):
                // lane (n, g) gets rows 16 nt + 4 g .. +3 of blurred column 16 mt + n
                acc[nt][mt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bfr[nt], afr[mt], cinit, 0, 0, 0);
        auto put = [&](int nt, int mt) {
            uint2 pk;
            pk.x = __builtin_amdgcn_perm((uint32_t)acc[nt][mt].y, (uint32_t)acc[nt][mt].x, 0x05040100u);
            pk.y = __builtin_amdgcn_perm((uint32_t)acc[nt][mt].w, (uint32_t)acc[nt][mt].z, 0x05040100u);
            *reinterpret_cast<uint2*>(&Hb[(16 * mt + n) * HCS + 16 * nt + 4 * lg]) = pk;   // rows 43..47: slack
        };
#pragma unroll
        for (int nt = 0; nt < 3; nt++) {
            put(nt, 0);
            put(nt, 1);
        }
        if (n < 8) {   // columns 32..39 of the third tile
#pragma unroll
            for (int nt = 0; nt < 3; nt++) put(nt, 2);
        }
    }

    // the lane's four pattern pairs, loaded before the angle / atan / sincos chain hides their latency
    float4 pat[4];
#pragma unroll
    for (int r = 0; r < 4; r++) pat[r] = __builtin_bit_cast(float4, tab16(DT_PAT + 1024 * r));
#if DESC_ANGLE_MFMA
    {
        i4v au[3], av[3];
#pragma unroll
        for (int nt = 0; nt < 3; nt++) {
            au[nt] = tab16(DT_AN + 1024 * (2 * nt));
            av[nt] = tab16(DT_AN + 1024 * (2 * nt + 1));
        }
        angle_products(au, av);
    }
#endif
    const float angle = fast_atan2_dev((float)m01, (float)m10);
    DESC_STAMP(2);
    __syncthreads();

    const float factorPI = (float)(M_PI / 180.f);
    const float ang = angle * factorPI;
    float a, b;   // (float)::cos / ::sin((double)ang) or cosf / sinf, sincos_f.h (each checked on every float in range)
    DESC_STAMP(3);
    if (TRIG) sincosf_glibc(ang, &b, &a);
    else sincos_f2d_k(ang, &b, &a, c_sincos_k);
    DESC_STAMP(4);
    auto sample = [&](float x, float y) -> int {
        // byte offset of blurred pixel (18 + dy, 18 + dx) from the rounded floats (exact integers)
        const float dy = rintf(x * b + y * a), dx = rintf(x * a - y * b);
        // u16 index of blurred pixel (18 + dy, 18 + dx) in the column-major map; its 7 vertical taps
        // (rows 18 + dy .. +6) are u16 q .. q + 6, inside dwords q / 2 .. q / 2 + 3, realigned by q's parity
        const int q = (int)fmaf(dx, (float)HCS, dy + (float)(18 * HCS + 18));
        const uint32_t* cw = reinterpret_cast<const uint32_t*>(Hb) + (q >> 1);
        const uint32_t d0 = cw[0], d1 = cw[1], d2 = cw[2], d3 = cw[3];
        const uint32_t sh = (uint32_t)(q & 1) * 2u;   // bytes
        const us2 p01 = u2us(__builtin_amdgcn_alignbyte(d1, d0, sh));
        const us2 p23 = u2us(__builtin_amdgcn_alignbyte(d2, d1, sh));
        const us2 p45 = u2us(__builtin_amdgcn_alignbyte(d3, d2, sh));
        const us2 p6x = u2us(__builtin_amdgcn_alignbyte(d3, d3, sh));   // tap 6 in the low half
        const us2 k01 = {18, 34}, k23 = {48, 56}, k45 = {48, 34}, k6x = {18, 0};
        unsigned acc = __builtin_amdgcn_udot2(p6x, k6x, 1u << 15, false);
        acc = __builtin_amdgcn_udot2(p01, k01, acc, false);
        acc = __builtin_amdgcn_udot2(p23, k23, acc, false);
        acc = __builtin_amdgcn_udot2(p45, k45, acc, false);
        return (int)(acc >> 16);
    };
    unsigned long long words[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const float4 q = pat[r];
        words[r] = __ballot(sample(q.x, q.y) < sample(q.z, q.w));
    }
    DESC_STAMP(5);
    // The 32 descriptor bytes and the 7-word keypoint record are wave-uniform: v_writelane places
    // them in lanes 0..7 / 0..6 of one register each (no per-lane selects or branches), one store each.
    uint32_t dv = 0, kv = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        dv = writelane_u32((uint32_t)words[r], 2 * r, dv);
        dv = writelane_u32((uint32_t)(words[r] >> 32), 2 * r + 1, dv);
    }
    const float ks = l > 0 ? L.scale : 1.f;   // (:812-815: pt *= scaleFactors_[s] above level 0; x * 1 = x)
    kv = writelane_u32(__float_as_uint((float)kx * ks), 0, kv);
    kv = writelane_u32(__float_as_uint((float)ky * ks), 1, kv);
    kv = writelane_u32(__float_as_uint(L.size), 2, kv);
    kv = writelane_u32(__float_as_uint(angle), 3, kv);
    kv = writelane_u32(__float_as_uint((float)score), 4, kv);
    kv = writelane_u32((uint32_t)l, 5, kv);
    kv = writelane_u32(0xffffffffu, 6, kv);
    if (lane < 8) reinterpret_cast<uint32_t*>(desc + o * 32)[lane] = dv;
    if (lane < 7) reinterpret_cast<uint32_t*>(kps + o)[lane] = kv;
    DESC_STAMP(6);
}

constexpr int LVP = 32;   // per-frame stride (ints) of describe's level prefix (nlevels + 1 <= 17 used; 128 B rows)

// Per frame: the exclusive prefix of the kept counts over levels (lvl_pre[f][l] = first output row of level
// l, lvl_pre[f][nl] = the frame's total) and counts[f].  One thread per frame, between the quadtree and
// describe; it takes the per-level sums out of every describe wavefront's scalar preamble (round 6: the
// 16-count load, the level compare chain and the prefix sum were ~150 of a wave's ~330 SALU instructions,
// and describe was SALU-issue-bound, SALUBusy 83 %).
// stat[0]: the batch's largest frame total (atomicMax; the host sizes the next batch's dense describe grid
// from it).
__global__ __launch_bounds__(256) void describe_prefix_kernel(const int* __restrict__ sel_cnt, int nl, int F,
                                                              int* __restrict__ lvl_pre, int32_t* __restrict__ counts,
                                                              int* __restrict__ stat) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    int acc = 0;
    int* pre = lvl_pre + (long long)f * LVP;
    for (int q = 0; q < nl; q++) {
        pre[q] = acc;
        acc += sel_cnt[f * nl + q];
    }
    pre[nl] = acc;
    counts[f] = acc;
    atomicMax(stat, acc);
}

// The dense describe grid (round 6): launch slot s of frame f IS output row s.  Its level is the number of
// levels 1..nl whose first row is <= s (one vector load of the frame's prefix, one ballot), its rank in the
// level s - pre[l], its selection word sel[f][out_base_l + rank].  A launch of C slots per frame covers the
// frames with at most C keypoints; C comes from the previous batch's largest total (stat[0]), so the grid
// no longer carries every level's out_cap slack (2024 slots for ~1395 keypoints per C2 pan frame, 31 % of
// the wavefronts empty), and describe_overflow_kernel covers rows >= C of any frame that has more.
struct DescGrid {
    int C;                 // slots per frame in this launch
    unsigned m;            // lb / C by the round-up magic (as divmod_of)
    int s1, s2;
};
template <int TRIG>
__device__ __forceinline__ void describe_dense_slot(const Geom& g, int f, int s, const uint8_t* __restrict__ in,
                                                    long long in_fstride, int in_step, const uint8_t* __restrict__ pyr,
                                                    const uint32_t* __restrict__ sel, orbx_keypoint* __restrict__ kps,
                                                    uint8_t* __restrict__ desc, int cap, const int* __restrict__ lvl_pre,
                                                    uint16_t* Hb, int lb) {
    const int lane = threadIdx.x, nl = g.nlevels;
    const int pq = lane <= nl ? lvl_pre[(long long)f * LVP + lane] : 0x7fffffff;
    const int T = __builtin_amdgcn_readlane(pq, nl);
    if (s >= T || s >= cap) return;   // wave-uniform
    const int l = popc64(__ballot(lane >= 1 && lane <= nl && pq <= s));
    const int pre_l = __builtin_amdgcn_readlane(pq, l);
    const uint32_t k = sel[(long long)f * g.out_frame + g.lv[l].out_base + (s - pre_l)];
    describe_keypoint<TRIG>(g, l, f, k, (long long)f * cap + s, in, in_fstride, in_step, pyr, kps, desc, Hb, lb);
}

// Rows >= C of the frames whose total exceeds the dense launch's C: a fixed grid of one-wave workgroups
// loops over the frames (wave w: frames w, w + grid, ...) and their extra rows.  Exits at once when no
// frame overflows.
template <int TRIG>
__global__ __launch_bounds__(64) void describe_overflow_kernel(Geom g, const uint8_t* __restrict__ in,
                                                               long long in_fstride, int in_step,
                                                               const uint8_t* __restrict__ pyr,
                                                               const uint32_t* __restrict__ sel,
                                                               orbx_keypoint* __restrict__ kps,
                                                               uint8_t* __restrict__ desc, int cap,
                                                               const int* __restrict__ lvl_pre, int F, int C) {
    __shared__ __attribute__((aligned(16))) uint16_t Hb[HB_ELEMS];
    for (int f = blockIdx.x; f < F; f += gridDim.x) {
        const int T = min(lvl_pre[(long long)f * LVP + g.nlevels], cap);
        for (int s = C; s < T; s++) {
            describe_dense_slot<TRIG>(g, f, s, in, in_fstride, in_step, pyr, sel, kps, desc, cap, lvl_pre, Hb,
                                      (int)blockIdx.x);
            __syncthreads();   // Hb is reused by the next row
        }
    }
}

// One wavefront per selection slot of a frame; slots past their level's kept count exit at once.
// TRIG: ComputeOrbDescriptor's cos / sin (:107): 0 = (float)::cos((double)angle), 1 = cosf / sinf.
template <int TRIG>
__global__ __launch_bounds__(64) void describe_kernel(Geom g, const uint8_t* __restrict__ in, long long in_fstride,
                                                      int in_step, const uint8_t* __restrict__ pyr,
                                                      const uint32_t* __restrict__ sel,
                                                      const int* __restrict__ sel_cnt, orbx_keypoint* __restrict__ kps,
                                                      uint8_t* __restrict__ desc, int32_t* __restrict__ counts,
                                                      int cap, const uint32_t* __restrict__ slot_tab,
                                                      const int* __restrict__ lvl_pre, DescGrid dg) {
    // the raw patch R is dead once every lane holds its row for the horizontal blur (one
    // wavefront: its LDS reads complete before its later writes), so the blurred rows Hb reuse it
    __shared__ __attribute__((aligned(16))) uint16_t Hb[HB_ELEMS];   // 43 blurred rows + 5 rows of blur slack
    static_assert(47 * RS + 64 <= HB_ELEMS * 2, "R (and the blur's reads of rows 43..47) must fit in Hb");
    const int lane = threadIdx.x;
    const int lb = xcd_swizzle(blockIdx.x + gridDim.x * blockIdx.y, gridDim.x * gridDim.y);
    DESC_STAMP(7);   // entry (diagnostic build): the preamble's loads are timed from here
    if (dg.C > 0) {   // the dense grid (DescGrid): slot = output row
        const unsigned t = __umulhi((unsigned)lb, dg.m);
        const int fd = (int)((t + (((unsigned)lb - t) >> dg.s1)) >> dg.s2);
        (void)sel_cnt; (void)counts; (void)slot_tab;
        describe_dense_slot<TRIG>(g, fd, lb - fd * dg.C, in, in_fstride, in_step, pyr, sel, kps, desc, cap, lvl_pre, Hb,
                                  lb);
        return;
    }
    const int f = divmod_of(g, lb);
    const int s = lb - f * g.out_frame;   // selection slot (level-major, out_cap slots per level)
    // slot -> (level, rank in the level) from the host's table, the level's output rows from the frame's
    // prefix (describe_prefix_kernel, which also wrote counts[f]): three scalar loads, no sums
    (void)sel_cnt;
    (void)counts;
    (void)lane;
    const uint32_t e = slot_tab[s];
    const uint32_t k = sel[(long long)f * g.out_frame + s];
    // both words in one scalar round trip (the compiler would sink k's load past the exits below, into a
    // third dependent round trip on every kept keypoint's chain)
    asm volatile("" ::"s"(e), "s"(k), "s"(cap), "s"(in), "s"(in_fstride), "s"(in_step), "s"(pyr), "s"(g.pyr_frame_bytes));
    const int l = (int)(e & 255u), i = (int)(e >> 8);
    const int2 pr = *reinterpret_cast<const int2*>(lvl_pre + (long long)f * LVP + l);
    {   // the level's fields describe_keypoint reads, in the same round trip as the prefix (kernarg, CSE'd)
        const LevelDev& L = g.lv[l];
        asm volatile("" ::"s"(pr.x), "s"(pr.y), "s"(L.w), "s"(L.h), "s"(L.stride), "s"(L.off));
    }
    if (i >= pr.y - pr.x) return;   // slot past the level's kept count
    const int oidx = pr.x + i;      // output order: level-major list order
    if (oidx >= cap) return;
    describe_keypoint<TRIG>(g, l, f, k, (long long)f * cap + oidx, in, in_fstride, in_step, pyr, kps, desc, Hb, lb);
}

}  // namespace orbamd
