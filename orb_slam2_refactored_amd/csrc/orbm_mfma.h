// orbm_mfma.h — the matrix-core matcher (included by orbm.hip): the operand expansions, the LDS layouts,
// the running top-2 (update, chunk -> global keys, row merge, result write), the two brute-force top-2
// kernels and their launch.  orbm_tri.h's tri_mm_kernel runs the same FP4 tile stream.
//
// Brute-force top-2 with the reference's scan semantics (SearchByBoW inner loop,
// src/ORBmatcher.cc:477-498).  For 0/1 bit vectors, Hamming(a, b) = |a| + |b| - 2<a, b>
// (DescriptorDistance, :1449-1457), and <a, b> over the 256 bits is an exact int32 dot product of bytes:
// bits are expanded to 0/1 bytes in registers and fed to v_mfma_i32_16x16x64_i8 (4 k-steps per 256 bits).
// Any k permutation applied identically to the A and B fragments leaves the dot product unchanged, so
// lane l (group g = l >> 4) simply takes descriptor bytes 8g..8g+7 and k-step s their bits 16s..16s+15.
// A's bits are expanded to int8 0 / -128, B's to 0 / 2, and the accumulator starts at 128 (|b| + 256) + t
// for column tile t of a 2048-column chunk, so the MFMA yields the key 128 S + t with S = d - |a| + 256 in
// [0, 512] directly (a lane holds one column class, so t is its column).  The running best key is the
// minimum (lowest j on equal d, as the reference's strict-< scan) and the running second key the second
// order statistic.  Chunk keys become global keys S << 16 | j for the cross-lane merge; after it
// d = S - 256 + |a|; keys with d >= 256 (d == 256 and the padding columns) never displace a real
// candidate and are mapped back to (256, -1), which is the reference's bestDist = 256 / bestIdx = -1
// initialisation.
//
// The tile stream (column tiles of 16 consumed in pairs, the pair's expansion shared by the 4 wavefronts
// through an LDS double buffer, the pair after next prefetched into registers) is written out in each of
// the three kernels that run it: as one inlined template over the operand form it compiled to other
// instruction schedules of all of them (same instruction counts, the prologue and the loop's LDS reads
// reordered), and these kernels only change together with a timing on the device.
#pragma once

namespace orbamd {

typedef int i4v __attribute__((ext_vector_type(4)));
typedef int i8v __attribute__((ext_vector_type(8)));
typedef float f4v __attribute__((ext_vector_type(4)));

__device__ __forceinline__ i4v expand16(uint32_t b) {   // bit k of b -> byte k (0 / 1)
    i4v r;
    r.x = (int)(((b & 0xfu) * 0x00204081u) & 0x01010101u);
    r.y = (int)((((b >> 4) & 0xfu) * 0x00204081u) & 0x01010101u);
    r.z = (int)((((b >> 8) & 0xfu) * 0x00204081u) & 0x01010101u);
    r.w = (int)((((b >> 12) & 0xfu) * 0x00204081u) & 0x01010101u);
    return r;
}

__device__ __forceinline__ uint32_t chunk16(uint2 v, int s) {
    return ((s < 2 ? v.x : v.y) >> (16 * (s & 1))) & 0xffffu;
}

__device__ __forceinline__ int popc_row(const uint8_t* r) {
    const uint4 a = reinterpret_cast<const uint4*>(r)[0], b = reinterpret_cast<const uint4*>(r)[1];
    return __popc(a.x) + __popc(a.y) + __popc(a.z) + __popc(a.w) + __popc(b.x) + __popc(b.y) + __popc(b.z) +
           __popc(b.w);
}

__device__ __forceinline__ int hamming8(const uint4& a0, const uint4& a1, const uint4& b0, const uint4& b1) {
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// The block-scaled FP4 matrix path (v_mfma_scale_f32_16x16x128_f8f6f4, e2m1 operands: K = 128 per
// instruction, twice the i8 form's K at the same issue cost, and half the expanded bytes).  A bit becomes
// a nibble: A's 1 -> -4 with block scale 2^6 (-256), B's 1 -> 1.0 with scale 2^0, so a common bit
// contributes -256 and, with the f32 accumulator started at 128 (|b| + 256) + t (exact: every value is an
// integer below 2^17), the MFMA again yields the chunk key 128 S + t, now as an f32.  The keys are
// non-negative, so their bit patterns order as the values: the running min / median run on the raw
// bits, converted to integers once per chunk.  Lane group g takes descriptor bytes 8g..8g+7; k-step m
// its bits 32m..32m+31.
__device__ __forceinline__ uint32_t spread8(uint32_t b) {   // bit i of the low byte -> bit 4i
    uint32_t x = b & 0xffu;
    x = (x | (x << 12)) & 0x000f000fu;
    x = (x | (x << 6)) & 0x03030303u;
    x = (x | (x << 3)) & 0x11111111u;
    return x;
}
__device__ __forceinline__ i4v expand32_nib(uint32_t b, uint32_t nib) {   // bit k of b -> nibble k (0 / nib)
    i4v r;
    r.x = (int)(spread8(b) * nib);
    r.y = (int)(spread8(b >> 8) * nib);
    r.z = (int)(spread8(b >> 16) * nib);
    r.w = (int)(spread8(b >> 24) * nib);
    return r;
}
constexpr uint32_t FP4_NEG4 = 0xEu, FP4_ONE = 0x2u;    // e2m1: -4.0, 1.0
constexpr int FP4_SCALE_A = 0x85858585, FP4_SCALE_B = 0x7f7f7f7f;   // e8m0: 2^6, 2^0

__device__ __forceinline__ f4v mfma_fp4(i4v a, i4v b, f4v c) {
    const i8v a8 = __builtin_shufflevector(a, a, 0, 1, 2, 3, -1, -1, -1, -1);
    const i8v b8 = __builtin_shufflevector(b, b, 0, 1, 2, 3, -1, -1, -1, -1);
    return __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a8, b8, c, 4, 4, 0, FP4_SCALE_A, 0, FP4_SCALE_B);
}

// ---------------------------------------------------------------------------------------------
// The LDS layouts of the dynamic region, offsets in ints; nBt is the column count padded to whole tile
// pairs and KS the k-steps per 256 bits (i8: 4, FP4: 2).  The kernel carves from the layout and the
// launcher sizes the launch from it.  XB: the double buffer xb[2][2][KS][64] of i4v.
template <int ROWS, int KS>
struct Top2Lds {   // pa[ROWS] | pb[nBt] | pad | xb
    static constexpr int pa = 0, pb = ROWS, XB = 2 * 2 * KS * 64 * 4;
    static __host__ __device__ constexpr int xb(int nBt) { return (ROWS + nBt + 16 + 3) & ~3; }
    static constexpr size_t bytes(int nBt) { return (size_t)(xb(nBt) + XB) * sizeof(int); }
};

template <int ROWS, int POOL>
struct TriMmLds {   // row (float4) | best | ovf | pa | ev[4 wavefronts][POOL] | xb (FP4) | pb[nBt]
    static constexpr int row = 0, best = 4 * ROWS, ovf = 5 * ROWS, pa = 6 * ROWS, ev = 7 * ROWS, xb = ev + 4 * POOL,
                         pb = xb + 2 * 2 * 2 * 64 * 4;
    static constexpr size_t bytes(int nBt) { return (size_t)(pb + nBt) * sizeof(int); }
};

// ---------------------------------------------------------------------------------------------
// The running top-2 of a lane, per accumulator element (row 16 rt + 4 g + r, the lane's column class): the
// chunk's best and second chunk key (lb, ls) and, across chunks, the global keys S << 16 | j (bk, sk).

// The median of (a, key, c), ordered after `dep`.  `key` is an MFMA result: the compiler's hazard recognizer
// does not see reads inside inline asm, so the asm must come after a compiler-generated read of
// the same register (the `min` that produces `dep`), which carries the MFMA -> VALU wait states.
__device__ __forceinline__ uint32_t umed3_after(uint32_t a, uint32_t key, uint32_t c, uint32_t dep) {
    uint32_t r;
    asm volatile("v_med3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(key), "v"(c), "v"(dep));
    return r;
}

__device__ __forceinline__ void top2_update(uint32_t& lb, uint32_t& ls, uint32_t key) {
    // lb <= ls always, so the new second order statistic min(ls, max(lb, key))
    // is the median of the three
    const uint32_t nb = min(lb, key);
    ls = umed3_after(lb, key, ls, nb);
    lb = nb;
}

constexpr int MM_CHUNK = 2048;   // columns per chunk key range (128 tiles of 16)

// The chunk's top-2 as global keys (b2, s2v): with MULTI (more than MM_CHUNK columns) merged into the top-2
// carried across chunks.  The chunk -> global key step stays in each kernel: shared, the single-chunk
// kernels' v_or3 operands came out in the other order.
template <bool MULTI>
__device__ __forceinline__ void top2_end_chunk(uint32_t& bk, uint32_t& sk, uint32_t b2, uint32_t s2v) {
    if (MULTI) {
        sk = min(min(sk, s2v), max(bk, b2));
        bk = min(bk, b2);
    } else {
        bk = b2;
        sk = s2v;
    }
}

// Merges the 16 column classes of each row (lanes with the same g) and writes the rows' results.  The
// top-2 merge is associative and commutative, so the 16 lanes of a row combine in any tree: DPP quad_perm
// [1,0,3,2], [2,3,0,1], then row_ror 4 and 8.  rl0: the wavefront's first row within the workgroup.
template <int RT>
__device__ __forceinline__ void top2_write_rows(const uint32_t (&bk)[RT][4], const uint32_t (&sk)[RT][4], int row_base, int rl0,
                                                const int* s_pa, int g, int c16, int nA, long long out0,
                                                float nnratio, int th_low, int32_t* __restrict__ best_idx,
                                                int32_t* __restrict__ best, int32_t* __restrict__ second,
                                                int32_t* __restrict__ match) {
#pragma unroll
    for (int rt = 0; rt < RT; rt++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            uint32_t b1 = bk[rt][r], s1 = sk[rt][r];
            auto merge = [&](uint32_t b2, uint32_t s2v) {
                s1 = min(min(s1, s2v), max(b1, b2));
                b1 = min(b1, b2);
            };
            merge((uint32_t)__builtin_amdgcn_update_dpp(0, (int)b1, 0xB1, 0xf, 0xf, false),
                  (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s1, 0xB1, 0xf, 0xf, false));
            merge((uint32_t)__builtin_amdgcn_update_dpp(0, (int)b1, 0x4E, 0xf, 0xf, false),
                  (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s1, 0x4E, 0xf, 0xf, false));
            merge((uint32_t)__builtin_amdgcn_update_dpp(0, (int)b1, 0x124, 0xf, 0xf, false),
                  (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s1, 0x124, 0xf, 0xf, false));
            merge((uint32_t)__builtin_amdgcn_update_dpp(0, (int)b1, 0x128, 0xf, 0xf, false),
                  (uint32_t)__builtin_amdgcn_update_dpp(0, (int)s1, 0x128, 0xf, 0xf, false));
            const int row = row_base + rl0 + 16 * rt + 4 * g + r;
            if (c16 == 0 && row < nA) {
                const int pa = s_pa[rl0 + 16 * rt + 4 * g + r];
                const int bdr = (int)(b1 >> 16) - 256 + pa, sdr = (int)(s1 >> 16) - 256 + pa;
                const int bd = bdr >= 256 ? 256 : bdr;
                const int bi = bdr >= 256 ? -1 : (int)(b1 & 0xffffu);
                const int sd = sdr >= 256 ? 256 : sdr;
                const long long o = out0 + row;
                if (best_idx) best_idx[o] = bi;
                if (best) best[o] = bd;
                if (second) second[o] = sd;
                if (match) match[o] = (bd <= th_low && (float)bd < nnratio * (float)sd) ? bi : -1;
            }
        }
}

#ifndef MM_RT_DEF
#define MM_RT_DEF 2
#endif
constexpr int MM_RT = MM_RT_DEF;          // 16-row tiles per wavefront
constexpr int MM_WROWS = 16 * MM_RT;      // query rows per wavefront
constexpr int MM_ROWS = 4 * MM_WROWS;     // query rows per workgroup (4 wavefronts)
typedef Top2Lds<MM_ROWS, 4> MmLds;

template <bool MULTI>   // MULTI: more than MM_CHUNK columns (chunked, global keys kept across chunks)
__global__ __launch_bounds__(256) void hamming_top2_mfma_kernel(
    const uint8_t* __restrict__ A, const int32_t* __restrict__ nA_arr, int nA_fixed, int strideA,
    const uint8_t* __restrict__ B, const int32_t* __restrict__ nB_arr, int nB_fixed, int strideB,
    const int32_t* __restrict__ pair_b, float nnratio, int th_low, int32_t* __restrict__ best_idx,
    int32_t* __restrict__ best, int32_t* __restrict__ second, int32_t* __restrict__ match) {
    extern __shared__ __attribute__((aligned(16))) int mm_sm[];   // MmLds
    int* s_pa = mm_sm + MmLds::pa;
    int* s_pb = mm_sm + MmLds::pb;
    const int p = blockIdx.y;
    const int q = pair_b ? pair_b[p] : p;
    const int nA = nA_arr ? nA_arr[p] : nA_fixed;
    const int nB = nB_arr ? nB_arr[q] : nB_fixed;
    const int row_base = blockIdx.x * MM_ROWS;
    if (row_base >= nA) return;   // block-uniform
    const uint8_t* Ap = A + (long long)p * strideA * 32;
    const uint8_t* Bp = B + (long long)q * strideB * 32;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c16 = lane & 15, g = lane >> 4;
    const int nBt = (nB + 31) & ~31;   // whole pairs of 16-column tiles
    const bool live = __builtin_amdgcn_readfirstlane(row_base + MM_WROWS * w < nA ? 1 : 0) != 0;
    for (int j = tid; j < nBt; j += blockDim.x) s_pb[j] = 128 * ((j < nB ? popc_row(Bp + (long long)j * 32) : 256) + 256);
    {
        const int row = row_base + tid;
        if (tid < MM_ROWS) s_pa[tid] = row < nA ? popc_row(Ap + (long long)row * 32) : 0;
    }
    // A fragments: tile rt rows row_base + 64w + 16rt + c16, bytes 8g..8g+7
    i4v af[MM_RT][4];
#pragma unroll
    for (int rt = 0; rt < MM_RT; rt++) {
        const int row = min(row_base + MM_WROWS * w + 16 * rt + c16, nA - 1);
        const uint2 v = *reinterpret_cast<const uint2*>(Ap + (long long)row * 32 + 8 * g);
#pragma unroll
        for (int s2 = 0; s2 < 4; s2++) af[rt][s2] = expand16(chunk16(v, s2)) * 0x80;   // bit -> int8 0 / -128
    }
    __syncthreads();
    uint32_t bk[MM_RT][4], sk[MM_RT][4], lb[MM_RT][4], ls[MM_RT][4];
#pragma unroll
    for (int rt = 0; rt < MM_RT; rt++)
#pragma unroll
        for (int r = 0; r < 4; r++) bk[rt][r] = sk[rt][r] = 0xffffffffu;
    // wavefront w expands k-step w of both tiles of the next pair
    i4v* xb = reinterpret_cast<i4v*>(mm_sm + MmLds::xb(nBt));   // [2][2][4][64]
    auto ldb = [&](int jj) -> uint2 {
        return jj < nB ? *reinterpret_cast<const uint2*>(Bp + (long long)jj * 32 + 8 * g) : make_uint2(0, 0);
    };
    {
        const uint2 b0 = ldb(c16), b1 = ldb(16 + c16);
        xb[(0 * 4 + w) * 64 + lane] = expand16(chunk16(b0, w)) * 2;
        xb[(1 * 4 + w) * 64 + lane] = expand16(chunk16(b1, w)) * 2;
    }
    uint2 bn0 = ldb(32 + c16), bn1 = ldb(48 + c16);
    __syncthreads();
    for (int c0 = 0; c0 < nB; c0 += MM_CHUNK) {
#pragma unroll
        for (int rt = 0; rt < MM_RT; rt++)
#pragma unroll
            for (int r = 0; r < 4; r++) lb[rt][r] = ls[rt][r] = 0xffffffffu;
        const int c1 = min(nB, c0 + MM_CHUNK);
        for (int j0 = c0; j0 < c1; j0 += 32) {
            const int cur = (j0 >> 5) & 1;
            if (j0 + 32 < nB) {   // block-uniform
                xb[(((cur ^ 1) * 2 + 0) * 4 + w) * 64 + lane] = expand16(chunk16(bn0, w)) * 2;   // bit -> 0 / 2
                xb[(((cur ^ 1) * 2 + 1) * 4 + w) * 64 + lane] = expand16(chunk16(bn1, w)) * 2;
                bn0 = ldb(j0 + 64 + c16);
                bn1 = ldb(j0 + 80 + c16);
            }
            const int t = (j0 - c0) >> 4;
            // a wavefront whose rows all lie past nA (the last workgroup of a frame is mostly
            // empty) only expands its share of the next pair
#pragma unroll
            for (int tt = 0; tt < 2; tt++) {
                if (!live) break;   // wavefront-uniform
                const int ci = s_pb[j0 + 16 * tt + c16] + t + tt;
                const i4v cinit = {ci, ci, ci, ci};
                i4v bf[4];
#pragma unroll
                for (int s2 = 0; s2 < 4; s2++) bf[s2] = xb[((cur * 2 + tt) * 4 + s2) * 64 + lane];
#pragma unroll
                for (int rt = 0; rt < MM_RT; rt++) {
                    i4v acc = cinit;
#pragma unroll
                    for (int s2 = 0; s2 < 4; s2++)
                        acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[rt][s2], bf[s2], acc, 0, 0, 0);
                    const int sv[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
                    for (int r = 0; r < 4; r++) top2_update(lb[rt][r], ls[rt][r], (uint32_t)sv[r]);
                }
            }
            __syncthreads();   // pair expanded into `cur ^ 1`; buffer `cur` free for the pair after
        }
        // the chunk's top-2 as global keys
        const uint32_t jb = (uint32_t)(c0 + c16);
#pragma unroll
        for (int rt = 0; rt < MM_RT; rt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                auto glob = [&](uint32_t k) {
                    return k == 0xffffffffu ? k : ((k >> 7) << 16) | (jb + 16 * (k & 127u));
                };
                top2_end_chunk<MULTI>(bk[rt][r], sk[rt][r], glob(lb[rt][r]), glob(ls[rt][r]));
            }
        if (!MULTI) break;
    }
    top2_write_rows<MM_RT>(bk, sk, row_base, MM_WROWS * w, s_pa, g, c16, nA, (long long)p * strideA,
                           nnratio, th_low, best_idx, best, second, match);
}

// The same top-2 on the FP4 path: wavefront w expands k-step (w & 1) of tile (w >> 1) of the next pair.
#ifndef FP_RT_DEF
#define FP_RT_DEF 3
#endif
constexpr int FP_RT = FP_RT_DEF;       // 16-row tiles per wavefront (89 VGPRs: 5 wavefronts per SIMD; 4 tiles: 114, 4)
constexpr int FP_WROWS = 16 * FP_RT;
constexpr int FP_ROWS = 4 * FP_WROWS;
typedef Top2Lds<FP_ROWS, 2> FpLds;

template <bool MULTI>
__global__ __launch_bounds__(256) void hamming_top2_fp4_kernel(
    const uint8_t* __restrict__ A, const int32_t* __restrict__ nA_arr, int nA_fixed, int strideA,
    const uint8_t* __restrict__ B, const int32_t* __restrict__ nB_arr, int nB_fixed, int strideB,
    const int32_t* __restrict__ pair_b, float nnratio, int th_low, int32_t* __restrict__ best_idx,
    int32_t* __restrict__ best, int32_t* __restrict__ second, int32_t* __restrict__ match) {
    extern __shared__ __attribute__((aligned(16))) int mm_sm[];   // FpLds
    int* s_pa = mm_sm + FpLds::pa;
    int* s_pb = mm_sm + FpLds::pb;
    const int p = blockIdx.y;
    const int q = pair_b ? pair_b[p] : p;
    const int nA = nA_arr ? nA_arr[p] : nA_fixed;
    const int nB = nB_arr ? nB_arr[q] : nB_fixed;
    const int row_base = blockIdx.x * FP_ROWS;
    if (row_base >= nA) return;   // block-uniform
    const uint8_t* Ap = A + (long long)p * strideA * 32;
    const uint8_t* Bp = B + (long long)q * strideB * 32;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, c16 = lane & 15, g = lane >> 4;
    const int nBt = (nB + 31) & ~31;   // whole pairs of 16-column tiles
    const bool live = __builtin_amdgcn_readfirstlane(row_base + FP_WROWS * w < nA ? 1 : 0) != 0;
    for (int j = tid; j < nBt; j += blockDim.x) s_pb[j] = 128 * ((j < nB ? popc_row(Bp + (long long)j * 32) : 256) + 256);
    {
        const int row = row_base + tid;
        if (tid < FP_ROWS) s_pa[tid] = row < nA ? popc_row(Ap + (long long)row * 32) : 0;
    }
    i4v af[FP_RT][2];
#pragma unroll
    for (int rt = 0; rt < FP_RT; rt++) {
        const int row = min(row_base + FP_WROWS * w + 16 * rt + c16, nA - 1);
        const uint2 v = *reinterpret_cast<const uint2*>(Ap + (long long)row * 32 + 8 * g);
        af[rt][0] = expand32_nib(v.x, FP4_NEG4);
        af[rt][1] = expand32_nib(v.y, FP4_NEG4);
    }
    __syncthreads();
    uint32_t bk[FP_RT][4], sk[FP_RT][4], lb[FP_RT][4], ls[FP_RT][4];
#pragma unroll
    for (int rt = 0; rt < FP_RT; rt++)
#pragma unroll
        for (int r = 0; r < 4; r++) bk[rt][r] = sk[rt][r] = 0xffffffffu;
    i4v* xb = reinterpret_cast<i4v*>(mm_sm + FpLds::xb(nBt));   // [2][2][2][64]
    const int xt = w >> 1, xs = w & 1;
    auto ldb = [&](int jj) -> uint32_t {
        return jj < nB ? *reinterpret_cast<const uint32_t*>(Bp + (long long)jj * 32 + 8 * g + 4 * xs) : 0u;
    };
    xb[((0 * 2 + xt) * 2 + xs) * 64 + lane] = expand32_nib(ldb(16 * xt + c16), FP4_ONE);
    uint32_t bn = ldb(32 + 16 * xt + c16);
    __syncthreads();
    for (int c0 = 0; c0 < nB; c0 += MM_CHUNK) {
#pragma unroll
        for (int rt = 0; rt < FP_RT; rt++)
#pragma unroll
            for (int r = 0; r < 4; r++) lb[rt][r] = ls[rt][r] = 0xffffffffu;
        const int c1 = min(nB, c0 + MM_CHUNK);
        for (int j0 = c0; j0 < c1; j0 += 32) {
            const int cur = (j0 >> 5) & 1;
            if (j0 + 32 < nB) {   // block-uniform
                xb[(((cur ^ 1) * 2 + xt) * 2 + xs) * 64 + lane] = expand32_nib(bn, FP4_ONE);
                bn = ldb(j0 + 64 + 16 * xt + c16);
            }
            const int t = (j0 - c0) >> 4;
#pragma unroll
            for (int tt = 0; tt < 2; tt++) {
                if (!live) break;   // wavefront-uniform
                const float ci = (float)(s_pb[j0 + 16 * tt + c16] + t + tt);
                const f4v cinit = {ci, ci, ci, ci};
                const i4v b0 = xb[((cur * 2 + tt) * 2 + 0) * 64 + lane];
                const i4v b1 = xb[((cur * 2 + tt) * 2 + 1) * 64 + lane];
#pragma unroll
                for (int rt = 0; rt < FP_RT; rt++) {
                    f4v acc = mfma_fp4(af[rt][0], b0, cinit);
                    acc = mfma_fp4(af[rt][1], b1, acc);
                    const float sv[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
                    for (int r = 0; r < 4; r++)   // keys >= 0: the bits order as the values
                        top2_update(lb[rt][r], ls[rt][r], __float_as_uint(sv[r]));
                }
            }
            __syncthreads();   // pair expanded into `cur ^ 1`; buffer `cur` free for the pair after
        }
        // the chunk's top-2 as global keys (chunk keys back to integers first)
        const uint32_t jb = (uint32_t)(c0 + c16);
#pragma unroll
        for (int rt = 0; rt < FP_RT; rt++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                auto glob = [&](uint32_t kb) {
                    if (kb == 0xffffffffu) return kb;
                    const uint32_t k = (uint32_t)__uint_as_float(kb);
                    return ((k >> 7) << 16) | (jb + 16 * (k & 127u));
                };
                top2_end_chunk<MULTI>(bk[rt][r], sk[rt][r], glob(lb[rt][r]), glob(ls[rt][r]));
            }
        if (!MULTI) break;
    }
    top2_write_rows<FP_RT>(bk, sk, row_base, FP_WROWS * w, s_pa, g, c16, nA, (long long)p * strideA,
                           nnratio, th_low, best_idx, best, second, match);
}

static int env_int(const char* name, int dflt) {   // read per launch: tests switch these
    const char* e = getenv(name);
    return e ? atoi(e) : dflt;
}
static int mm_fp4() { return env_int("ORBM_FP4", 1); }     // ORBM_FP4=0 selects the i8 kernel
static int tri_mm() { return env_int("ORBM_TRI_MM", 1); }   // 0: the per-lane scan for the all-pairs triangulation search
// kf2 column parts per query block of the matrix-core triangulation path
static int tri_split() { return std::max(1, std::min(8, env_int("ORBM_TRI_SPLIT", 1))); }

static void launch_top2(const uint8_t* A, const int32_t* nA_arr, int nA_fixed, int strideA, const uint8_t* B,
                        const int32_t* nB_arr, int nB_fixed, int strideB, const int32_t* pair_b, int n_pairs,
                        float nnratio, int th_low, int32_t* bi, int32_t* bd, int32_t* sd, int32_t* mt,
                        hipStream_t st) {
    const bool fp4 = mm_fp4() != 0;
    const int rows = fp4 ? FP_ROWS : MM_ROWS, nBt = (strideB + 31) & ~31;
    const size_t lds = fp4 ? FpLds::bytes(nBt) : MmLds::bytes(nBt);
    auto kern = fp4 ? (strideB <= MM_CHUNK ? hamming_top2_fp4_kernel<false> : hamming_top2_fp4_kernel<true>)
                    : (strideB <= MM_CHUNK ? hamming_top2_mfma_kernel<false> : hamming_top2_mfma_kernel<true>);
    hipLaunchKernelGGL(kern, dim3((unsigned)((strideA + rows - 1) / rows), (unsigned)n_pairs),
                       dim3(256), lds, st, A, nA_arr, nA_fixed, strideA, B, nB_arr, nB_fixed, strideB, pair_b,
                       nnratio, th_low, bi, bd, sd, mt);
}

}  // namespace orbamd
