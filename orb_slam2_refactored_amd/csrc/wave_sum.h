// Cross-lane sums of fp64 values on one wavefront, VALU only (v_permlane32_swap / v_permlane16_swap and DPP
// moves, no LDS round trips): a reduce-scatter butterfly of 32 values, an all-reduce of one, and a
// v_readlane broadcast.  Every sum runs in a fixed order, so results are bit-reproducible.  Shared by
// PoseOptimization (orbpo.hip) and OptimizeSim3 (orbsim3.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace orbamd {

template <int CTRL>
__device__ __forceinline__ double po_dpp(double v) {
    return __builtin_amdgcn_update_dpp(0.0, v, CTRL, 0xf, 0xf, false);
}
constexpr int DPP_QUAD_XOR1 = 0xB1;   // quad_perm [1,0,3,2]
constexpr int DPP_QUAD_XOR2 = 0x4E;   // quad_perm [2,3,0,1]
constexpr int DPP_ROR4 = 0x124, DPP_ROR8 = 0x128, DPP_ROR12 = 0x12C;

union PoD2 { double d; int i[2]; };

// (a, b) -> (a', b'): lanes 32..63 of a swapped with lanes 0..31 of b (v_permlane32_swap), or odd
// rows of a with even rows of b (v_permlane16_swap) when ROW16.
template <bool ROW16>
__device__ __forceinline__ void po_swap(double& a, double& b) {
    PoD2 x{a}, y{b};
#pragma unroll
    for (int h = 0; h < 2; h++) {
        if constexpr (ROW16) {
            auto r = __builtin_amdgcn_permlane16_swap(x.i[h], y.i[h], false, false);
            x.i[h] = r[0]; y.i[h] = r[1];
        } else {
            auto r = __builtin_amdgcn_permlane32_swap(x.i[h], y.i[h], false, false);
            x.i[h] = r[0]; y.i[h] = r[1];
        }
    }
    a = x.d; b = y.d;
}

// Partner value across lane bit M (M = 4, 8 via DPP row rotates, 1, 2 via quad perms).
template <int M>
__device__ __forceinline__ double po_xor(double v, int lane) {
    if constexpr (M == 1) return po_dpp<DPP_QUAD_XOR1>(v);
    else if constexpr (M == 2) return po_dpp<DPP_QUAD_XOR2>(v);
    else if constexpr (M == 8) return po_dpp<DPP_ROR8>(v);
    else {
        static_assert(M == 4, "");
        // row_ror:N delivers lane (l - N) mod 16: l + 4 is ror 12, l - 4 is ror 4
        const double up = po_dpp<DPP_ROR12>(v), dn = po_dpp<DPP_ROR4>(v);
        return (lane & 4) ? dn : up;
    }
}

// One butterfly step over H value pairs: a lane keeps index i (bit clear) or i + H (bit set)
// and adds its partner's copy of it.
template <int H>
__device__ __forceinline__ void po_scatter_step(double (&v)[32], int lane) {
#pragma unroll
    for (int i = 0; i < H; i++) {
        if constexpr (H == 16) {          // across lane bit 5
            double a = v[i], b = v[i + H];
            po_swap<false>(a, b);
            v[i] = a + b;
        } else if constexpr (H == 8) {    // across lane bit 4
            double a = v[i], b = v[i + H];
            po_swap<true>(a, b);
            v[i] = a + b;
        } else {                          // across lane bit log2(2H): DPP
            const bool hi = (lane & (2 * H)) != 0;
            const double send = hi ? v[i] : v[i + H];
            const double keep = hi ? v[i + H] : v[i];
            v[i] = keep + po_xor<2 * H>(send, lane);
        }
    }
}

// Wavefront reduce-scatter of 32 doubles: on return lane l holds the wave total of value l >> 1.
__device__ __forceinline__ double po_wave_scatter32(double (&v)[32], int lane) {
    po_scatter_step<16>(v, lane);
    po_scatter_step<8>(v, lane);
    po_scatter_step<4>(v, lane);
    po_scatter_step<2>(v, lane);
    po_scatter_step<1>(v, lane);
    return v[0] + po_xor<1>(v[0], lane);
}

// Wavefront all-reduce of one double (every lane gets the same bits: each step adds the same two
// operands, a + b == b + a).
__device__ __forceinline__ double po_wave_sum(double v, int lane) {
    v += po_xor<1>(v, lane);
    v += po_xor<2>(v, lane);
    v += po_xor<4>(v, lane);
    v += po_xor<8>(v, lane);
    { double a = v, b = v; po_swap<true>(a, b); v = a + b; }
    { double a = v, b = v; po_swap<false>(a, b); v = a + b; }
    return v;
}

__device__ __forceinline__ double po_readlane(double v, int l) {
    PoD2 x{v};
    x.i[0] = __builtin_amdgcn_readlane(x.i[0], l);
    x.i[1] = __builtin_amdgcn_readlane(x.i[1], l);
    return x.d;
}

}  // namespace orbamd
