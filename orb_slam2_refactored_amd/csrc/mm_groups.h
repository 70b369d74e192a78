// The lane groups the map-maintenance kernels (orbmm.hip, orbmm_observe.hip) hand to the rules of mm_connect.h,
// mm_cull.h and mm_observe.h, and the one-workgroup scan they share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace orbamd {

struct MmWave {
    int lane;
    static constexpr int width = 64;
    __device__ void sync() const { __syncthreads(); }   // one wavefront per workgroup: a wait and a fence
    __device__ int sum(int v) const {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v += __shfl_xor(v, s, 64);
        return v;
    }
    __device__ int min(int v) const {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v = ::min(v, __shfl_xor(v, s, 64));
        return v;
    }
    __device__ int max(int v) const {
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) v = ::max(v, __shfl_xor(v, s, 64));
        return v;
    }
    __device__ int prefix(bool flag, int& total) const {
        const unsigned long long b = __ballot(flag);
        total = __popcll(b);
        return __popcll(b & ((1ull << lane) - 1));
    }
};

constexpr int MM_CULL_WAVES = 4;

// One wavefront of a workgroup of several: its lanes run in lockstep, so sync() only has to order its memory operations.
struct MmSubWave : MmWave {
    __device__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
};

// The workgroup of MM_CULL_WAVES wavefronts; s: MM_CULL_WAVES ints of LDS.
struct MmBlock {
    int lane;
    int32_t* s;
    static constexpr int width = 64 * MM_CULL_WAVES;
    __device__ void sync() const { __syncthreads(); }
    template <class Op>
    __device__ int across(int v, Op op) const {   // v: this wavefront's value
        if ((lane & 63) == 0) s[lane >> 6] = v;
        __syncthreads();
        int r = s[0];
#pragma unroll
        for (int q = 1; q < MM_CULL_WAVES; q++) r = op(r, s[q]);
        __syncthreads();
        return r;
    }
    __device__ int sum(int v) const { return across(MmWave{lane & 63}.sum(v), [](int a, int b) { return a + b; }); }
    __device__ int min(int v) const { return across(MmWave{lane & 63}.min(v), [](int a, int b) { return ::min(a, b); }); }
    __device__ int max(int v) const { return across(MmWave{lane & 63}.max(v), [](int a, int b) { return ::max(a, b); }); }
    __device__ int prefix(bool flag, int& total) const {
        int mine;
        const int off = MmWave{lane & 63}.prefix(flag, mine);
        if ((lane & 63) == 0) s[lane >> 6] = mine;
        __syncthreads();
        int before = 0;
        total = 0;
#pragma unroll
        for (int q = 0; q < MM_CULL_WAVES; q++) {
            before += q < (lane >> 6) ? s[q] : 0;
            total += s[q];
        }
        __syncthreads();
        return before + off;
    }
};

// Exclusive scan of count[0 .. n), each entry clamped to [lo, hi] and add added, by one workgroup of 256, summed in T; in
// place allowed (every entry is read and written by one thread); off[n] = the total, which every thread returns.  With
// T = long long an offset past top is stored as top (the 32-bit sums are stored as they are).
template <class T>
__device__ T mm_block_scan(const int32_t* count, int n, int32_t* off, int lo, int hi, int add, T top = 0) {
    __shared__ T s_wave[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto stored = [&](T v) {
        if constexpr (sizeof(T) > sizeof(int32_t)) return (int32_t)::min(v, top);
        else return v;
    };
    T carry = 0;
    for (int base = 0; base < n; base += 256) {   // uniform trip count
        const int i = base + (int)threadIdx.x;
        const T v = i < n ? ::min(::max(count[i], lo), hi) + add : 0;
        T x = v;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const T y = __shfl_up(x, d, 64);
            if (lane >= d) x += y;
        }
        if (lane == 63) s_wave[wave] = x;
        __syncthreads();
        T before = 0;
        for (int q = 0; q < wave; q++) before += s_wave[q];
        const T total = (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        if (i < n) off[i] = stored(carry + before + x - v);
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) off[n] = stored(carry);
    return carry;
}

}  // namespace orbamd
