// MapPoint::ComputeDistinctiveDescriptors, batched over map points (included by orbm.hip).
//
// Reference: src/MapPoint.cc:285-319.  Point p holds N descriptor rows [begin[p], begin[p + 1]) (the
// observations' descriptorsL rows from non-bad keyframes, in the reference's iteration order).  Row i's
// score is sorted(Hamming(row i, row j) for every j, the zero self-distance included)[(N - 1) / 2]; the
// winner is the strict-< minimum, so the lowest i of a tie.
//
// The median is found by rank, not by sorting: distances lie in 0..256, and the median is the smallest
// v with count(dist(i, j) <= v) >= (N - 1) / 2 + 1, located by bisection over v.  Three launches share
// one batch, each taking the points of its size class and leaving the others alone:
//   distinct_group_kernel<16>  N <= 16 (and the empty points): a 16-lane group per point, 16 points per
//                              workgroup.  The LocalMapping shape (N ~ 3-15) lives here; a wavefront per
//                              point would idle three quarters of the lanes or more.
//   distinct_group_kernel<64>  16 < N <= 64: one wavefront per point.
//                              In both, lane i holds row i in 8 VGPRs, row j is broadcast by lane read,
//                              and the row of distances stays in registers (a fully unrolled loop), so a
//                              bisection step is N compares.
//   distinct_block_kernel      64 < N <= ORBM_DISTINCT_MAX_OBS: a workgroup per point, the descriptors in
//                              LDS (32 KB at the cap), lanes striding over i, the bisection recomputing
//                              the distances from LDS (every lane reads the same row j: a broadcast).
//                              Also reports the points over the cap (best = best_median = -1, no row written).
// The winner is the group / workgroup minimum of (median << 10 | i).
#pragma once

namespace orbamd {

constexpr int DD_MAX = ORBM_DISTINCT_MAX_OBS;
constexpr int DD_IDX_BITS = 10;
static_assert((1 << DD_IDX_BITS) == DD_MAX, "the reduction key packs the row index in 10 bits");

struct DistinctArgs {
    const uint8_t* desc;    // total x 32
    const int32_t* begin;   // n_points + 1
    int n_points;
    int32_t* best;          // point-relative row, -1: empty or over the cap
    int32_t* best_median;   // or nullptr; -1 with best = -1
    uint8_t* out_desc;      // n_points x 32 or nullptr; written for non-empty points within the cap only
};

template <int W>
__device__ __forceinline__ uint32_t dd_group_min(uint32_t v) {
#pragma unroll
    for (int m = W / 2; m > 0; m >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m, W));
    return v;
}

// the smallest v in 0..256 with cnt(v) >= need, cnt non-decreasing and cnt(256) >= need
template <class Cnt>
__device__ __forceinline__ int dd_bisect(int need, Cnt cnt) {
    int lo = 0, hi = 256;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cnt(mid) >= need) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__device__ __forceinline__ void dd_none(const DistinctArgs& a, int p) {
    a.best[p] = -1;
    if (a.best_median) a.best_median[p] = -1;
}

__device__ __forceinline__ void dd_write(const DistinctArgs& a, int p, int k0, uint32_t key, int lane) {
    const int idx = (int)(key & (DD_MAX - 1));
    if (lane == 0) {
        a.best[p] = idx;
        if (a.best_median) a.best_median[p] = (int)(key >> DD_IDX_BITS);
    }
    if (a.out_desc && lane < 8)
        reinterpret_cast<uint32_t*>(a.out_desc + 32 * (size_t)p)[lane] =
            reinterpret_cast<const uint32_t*>(a.desc + 32 * (size_t)(k0 + idx))[lane];
}

template <int W>   // points with LO < N <= W, LO = 16 for the wavefront form and -1 (every N <= 16) for the 16-lane form
__global__ __launch_bounds__(256) void distinct_group_kernel(DistinctArgs a) {
    constexpr int LO = W == 16 ? -1 : 16;
    const int lane = threadIdx.x & (W - 1);
    const int p = blockIdx.x * (256 / W) + (threadIdx.x / W);
    int k0 = 0, n = -1;
    if (p < a.n_points) {
        k0 = a.begin[p];
        n = a.begin[p + 1] - k0;
    }
    const bool mine = n > LO && n <= W;   // group-uniform
    uint32_t r[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (mine && lane < n) {
        const uint4* x = reinterpret_cast<const uint4*>(a.desc + 32 * (size_t)(k0 + lane));
        const uint4 x0 = x[0], x1 = x[1];
        r[0] = x0.x; r[1] = x0.y; r[2] = x0.z; r[3] = x0.w;
        r[4] = x1.x; r[5] = x1.y; r[6] = x1.z; r[7] = x1.w;
    }
    // every lane of the wavefront takes part in the lane reads; the rows past n are never counted
    int d[W];
#pragma unroll
    for (int j = 0; j < W; j++) {
        int s = 0;
#pragma unroll
        for (int w = 0; w < 8; w++) s += __popc(r[w] ^ (uint32_t)__shfl((int)r[w], j, W));
        d[j] = s;
    }
    uint32_t key = 0xffffffffu;
    if (mine && lane < n) {
        const int med = dd_bisect((n - 1) / 2 + 1, [&](int v) {
            int c = 0;
#pragma unroll
            for (int j = 0; j < W; j++) c += (j < n && d[j] <= v) ? 1 : 0;
            return c;
        });
        key = ((uint32_t)med << DD_IDX_BITS) | (uint32_t)lane;
    }
    key = dd_group_min<W>(key);
    if (!mine) return;
    if (n == 0) {
        if (lane == 0) dd_none(a, p);   // an empty point: its descriptor stays as it is
        return;
    }
    dd_write(a, p, k0, key, lane);
}

__global__ __launch_bounds__(256) void distinct_block_kernel(DistinctArgs a) {
    __shared__ uint4 rows[DD_MAX * 2];
    __shared__ uint32_t wmin[4];
    const int p = blockIdx.x;
    const int k0 = a.begin[p], n = a.begin[p + 1] - k0;
    if (n <= 64) return;   // the group kernels' points (workgroup-uniform)
    if (n > DD_MAX) {
        if (threadIdx.x == 0) dd_none(a, p);
        return;
    }
    const uint4* src = reinterpret_cast<const uint4*>(a.desc + 32 * (size_t)k0);
    for (int t = threadIdx.x; t < 2 * n; t += 256) rows[t] = src[t];
    __syncthreads();
    const int need = (n - 1) / 2 + 1;
    uint32_t key = 0xffffffffu;
    for (int i = threadIdx.x; i < n; i += 256) {   // ascending i: the first minimum of a lane is its lowest row
        const uint4 a0 = rows[2 * i], a1 = rows[2 * i + 1];
        const int med = dd_bisect(need, [&](int v) {
            int c = 0;
            for (int j = 0; j < n; j++) {
                const uint4 b0 = rows[2 * j], b1 = rows[2 * j + 1];
                const int dist = __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
                                 __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
                c += dist <= v ? 1 : 0;
            }
            return c;
        });
        key = min(key, ((uint32_t)med << DD_IDX_BITS) | (uint32_t)i);
    }
    key = dd_group_min<64>(key);
    if ((threadIdx.x & 63) == 0) wmin[threadIdx.x >> 6] = key;
    __syncthreads();
    key = min(min(wmin[0], wmin[1]), min(wmin[2], wmin[3]));
    dd_write(a, p, k0, key, threadIdx.x);
}

static int launch_distinct(const DistinctArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(distinct_group_kernel<16>, dim3((a.n_points + 15) / 16), dim3(256), 0, st, a);
    ORB_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(distinct_group_kernel<64>, dim3((a.n_points + 3) / 4), dim3(256), 0, st, a);
    ORB_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(distinct_block_kernel, dim3(a.n_points), dim3(256), 0, st, a);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

}  // namespace orbamd
