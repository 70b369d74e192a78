// What every projection search shares (included by orbp.hip after orbp_layout.h): the constants, PjArgs, the Hamming
// distance and wave reductions, FeaturesGrid::AssignFeatures (pj_grid_kernel), GetFeaturesInArea's window
// and scan order, CheckOrientation's bin selection and the float sequences of the projection kernels.
//
// Reference: src/Frame.cc:71-145 (AssignFeatures / GetFeaturesInArea, Round / RoundUp / RoundDn at :32-34),
// src/ORBmatcher.cc:249-309 (CheckOrientation).
#pragma once

#include "world_to_camera.h"

namespace orbamd {

using orbamd_host::PJ_CELLS;
using orbamd_host::PJ_K;
constexpr int PJ_COLS = ORBM_GRID_COLS, PJ_ROWS = ORBM_GRID_ROWS;
constexpr int PJ_MAXKP = ORBM_PROJ_MAX_KP;
constexpr int PJ_IDX_BITS = 13;
static_assert((1 << PJ_IDX_BITS) == PJ_MAXKP, "sort key packs the keypoint index in 13 bits");
constexpr uint32_t PJ_IDX_MASK = (1u << PJ_IDX_BITS) - 1;
constexpr int PJ_TH_HIGH = 100;  // ORBmatcher.cc:41
constexpr int PJ_MAX_LEVELS = 32;
constexpr uint32_t PJ_NONE = 0xffffffffu;
constexpr int PJ_GW = 16;        // lanes of a group scanning one point's window (4 groups per wavefront)

struct PjArgs {
    int n_frames;
    const int32_t* kp_begin;
    const float* kp_xy;
    const int32_t* kp_oct;
    const float* kp_ur;
    const uint8_t* kp_desc;
    const uint8_t* kp_claimed;
    const float* bounds;
    const int32_t* mp_begin;
    const uint8_t* mp_valid;
    const float* mp_proj;
    const float* mp_vcos;
    const int32_t* mp_level;
    const uint8_t* mp_desc;
    const uint8_t* mp_has_obs;
    int n_levels;
    float scale[PJ_MAX_LEVELS];
    float th, nnratio;
    int total_mp;
    // workspace (PjGridLayout)
    int32_t* grid_idx;    // total_kp: frame-relative keypoint index at each sorted position
    int32_t* grid_start;  // n_frames x (PJ_CELLS + 1)
    int32_t* mp_cnt;      // total_mp
    int32_t* mp_frame;    // total_mp: frame of each map point (pj_grid_kernel)
    uint2* mp_top;        // total_mp x PJ_K: (key, index | level << 24)
    // outputs
    int32_t* kp_match;
    int32_t* n_matches;
};

__device__ __forceinline__ int pj_hamming(const uint8_t* a, const uint8_t* b) {
    const uint4* x = reinterpret_cast<const uint4*>(a);
    const uint4* y = reinterpret_cast<const uint4*>(b);
    const uint4 a0 = x[0], a1 = x[1], b0 = y[0], b1 = y[1];
    return __popc(a0.x ^ b0.x) + __popc(a0.y ^ b0.y) + __popc(a0.z ^ b0.z) + __popc(a0.w ^ b0.w) +
           __popc(a1.x ^ b1.x) + __popc(a1.y ^ b1.y) + __popc(a1.z ^ b1.z) + __popc(a1.w ^ b1.w);
}

// reductions over a group of W lanes (W = 64: the wavefront; W = 16: a quarter of it)
template <int W = 64>
__device__ __forceinline__ uint32_t pj_wave_min(uint32_t v) {
#pragma unroll
    for (int m = W / 2; m > 0; m >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m, W));
    return v;
}

template <int W = 64>
__device__ __forceinline__ int pj_wave_sum(int v) {
#pragma unroll
    for (int m = W / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, W);
    return v;
}

// ---------------------------------------------------------------- FeaturesGrid::AssignFeatures
__global__ __launch_bounds__(256) void pj_grid_kernel(PjArgs a) {
    __shared__ uint32_t keys[PJ_MAXKP];
    const int f = blockIdx.x;
    const int k0 = a.kp_begin[f], n = a.kp_begin[f + 1] - k0;
    int32_t* cs = a.grid_start + (size_t)f * (PJ_CELLS + 1);
    for (int j = a.mp_begin[f] + threadIdx.x; j < a.mp_begin[f + 1]; j += 256) a.mp_frame[j] = f;
    if (n > PJ_MAXKP) return;   // the search's walk kernel reports the frame
    const float* bd = a.bounds + 4 * (size_t)f;
    const float minx = bd[0], miny = bd[2];
    const float invW = PJ_COLS / (bd[1] - bd[0]);   // COLS / ImageBounds::Width() (Frame.cc:73)
    const float invH = PJ_ROWS / (bd[3] - bd[2]);
    int P = 1;
    while (P < n) P <<= 1;
    for (int i = threadIdx.x; i < P; i += 256) {
        uint32_t key = PJ_NONE;
        if (i < n) {
            const int cx = (int)roundf(invW * (a.kp_xy[2 * (size_t)(k0 + i)] - minx));   // Round (:32, :91)
            const int cy = (int)roundf(invH * (a.kp_xy[2 * (size_t)(k0 + i) + 1] - miny));
            if (cx >= 0 && cx < PJ_COLS && cy >= 0 && cy < PJ_ROWS)
                key = ((uint32_t)(cx * PJ_ROWS + cy) << PJ_IDX_BITS) | (uint32_t)i;
        }
        keys[i] = key;
    }
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)       // bitonic sort; keys are unique (index in the low bits)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < P; i += 256) {
                const int ixj = i ^ j;
                if (ixj > i) {
                    const uint32_t x = keys[i], y = keys[ixj];
                    if ((x > y) == ((i & k) == 0)) { keys[i] = y; keys[ixj] = x; }
                }
            }
            __syncthreads();
        }
    for (int p = threadIdx.x; p < n; p += 256)
        a.grid_idx[k0 + p] = keys[p] == PJ_NONE ? -1 : (int32_t)(keys[p] & PJ_IDX_MASK);
    for (int c = threadIdx.x; c <= PJ_CELLS; c += 256) {   // lower_bound(c << 13)
        const uint32_t want = (uint32_t)c << PJ_IDX_BITS;
        int lo = 0, hi = n;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (keys[mid] < want) lo = mid + 1; else hi = mid;
        }
        cs[c] = lo;
    }
}

static int launch_grid(const PjArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(pj_grid_kernel, dim3(a.n_frames), dim3(256), 0, st, a);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

// ---------------------------------------------------------------- GetFeaturesInArea
// The cells of the window (u +- r, v +- r) of a frame with image bounds bd = (minx, maxx, miny, maxy)
// (Frame.cc:109-119); !any: the window misses the grid.
struct PjWindow {
    int mincx, maxcx, mincy, maxcy;
    bool any;
};

struct PjBounds {   // a frame's grid origin and cells per pixel (Frame.cc:73-74)
    float minx, miny, invW, invH;
};

// (separate from pj_window so that a caller can issue the loads before it knows the radius)
__device__ __forceinline__ PjBounds pj_bounds(const float* bd) {
    return PjBounds{bd[0], bd[2], PJ_COLS / (bd[1] - bd[0]), PJ_ROWS / (bd[3] - bd[2])};
}

__device__ __forceinline__ PjWindow pj_window(const PjBounds& b, float u, float v, float r) {
    PjWindow w;
    const float minx = b.minx, miny = b.miny, invW = b.invW, invH = b.invH;
    w.mincx = max((int)floorf(invW * (u - r - minx)), 0);
    w.maxcx = min((int)ceilf(invW * (u + r - minx)), PJ_COLS - 1);
    w.mincy = max((int)floorf(invH * (v - r - miny)), 0);
    w.maxcy = min((int)ceilf(invH * (v + r - miny)), PJ_ROWS - 1);
    w.any = !(w.mincx >= PJ_COLS || w.maxcx < 0 || w.mincy >= PJ_ROWS || w.maxcy < 0);
    return w;
}

// The window's keypoints in GetFeaturesInArea's scan order, dealt to the W lanes of a group: calls
// fn(p, idx) for this lane's sorted positions p, idx = the frame-relative keypoint there.  cs = the
// frame's row of grid_start, k0 = the frame's first keypoint (the index into grid_idx stays a 32-bit sum).
// The caller's fn applies that search's gates (in the reference's order) and consumes the candidate.
template <int W, class Fn>
__device__ __forceinline__ void pj_scan_window(const PjWindow& w, const int32_t* cs, const int32_t* grid_idx, int k0,
                                               int lane, Fn&& fn) {
    if (!w.any) return;
    for (int cx = w.mincx; cx <= w.maxcx; cx++) {
        const int p0 = cs[cx * PJ_ROWS + w.mincy], p1 = cs[cx * PJ_ROWS + w.maxcy + 1];
        for (int p = p0 + lane; p < p1; p += W) fn(p, grid_idx[k0 + p]);
    }
}

// the strict box of GetFeaturesInArea (Frame.cc:134-137): a nan coordinate is outside
__device__ __forceinline__ bool pj_in_box(float kx, float ky, float u, float v, float r) {
    const float distx = kx - u;
    const float disty = ky - v;
    return fabsf(distx) < r && fabsf(disty) < r;
}

// ---------------------------------------------------------------- CheckOrientation
__device__ __forceinline__ int pjm_bin(float ang1, float ang2) {   // diffToBin(keypoint1.angle - keypoint2.angle)
    float diff = ang1 - ang2;
    if (diff < 0) diff += 360.f;
    int bin = __float2int_rn((1.f / 30) * diff);
    if (bin == 30) bin = 0;
    return min(max(bin, 0), 29);
}

// The bins CheckOrientation keeps (:283-303): the 30 bins sorted by size with libstdc++'s order (qt_sort),
// the largest and those of the next two not under 0.1 of it.  Returns their mask, *kept = their total.
__device__ __forceinline__ uint32_t pjm_keep_bins(const int* hist, int* kept) {
    QtItem it[30];
    for (int b = 0; b < 30; b++) it[b] = QtItem{hist[b], b};
    qt_sort(it, it + 30);
    const double max1 = it[0].size, max2 = it[1].size, max3 = it[2].size;
    const int eraseBin = max2 < 0.1 * max1 ? 1 : (max3 < 0.1 * max1 ? 2 : 3);
    uint32_t k = 0;
    int n = 0;
    for (int r = 0; r < eraseBin; r++) {
        k |= 1u << it[r].node;
        n += it[r].size;
    }
    *kept = n;
    return k;
}

// ---------------------------------------------------------------- projection pieces
// P = a pose, 12 floats: Rcw (row-major) then tcw.
// (pj_world_to_camera: world_to_camera.h)

// Ow = -Rcw^T * tcw (CameraPose::Invt)
__device__ __forceinline__ float3 pj_camera_centre(const float* P) {
    return make_float3(-((P[0] * P[9] + P[3] * P[10]) + P[6] * P[11]), -((P[1] * P[9] + P[4] * P[10]) + P[7] * P[11]),
                       -((P[2] * P[9] + P[5] * P[10]) + P[8] * P[11]));
}

// (float)cv::norm(p): the sum in double
__device__ __forceinline__ float pj_dist3d(float p0, float p1, float p2) {
    const double d0 = (double)p0, d1 = (double)p1, d2 = (double)p2;
    return (float)sqrt((d0 * d0 + d1 * d1) + d2 * d2);
}

// PredictScale(dist3D, ...) (MapPoint.cc:394-415): ceil(log(maxDistance / dist3D) / logScaleFactor), clamped
__device__ __forceinline__ int pj_predict_scale(float maxD, float dist3D, float log_sf, int n_levels) {
    const float ratio = maxD / dist3D;
    const int sc = (int)ceil(log((double)ratio) / (double)log_sf);
    return max(0, min(sc, n_levels - 1));
}

}  // namespace orbamd
