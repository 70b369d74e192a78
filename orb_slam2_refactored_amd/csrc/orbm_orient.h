// orbm_orient.h — CheckOrientation on a query-indexed match list (included by orbm.hip).
//
// CheckOrientation (src/ORBmatcher.cc:249-309) on a query-indexed brute-force result, applied the
// way SearchForInitialization applies it (:676-686): matchIds = (bestIdx2, idx1) for every accepted
// query in ascending idx1, keypoints1 = frame B, keypoints2 = frame A, so a match's bin is
// diffToBin(angleB[j] - angleA[i]) and erasing sets match[i] = -1.  The histogram's 30 bins are
// sorted by size with libstdc++'s unstable std::sort (qt_sort.h reproduces its move sequence, so
// equal-size bins land where the reference puts them), then the bins from eraseBin on are erased.
// One workgroup per pair: counts into LDS, one lane sorts 30 items, then the erase pass.
#pragma once

namespace orbamd {

constexpr int HISTO_LENGTH = 30;

__device__ __forceinline__ int rot_bin(float angB, float angA) {
    float diff = angB - angA;
    if (diff < 0) diff += 360.f;
    int bin = __float2int_rn((1.f / HISTO_LENGTH) * diff);   // cvRound: round half to even
    if (bin == HISTO_LENGTH) bin = 0;
    return min(max(bin, 0), HISTO_LENGTH - 1);   // angles outside [0, 360) (the reference asserts)
}

__global__ __launch_bounds__(256) void check_orientation_kernel(
    const float* __restrict__ angA, int kstrideA, int capA, const int32_t* __restrict__ nA_arr,
    const float* __restrict__ angB, int kstrideB, int capB, const int32_t* __restrict__ pair_b,
    int32_t* __restrict__ match, int strideM, int32_t* __restrict__ nmatch, const int32_t* __restrict__ pair_a) {
    __shared__ int hist[HISTO_LENGTH];
    __shared__ uint32_t keep;
    const int p = blockIdx.x, q = pair_b ? pair_b[p] : p, tid = threadIdx.x;
    const int pa = pair_a ? pair_a[p] : p;   // A frame of pair p (SearchByBoW(KeyFrame, KeyFrame): kf1 slots)
    const int n = nA_arr[pa];
    const float* aA = angA + (long long)pa * capA * kstrideA;
    const float* aB = angB + (long long)q * capB * kstrideB;
    int32_t* m = match + (long long)p * strideM;
    if (tid < HISTO_LENGTH) hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += blockDim.x) {
        const int j = m[i];
        if (j >= 0) atomicAdd(&hist[rot_bin(aB[(long long)j * kstrideB], aA[(long long)i * kstrideA])], 1);
    }
    __syncthreads();
    if (tid == 0) {
        QtItem it[HISTO_LENGTH];
        for (int b = 0; b < HISTO_LENGTH; b++) it[b] = QtItem{hist[b], b};
        qt_sort(it, it + HISTO_LENGTH);
        const double max1 = it[0].size, max2 = it[1].size, max3 = it[2].size;
        const int eraseBin = max2 < 0.1 * max1 ? 1 : (max3 < 0.1 * max1 ? 2 : 3);
        uint32_t k = 0;
        int kept = 0;
        for (int r = 0; r < eraseBin; r++) {
            k |= 1u << it[r].node;
            kept += it[r].size;
        }
        keep = k;
        if (nmatch) nmatch[p] = kept;   // matchIds.size() - reduction
    }
    __syncthreads();
    const uint32_t k = keep;
    for (int i = tid; i < n; i += blockDim.x) {
        const int j = m[i];
        if (j >= 0 && !((k >> rot_bin(aB[(long long)j * kstrideB], aA[(long long)i * kstrideA])) & 1u)) m[i] = -1;
    }
}

}  // namespace orbamd
