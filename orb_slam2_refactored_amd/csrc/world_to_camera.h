// WorldToCamera in the reference's float expression, shared by the projection searches (orbp_*.h),
// OptimizeSim3 (orbsim3.hip), which must put the same camera-frame point into the optimiser, and Tracking's frame
// state (tf_frame.h), which a plain C++ compiler takes too.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PJ_HD __host__ __device__ __forceinline__
#else
#define PJ_HD inline
#endif

namespace orbamd {

// P = a pose, 12 floats: Rcw (row-major) then tcw.
// Rcw * Xw + tcw (cv::Matx: s = 0; s += a(i, k) * b(k) for k = 0..2)
PJ_HD void pj_world_to_camera3(const float* P, float X0, float X1, float X2, float* Xc) {
    Xc[0] = ((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[9];
    Xc[1] = ((P[3] * X0 + P[4] * X1) + P[5] * X2) + P[10];
    Xc[2] = ((P[6] * X0 + P[7] * X1) + P[8] * X2) + P[11];
}

#if defined(__HIPCC__)
__device__ __forceinline__ float3 pj_world_to_camera(const float* P, float X0, float X1, float X2) {
    float c[3];
    pj_world_to_camera3(P, X0, X1, X2, c);
    return make_float3(c[0], c[1], c[2]);
}
#endif

}  // namespace orbamd
