// WorldToCamera in the reference's float expression, shared by the projection searches (orbp_*.h) and
// OptimizeSim3 (orbsim3.hip), which must put the same camera-frame point into the optimiser.
#pragma once

#include <hip/hip_runtime.h>

namespace orbamd {

// P = a pose, 12 floats: Rcw (row-major) then tcw.
// Rcw * Xw + tcw (cv::Matx: s = 0; s += a(i, k) * b(k) for k = 0..2)
__device__ __forceinline__ float3 pj_world_to_camera(const float* P, float X0, float X1, float X2) {
    return make_float3(((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[9], ((P[3] * X0 + P[4] * X1) + P[5] * X2) + P[10],
                       ((P[6] * X0 + P[7] * X1) + P[8] * X2) + P[11]);
}

}  // namespace orbamd
