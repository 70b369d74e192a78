// cv::norm of a 3-vector of floats, shared by lm_newpoint.h and mm_normal.h: the squares are summed in double, ascending;
// the root stays double where the reference divides by it (Normalized) and is narrowed where it stores a float.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define N3_HD __host__ __device__ __forceinline__
#else
#define N3_HD inline
#endif

namespace orbamd {

// cv::norm(v)
N3_HD double norm3d(float x, float y, float z) { return sqrt(((double)x * x + (double)y * y) + (double)z * z); }

// (float)cv::norm(v)
N3_HD float lm_norm3(float x, float y, float z) { return (float)norm3d(x, y, z); }

}  // namespace orbamd
