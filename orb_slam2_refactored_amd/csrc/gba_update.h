// The arithmetic of the map update behind a global bundle adjustment (LoopClosing.cc:392-446), host and device:
// the float CameraPose algebra (include/CameraPose.h:44-63) and the two per-element steps built from it.  A pose
// is 12 floats: Rcw row-major, then tcw.  cv::Matx products start at 0 and add the k = 0, 1, 2 terms in order;
// one rounding per operation (the library is built with -ffp-contract=off, and so is every test of this file).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define GBA_HD __host__ __device__ __forceinline__
#else
#define GBA_HD inline
#endif

namespace orbamd {

// R (3x3) * v (3x1)
GBA_HD void gba_mat_vec(const float* R, const float* v, float* o) {
    for (int i = 0; i < 3; i++) {
        float s = 0;
        for (int k = 0; k < 3; k++) s += R[3 * i + k] * v[k];
        o[i] = s;
    }
}

// CameraPose::Inverse: (R^T, -R^T * t), the negation applied to the matrix (CameraPose.h:44-45)
GBA_HD void gba_pose_inverse(const float* T, float* o) {
    float nRt[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            o[3 * i + j] = T[3 * j + i];
            nRt[3 * i + j] = -T[3 * j + i];
        }
    gba_mat_vec(nRt, T + 9, o + 9);
}

// CameraPose::operator*: t = R1 * t2 + t1, R = R1 * R2 (CameraPose.h:50-56).  o may not alias A or B.
GBA_HD void gba_pose_mul(const float* A, const float* B, float* o) {
    float Rt[3];
    gba_mat_vec(A, B + 9, Rt);
    for (int i = 0; i < 3; i++) o[9 + i] = Rt[i] + A[9 + i];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            float s = 0;
            for (int k = 0; k < 3; k++) s += A[3 * i + k] * B[3 * k + j];
            o[3 * i + j] = s;
        }
}

// A child the adjustment did not see (:402-403): TcwGBA = (Tchild * Tparent^-1) * parent.TcwGBA, both poses
// the ones before the update.
GBA_HD void gba_child_pose(const float* child_old, const float* parent_old, const float* parent_gba, float* o) {
    float Twc[12], Tchildc[12];
    gba_pose_inverse(parent_old, Twc);
    gba_pose_mul(child_old, Twc, Tchildc);
    gba_pose_mul(Tchildc, parent_gba, o);
}

// A point the adjustment did not see (:435-444): into the reference keyframe's camera before the update, back
// out through its pose after it.
GBA_HD void gba_move_point(const float* bef, const float* pose_new, const float* X, float* o) {
    float Xc[3], Twc[12], RX[3];
    gba_mat_vec(bef, X, RX);
    for (int i = 0; i < 3; i++) Xc[i] = RX[i] + bef[9 + i];
    gba_pose_inverse(pose_new, Twc);
    gba_mat_vec(Twc, Xc, RX);
    for (int i = 0; i < 3; i++) o[i] = RX[i] + Twc[9 + i];
}

}  // namespace orbamd
