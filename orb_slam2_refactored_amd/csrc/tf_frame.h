// tf_frame.h — the per-element arithmetic of Tracking's per-frame state (src/Tracking.cc, orbtf.hip) for host and device
// (tests/native/tracking_frame_check.cpp compiles it with a plain C++ compiler).
//
//   tf_pose_product   CameraPose::operator* (include/CameraPose.h:50-63): cv::Matx products, s = 0; s += a(i, k) * b(k, j)
//   tf_motion         tlc = lastFrame.pose.R() * currFrame.pose.Invt() + lastFrame.pose.t(); forward / backward
//                     (src/ORBmatcher.cc:1286-1288)
//   tf_project        the tests of src/ORBmatcher.cc:1301-1311 on one map point of the last frame
//   tf_unproject      CameraUnProjection::uvZToWorld (lm_newpoint.h), or Frame::UnprojectStereo's camera point
//                     (src/Frame.cc:221-238)
//   tf_depth_*        Z > 0, Z > thDepth and Z < thDepth on the bits of a float (a denormal depth is positive whatever
//                     the device's denormal mode), the sort key, and the prefix rule of src/Tracking.cc:703-742
// Every float operation is done in the reference's type and order (-ffp-contract=off, as the whole library).
#pragma once

#include <cstdint>
#include <cstring>

#include "lm_newpoint.h"
#include "world_to_camera.h"

#define TF_HD LM_HD

namespace orbamd {

constexpr int TF_MAX_LEVELS = 32;       // ORBTF_MAX_LEVELS
constexpr int TF_CLOSEST = 100;         // "npoints > 100" (:740, :783)

TF_HD bool tf_slot_ok(int p, int n) { return p >= 0 && p < n; }

TF_HD uint32_t tf_bits(float x) {
    uint32_t b;
    memcpy(&b, &x, 4);
    return b;
}

// cv::Matx product element: s = 0; s += a_k * b_k
TF_HD float tf_dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    float s = 0.f;
    s += a0 * b0;
    s += a1 * b1;
    s += a2 * b2;
    return s;
}

// C = A * B for poses of 12 floats (Rcw row-major, then tcw): t = A.R * B.t + A.t, then R = A.R * B.R
TF_HD void tf_pose_product(const float* A, const float* B, float* C) {
#pragma unroll
    for (int i = 0; i < 3; i++) C[9 + i] = tf_dot3(A[3 * i], A[3 * i + 1], A[3 * i + 2], B[9], B[10], B[11]) + A[9 + i];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = tf_dot3(A[3 * i], A[3 * i + 1], A[3 * i + 2], B[j], B[3 + j], B[6 + j]);
}

// 0, 1 = forward, 2 = backward.  L: the last frame's pose, Cp: the current one's.
TF_HD int tf_motion(const float* L, const float* Cp, float baseline, bool monocular) {
    float inv[3];   // Invt() = (-R^T) * t
#pragma unroll
    for (int i = 0; i < 3; i++) inv[i] = tf_dot3(-Cp[i], -Cp[3 + i], -Cp[6 + i], Cp[9], Cp[10], Cp[11]);
    const float z = tf_dot3(L[6], L[7], L[8], inv[0], inv[1], inv[2]) + L[11];
    const bool forward = z > baseline && !monocular, backward = -z > baseline && !monocular;
    return forward ? 1 : (backward ? 2 : 0);
}

struct TfProj {
    int valid;
    float u, v, ur;
};

// P: the current pose.  cam: fx, fy, cx, cy, bf.  bd: minx, maxx, miny, maxy.
TF_HD TfProj tf_project(const float* P, const float* cam, const float* bd, const float* Xw) {
    const TfProj none{0, 0.f, 0.f, 0.f};
    float c[3];
    pj_world_to_camera3(P, Xw[0], Xw[1], Xw[2], c);
    if (c[2] < 0.f) return none;   // :1302
    const float invZ = 1.f / c[2];   // CameraToImage
    const float u = invZ * cam[0] * c[0] + cam[2];
    const float v = invZ * cam[1] * c[1] + cam[3];
    const float ur = u - cam[4] / c[2];   // DepthToDisparity
    if (!(u >= bd[0] && u < bd[1] && v >= bd[2] && v < bd[3])) return none;   // Contains, :1310
    return TfProj{1, u, v, ur};
}

// The world point of keypoint (u, v) at depth Z in the frame of pose P (12 floats).  vo: Frame::UnprojectStereo's
// camera point ((u - cx) * Z * invfx) in place of uvZToCamera's (invfx * (u - cx) * Z).
TF_HD void tf_unproject(const float* P, const float* cam, float u, float v, float Z, bool vo, float* X) {
    const float T[12] = {P[0], P[1], P[2], P[9], P[3], P[4], P[5], P[10], P[6], P[7], P[8], P[11]};
    const float cam6[6] = {cam[0], cam[1], cam[2], cam[3], cam[4], 0.f};
    LmFrame f;
    lm_frame(T, cam6, f);
    if (vo)
        lm_camera_to_world(f, (u - f.cx) * Z * f.invfx, (v - f.cy) * Z * f.invfy, Z, X);
    else
        lm_uvz_to_world(f, u, v, Z, X);
}

// Z > 0: NaN, zeros and negatives are out; +inf and denormals are in
TF_HD bool tf_depth_valid(uint32_t zbits) { return zbits - 1u < 0x7f800000u; }
// Z > th for a valid Z
TF_HD bool tf_depth_far(uint32_t zbits, float th) {
    const uint32_t t = tf_bits(th);
    if ((t & 0x7fffffffu) > 0x7f800000u) return false;   // NaN
    if ((t >> 31) || t == 0u) return true;               // th <= 0 < Z
    return zbits > t;
}
// Z < th for a valid Z
TF_HD bool tf_depth_near(uint32_t zbits, float th) {
    const uint32_t t = tf_bits(th);
    if ((t & 0x7fffffffu) > 0x7f800000u || (t >> 31) || t == 0u) return false;
    return zbits < t;
}
// std::pair<float, int> order on (word, index): positive float bits are monotone as unsigned, and a keypoint's index is
// its position in the table.  by_index: keypoint order (StereoInitialization).  TF_WORD_NONE sorts behind every depth.
constexpr uint32_t TF_WORD_NONE = 0xffffffffu;
TF_HD uint32_t tf_depth_word(uint32_t zbits, bool by_index) {
    return !tf_depth_valid(zbits) ? TF_WORD_NONE : (by_index ? 0u : zbits);
}
TF_HD bool tf_depth_before(uint32_t wj, int j, uint32_t wi, int i) { return wj < wi || (wj == wi && j < i); }
// How many ranks the loop of :706-742 visits: it leaves after the first rank with Z > thDepth and rank + 1 > 100.
// n_close: the valid depths that are not far (they hold the ranks below it).
TF_HD int tf_n_processed(int n_valid, int n_close) {
    const int q = n_close > TF_CLOSEST ? n_close : TF_CLOSEST;
    return q < n_valid ? q + 1 : n_valid;
}

}  // namespace orbamd
