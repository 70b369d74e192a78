// The per-pair and per-match arithmetic of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:380-578):
// ComputeF12 (:55-71), the epipole of SearchForTriangulation (src/ORBmatcher.cc:772-773), one depth of
// ComputeSceneMedianDepth (src/KeyFrame.cc:544), the skip rule (:410-422), one match (:437-560) and what
// UpdateNormalAndDepth (src/MapPoint.cc:341-380) gives the new point.  Plain IEEE arithmetic that compiles for host
// and device (-ffp-contract=off, as the whole library): orblm.hip runs it per lane, tests/native/newpoints_check.cpp
// on the CPU, tests/newpoints_ref.py restates it in numpy.
//
// Everything is float arithmetic in one fixed order, so F12, ep2, the baseline and the depths are equal bit for bit
// wherever they are computed (the search gates on F12: one ulp there would change matches):
//   products      C = A B and y = A x are ((a0 b0 + a1 b1) + a2 b2), k ascending, zeros of K's inverse included; a
//                 translation is added last: (..) + t.
//   Rwc, Ow       Rwc = R^T; Ow = (-R^T) t (CameraPose::Invt).
//   K inverse     closed form: (1/fx, 0, (-cx)/fx; 0, 1/fy, (-cy)/fy; 0, 0, 1), every quotient one float division.
//   F12           R12 = R1w R2w^T; t12 = (-R12) t2w + t1w; F12 = ((K1^-T t12x) R12) K2^-1, left to right.
//   ep2           Xc = R2w Ow1 + t2w; invZ = 1 / Xc.z; u = (invZ fx) Xc.x + cx (CameraProjection::CameraToImage).
//   cv::norm      the squares are summed in double, ascending, the root is narrowed to float.
//   uvZToCamera   X = (invfx (u - cx)) Z with invfx = 1 / fx.
// The comparisons against 0.9998, 5.991 and 7.8 are made in double, as the reference's literals make them.
// cosf and atan2f (the stereo parallax) are the platform's: a decision within their rounding of its gate may differ
// between host, device and numpy.  Where OpenCV's SVD decides the reference's bits (the null vector of the 4 x 4 A),
// the rule of init_hyp.h stands: the eigenvector of the smallest diagonal entry of A^T A after INI_SWEEPS cyclic
// Jacobi sweeps in fp64, narrowed to float where the reference holds vt.
//
// Departure: a keyframe 2 without any MapPoint (n = 0) skips a monocular pair; the reference indexes an empty vector.
#pragma once

#include "init_hyp.h"
#include "norm3.h"

#define LM_HD INI_HD

namespace orbamd {

constexpr int LM_MAX_LEVELS = 32;   // ORBM_TRI_MAX_LEVELS

// statuses and branches: ORBLM_* of include/orbslam2_amd.h
enum LmStatus : int32_t {
    LM_CREATED = 0, LM_NO_MATCH = 1, LM_PAIR_SKIPPED = 2, LM_LOW_PARALLAX = 3, LM_W_ZERO = 4, LM_BEHIND1 = 5, LM_BEHIND2 = 6,
    LM_REPROJ1 = 7, LM_REPROJ2 = 8, LM_DIST_ZERO = 9, LM_SCALE = 10
};
enum LmBranch : int32_t { LM_BRANCH_NONE = 0, LM_BRANCH_TRIANGULATED = 1, LM_BRANCH_STEREO1 = 2, LM_BRANCH_STEREO2 = 3 };

// One keyframe: Tcw (3 x 4 row-major), Rwc, Ow, the camera.  32 floats.
struct LmFrame {
    float T[12], Rwc[9], Ow[3];
    float fx, fy, cx, cy, bf, b, invfx, invfy;
};
static_assert(sizeof(LmFrame) == 128, "");

struct LmTables {
    float scale1[LM_MAX_LEVELS], sigma1[LM_MAX_LEVELS], scale2[LM_MAX_LEVELS], sigma2[LM_MAX_LEVELS];
    int n_levels;
    float ratio_factor;   // 1.5f * keyframe1->pyramid.scaleFactor (:396)
};

struct LmPoint {
    int32_t status, branch;
    float xw[3], normal[3], min_distance, max_distance;
};

LM_HD float lm_dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// C = A B, 3 x 3 row-major float
LM_HD void lm_mul3(const float* A, const float* B, float* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = lm_dot3(A[3 * i], A[3 * i + 1], A[3 * i + 2], B[j], B[3 + j], B[6 + j]);
}

// lm_norm3, (float)cv::norm(v): norm3.h

// Tcw = 12 floats (3 x 4 row-major), cam = fx, fy, cx, cy, bf, baseline
LM_HD void lm_frame(const float* Tcw, const float* cam, LmFrame& f) {
#pragma unroll
    for (int i = 0; i < 12; i++) f.T[i] = Tcw[i];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) f.Rwc[3 * i + j] = Tcw[4 * j + i];
#pragma unroll
    for (int i = 0; i < 3; i++) f.Ow[i] = lm_dot3(-f.Rwc[3 * i], -f.Rwc[3 * i + 1], -f.Rwc[3 * i + 2], Tcw[3], Tcw[7], Tcw[11]);
    f.fx = cam[0]; f.fy = cam[1]; f.cx = cam[2]; f.cy = cam[3]; f.bf = cam[4]; f.b = cam[5];
    f.invfx = 1.f / cam[0];
    f.invfy = 1.f / cam[1];
}

// Rcw Xw + tcw (CameraProjection::WorldToCamera)
LM_HD void lm_world_to_camera(const LmFrame& f, const float* X, float* Xc) {
#pragma unroll
    for (int i = 0; i < 3; i++) Xc[i] = lm_dot3(f.T[4 * i], f.T[4 * i + 1], f.T[4 * i + 2], X[0], X[1], X[2]) + f.T[4 * i + 3];
}

LM_HD void lm_camera_to_image(const LmFrame& f, const float* Xc, float& u, float& v) {
    const float invZ = 1.f / Xc[2];
    u = invZ * f.fx * Xc[0] + f.cx;
    v = invZ * f.fy * Xc[1] + f.cy;
}

// Rwc (x, y, Z) + twc (CameraUnProjection::CameraToWorld)
LM_HD void lm_camera_to_world(const LmFrame& f, float x, float y, float Z, float* X) {
#pragma unroll
    for (int i = 0; i < 3; i++) X[i] = lm_dot3(f.Rwc[3 * i], f.Rwc[3 * i + 1], f.Rwc[3 * i + 2], x, y, Z) + f.Ow[i];
}

// CameraToWorld of uvZToCamera(u, v, Z) (CameraUnProjection::uvZToWorld)
LM_HD void lm_uvz_to_world(const LmFrame& f, float u, float v, float Z, float* X) {
    const float x = f.invfx * (u - f.cx) * Z, y = f.invfy * (v - f.cy) * Z;
    lm_camera_to_world(f, x, y, Z, X);
}

LM_HD void lm_kinv(const LmFrame& f, float* Ki) {
    Ki[0] = f.invfx; Ki[1] = 0.f; Ki[2] = (-f.cx) / f.fx;
    Ki[3] = 0.f; Ki[4] = f.invfy; Ki[5] = (-f.cy) / f.fy;
    Ki[6] = 0.f; Ki[7] = 0.f; Ki[8] = 1.f;
}

// ComputeF12, the epipole and the baseline of one pair
LM_HD void lm_pair(const LmFrame& f1, const LmFrame& f2, float* F12, float* ep2, float& baseline) {
    float R1[9], R2t[9], R12[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) R1[3 * i + j] = f1.T[4 * i + j];
#pragma unroll
    for (int i = 0; i < 9; i++) R2t[i] = f2.Rwc[i];
    lm_mul3(R1, R2t, R12);
    float t12[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
        t12[i] = lm_dot3(-R12[3 * i], -R12[3 * i + 1], -R12[3 * i + 2], f2.T[3], f2.T[7], f2.T[11]) + f1.T[4 * i + 3];
    const float tx[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};
    float K1i[9], K1it[9], K2i[9], a[9], b[9];
    lm_kinv(f1, K1i);
    lm_kinv(f2, K2i);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) K1it[3 * i + j] = K1i[3 * j + i];
    lm_mul3(K1it, tx, a);
    lm_mul3(a, R12, b);
    lm_mul3(b, K2i, F12);
    float Xc[3];
    lm_world_to_camera(f2, f1.Ow, Xc);
    lm_camera_to_image(f2, Xc, ep2[0], ep2[1]);
    baseline = lm_norm3(f2.Ow[0] - f1.Ow[0], f2.Ow[1] - f1.Ow[1], f2.Ow[2] - f1.Ow[2]);
}

// Z of one MapPoint of keyframe 2 (KeyFrame.cc:544)
LM_HD float lm_depth(const LmFrame& f2, const float* X) {
    return lm_dot3(f2.T[8], f2.T[9], f2.T[10], X[0], X[1], X[2]) + f2.T[11];
}

// :410-422; n = MapPoints of keyframe 2, median = depths[(n - 1) / 2] (monocular only)
LM_HD bool lm_skip(bool monocular, float baseline, const LmFrame& f2, int n, float median) {
    if (!monocular) return baseline < f2.b;
    if (n == 0) return true;
    return baseline / median < 0.01f;
}

// One match (:437-560) and UpdateNormalAndDepth of the created point.
LM_HD void lm_match(const LmFrame& f1, const LmFrame& f2, const LmTables& t, float u1, float v1, float ur1, float Z1, int o1,
                    float u2, float v2, float ur2, float Z2, int o2, LmPoint& r) {
    r.status = LM_LOW_PARALLAX;
    r.branch = LM_BRANCH_NONE;
#pragma unroll
    for (int i = 0; i < 3; i++) { r.xw[i] = 0.f; r.normal[i] = 0.f; }
    r.min_distance = 0.f;
    r.max_distance = 0.f;
    o1 = o1 < 0 ? 0 : (o1 >= t.n_levels ? t.n_levels - 1 : o1);
    o2 = o2 < 0 ? 0 : (o2 >= t.n_levels ? t.n_levels - 1 : o2);
    const bool stereo1 = ur1 >= 0, stereo2 = ur2 >= 0;
    const float xn1[2] = {f1.invfx * (u1 - f1.cx), f1.invfy * (v1 - f1.cy)};
    const float xn2[2] = {f2.invfx * (u2 - f2.cx), f2.invfy * (v2 - f2.cy)};
    float ray1[3], ray2[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        ray1[i] = lm_dot3(f1.Rwc[3 * i], f1.Rwc[3 * i + 1], f1.Rwc[3 * i + 2], xn1[0], xn1[1], 1.f);
        ray2[i] = lm_dot3(f2.Rwc[3 * i], f2.Rwc[3 * i + 1], f2.Rwc[3 * i + 2], xn2[0], xn2[1], 1.f);
    }
    const float dot = lm_dot3(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]);
    const double n1 = sqrt(((double)ray1[0] * ray1[0] + (double)ray1[1] * ray1[1]) + (double)ray1[2] * ray1[2]);
    const double n2 = sqrt(((double)ray2[0] * ray2[0] + (double)ray2[1] * ray2[1]) + (double)ray2[2] * ray2[2]);
    const float cosParallaxRays = (float)((double)dot / (n1 * n2));
    float cosParallaxStereo1 = cosParallaxRays + 1, cosParallaxStereo2 = cosParallaxRays + 1;
    if (stereo1)
        cosParallaxStereo1 = cosf(2.f * atan2f(0.5f * f1.b, Z1));
    else if (stereo2)
        cosParallaxStereo2 = cosf(2.f * atan2f(0.5f * f2.b, Z2));
    const float cosParallaxStereo = cosParallaxStereo1 < cosParallaxStereo2 ? cosParallaxStereo1 : cosParallaxStereo2;
    float X[3];
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (stereo1 || stereo2 || (double)cosParallaxRays < 0.9998)) {
        r.branch = LM_BRANCH_TRIANGULATED;
        double M[4][4], V[4][4], nv[4];
        ini_ata_zero(M);
        float row[4];
#pragma unroll
        for (int j = 0; j < 4; j++) row[j] = xn1[0] * f1.T[8 + j] - f1.T[j];
        ini_ata_add(M, row);
#pragma unroll
        for (int j = 0; j < 4; j++) row[j] = xn1[1] * f1.T[8 + j] - f1.T[4 + j];
        ini_ata_add(M, row);
#pragma unroll
        for (int j = 0; j < 4; j++) row[j] = xn2[0] * f2.T[8 + j] - f2.T[j];
        ini_ata_add(M, row);
#pragma unroll
        for (int j = 0; j < 4; j++) row[j] = xn2[1] * f2.T[8 + j] - f2.T[4 + j];
        ini_ata_add(M, row);
        ini_jacobi(M, V, INI_SWEEPS);
        ini_min_vector(M, V, nv);
        const float v[4] = {(float)nv[0], (float)nv[1], (float)nv[2], (float)nv[3]};
        if (v[3] == 0) { r.status = LM_W_ZERO; return; }
        const double denom = 1. / v[3];
#pragma unroll
        for (int i = 0; i < 3; i++) X[i] = (float)((double)v[i] * denom);
    } else if (stereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        r.branch = LM_BRANCH_STEREO1;
        lm_uvz_to_world(f1, u1, v1, Z1, X);
    } else if (stereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        r.branch = LM_BRANCH_STEREO2;
        lm_uvz_to_world(f2, u2, v2, Z2, X);
    } else {
        return;   // no stereo and very low parallax
    }
#pragma unroll
    for (int i = 0; i < 3; i++) r.xw[i] = X[i];
    float Xc1[3], Xc2[3];
    lm_world_to_camera(f1, X, Xc1);
    lm_world_to_camera(f2, X, Xc2);
    if (Xc1[2] <= 0) { r.status = LM_BEHIND1; return; }
    if (Xc2[2] <= 0) { r.status = LM_BEHIND2; return; }
    {
        float pu, pv;
        lm_camera_to_image(f1, Xc1, pu, pv);
        const float dx = pu - u1, dy = pv - v1;
        if (!stereo1) {
            if ((double)(dx * dx + dy * dy) > 5.991 * (double)t.sigma1[o1]) { r.status = LM_REPROJ1; return; }
        } else {
            const float dz = (pu - f1.bf / Xc1[2]) - ur1;
            if ((double)(dx * dx + dy * dy + dz * dz) > 7.8 * (double)t.sigma1[o1]) { r.status = LM_REPROJ1; return; }
        }
    }
    {
        float pu, pv;
        lm_camera_to_image(f2, Xc2, pu, pv);
        const float dx = pu - u2, dy = pv - v2;
        if (!stereo2) {
            if ((double)(dx * dx + dy * dy) > 5.991 * (double)t.sigma2[o2]) { r.status = LM_REPROJ2; return; }
        } else {
            const float dz = (pu - f2.bf / Xc2[2]) - ur2;
            if ((double)(dx * dx + dy * dy + dz * dz) > 7.8 * (double)t.sigma2[o2]) { r.status = LM_REPROJ2; return; }
        }
    }
    const float nA[3] = {X[0] - f1.Ow[0], X[1] - f1.Ow[1], X[2] - f1.Ow[2]};
    const float nB[3] = {X[0] - f2.Ow[0], X[1] - f2.Ow[1], X[2] - f2.Ow[2]};
    const double d1 = sqrt(((double)nA[0] * nA[0] + (double)nA[1] * nA[1]) + (double)nA[2] * nA[2]);
    const double d2 = sqrt(((double)nB[0] * nB[0] + (double)nB[1] * nB[1]) + (double)nB[2] * nB[2]);
    const float dist1 = (float)d1, dist2 = (float)d2;
    if (dist1 == 0 || dist2 == 0) { r.status = LM_DIST_ZERO; return; }
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = t.scale1[o1] / t.scale2[o2];
    if (ratioDist * t.ratio_factor < ratioOctave || ratioDist > ratioOctave * t.ratio_factor) { r.status = LM_SCALE; return; }
    r.status = LM_CREATED;
    // UpdateNormalAndDepth with the observations (keyframe 1, keyframe 2) and keyframe 1 as the reference keyframe:
    // normal = (1. / 2) (Normalized(Xw - Ow1) + Normalized(Xw - Ow2)), Normalized(v) = (1. / cv::norm(v)) v
    const double i1 = 1. / d1, i2 = 1. / d2;
#pragma unroll
    for (int i = 0; i < 3; i++) r.normal[i] = (float)((double)((float)(i1 * (double)nA[i]) + (float)(i2 * (double)nB[i])) * (1. / 2));
    r.max_distance = t.scale1[o1] * dist1;
    r.min_distance = r.max_distance / t.scale1[t.n_levels - 1];
}

}  // namespace orbamd
