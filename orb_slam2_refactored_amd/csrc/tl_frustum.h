// tl_frustum.h — IsInFrustum's per-point arithmetic (src/Tracking.cc:554-605) for host and device (orbtl.hip,
// tests/native/local_map_check.cpp).
//
// Every float and double operation is done in the reference's type and order; the library is built with
// -ffp-contract=off, so none of them fuses.  The expressions are those of pj_world_to_camera, pj_camera_centre,
// pj_dist3d and pj_predict_scale (world_to_camera.h, orbp_grid.h) and of reloc_project_kernel's
// ImageBounds::Contains (orbp_motion.h), restated here without HIP types so that a plain C++ compiler takes them.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define TL_HD __host__ __device__ __forceinline__
#else
#define TL_HD inline
#endif

namespace orbamd {

// The test a point left IsInFrustum at (TL_PASS: it returned true).
enum TlFail : int { TL_PASS = 0, TL_DEPTH = 1, TL_BOUNDS = 2, TL_DISTANCE = 3, TL_VIEW_COS = 4 };

struct TlPoint {
    int fail;             // TlFail
    float u, v, ur;       // trackProjX, trackProjY, trackProjXR
    float view_cos;       // trackViewCos
    int level;            // trackScaleLevel
    double scale_exact;   // log(maxDistance / dist) / logScaleFactor before ceil (the tests keep it off the integers)
};

// P: Rcw row-major then tcw (12).  cam: fx, fy, cx, cy, bf.  bd: minx, maxx, miny, maxy.  maxD / minD: the map
// point's raw maxDistance_ / minDistance_ (Get*DistanceInvariance apply 1.2f / 0.8f, MapPoint.cc).
TL_HD TlPoint tl_frustum(const float* P, const float* cam, const float* bd, const float* Xw, const float* Pn, float maxD,
                         float minD, float min_view_cos, float log_sf, int n_levels) {
    TlPoint r{TL_PASS, 0.f, 0.f, 0.f, 0.f, 0, 0.0};
    // Rcw * Xw + tcw (cv::Matx: s = 0; s += a(i, k) * b(k))
    const float x = ((P[0] * Xw[0] + P[1] * Xw[1]) + P[2] * Xw[2]) + P[9];
    const float y = ((P[3] * Xw[0] + P[4] * Xw[1]) + P[5] * Xw[2]) + P[10];
    const float z = ((P[6] * Xw[0] + P[7] * Xw[1]) + P[8] * Xw[2]) + P[11];
    if (z < 0.f) { r.fail = TL_DEPTH; return r; }   // :567
    const float invZ = 1.f / z;                       // CameraToImage
    const float u = invZ * cam[0] * x + cam[2];
    const float v = invZ * cam[1] * y + cam[3];
    if (!(u >= bd[0] && u < bd[1] && v >= bd[2] && v < bd[3])) { r.fail = TL_BOUNDS; return r; }   // Contains, :573
    // Ow = -Rcw^T * tcw (CameraPose::Invt), PO = Xw - Ow
    const float o0 = -((P[0] * P[9] + P[3] * P[10]) + P[6] * P[11]);
    const float o1 = -((P[1] * P[9] + P[4] * P[10]) + P[7] * P[11]);
    const float o2 = -((P[2] * P[9] + P[5] * P[10]) + P[8] * P[11]);
    const float p0 = Xw[0] - o0, p1 = Xw[1] - o1, p2 = Xw[2] - o2;
    const double d0 = (double)p0, d1 = (double)p1, d2 = (double)p2;
    const float dist = (float)sqrt((d0 * d0 + d1 * d1) + d2 * d2);   // (float)cv::norm(PO)
    if (dist < 0.8f * minD || dist > 1.2f * maxD) { r.fail = TL_DISTANCE; return r; }   // :582
    float s = 0.f;   // Matx::dot
    s += p0 * Pn[0];
    s += p1 * Pn[1];
    s += p2 * Pn[2];
    const float view_cos = s / dist;
    if (view_cos < min_view_cos) { r.fail = TL_VIEW_COS; return r; }   // :590
    // PredictScale (MapPoint.cc:394-415)
    const float ratio = maxD / dist;
    r.scale_exact = log((double)ratio) / (double)log_sf;
    const int sc = (int)ceil(r.scale_exact);
    r.level = sc < 0 ? 0 : (sc > n_levels - 1 ? n_levels - 1 : sc);
    r.u = u;
    r.v = v;
    r.ur = u - cam[4] / z;   // pt.x - DepthToDisparity(Xc(2))
    r.view_cos = view_cos;
    return r;
}

}  // namespace orbamd
