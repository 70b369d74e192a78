// fr_undistort.h — the per-element arithmetic of building a Frame from extractor output (src/System.cc:153-219, orbfr.hip)
// for host and device (tests/native/frame_check.cpp compiles it with a plain C++ compiler).
//
//   fr_undistort      cv::undistortPoints(points, points, K, distCoeffs, cv::Mat(), K) on one CV_32FC2 point with a float K
//                     and 4 or 5 float coefficients, restated from recall [ext, recalled]: everything widened to double,
//                     x0 = (u - cx) * (1. / fx), exactly FR_ITERS = 5 fixed-point iterations, then K applied again as a
//                     3x3 product (the zeros of K take part: 0 * y is added) and one rounding to float per coordinate.
//                     Four coefficients are five with k3 = 0.  Five iterations are not converged (TUM1: the forward model
//                     of the result misses the input by up to 0.11 px); that is the reference's result.
//                     icdist < 0: newer OpenCV leaves the loop there with the undistorted first guess (x0, y0); this header
//                     does the same (parity unpinned: older OpenCV iterates on).
//   fr_keypoint_xy    UndistortKeyPoints' rule (:155): k1 == 0.f copies the point bit for bit
//   fr_image_bounds   ComputeImageBounds (:177-194): (0, cols, 0, rows) for k1 == 0.f, else the four undistorted corners
//                     paired as :189-192 pair them (std::min / std::max)
//   fr_depth_value    depth.convertTo(CV_32F, depthFactor) of one element: one float multiply [ext, recalled]
//   fr_rgbd           ComputeStereoFromRGBD (:197-219) for one keypoint: d > 0 on the bits of the float (a denormal depth is
//                     positive whatever the device's denormal mode; NaN, zeros and negatives are out, +inf is in)
//   fr_pixel          (int)pt.x, (int)pt.y of the distorted keypoint, or false when that is outside the image or a
//                     coordinate is NaN (a departure: the reference reads outside the depth map there)
// Every operation is done in the reference's type and order (-ffp-contract=off, as the whole library).
#pragma once

#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define FR_HD __host__ __device__ __forceinline__
#else
#define FR_HD inline
#endif

namespace orbamd {

constexpr int FR_ITERS = 5;

// cam: fx, fy, cx, cy (float).  dist: k1, k2, p1, p2, k3 (float).
FR_HD void fr_undistort(const float* cam, const float* dist, float u, float v, float* out, int iters = FR_ITERS) {
    const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
    const double k1 = dist[0], k2 = dist[1], p1 = dist[2], p2 = dist[3], k3 = dist[4];
    const double ifx = 1. / fx, ify = 1. / fy;
    const double x0 = ((double)u - cx) * ifx, y0 = ((double)v - cy) * ify;
    double x = x0, y = y0;
    for (int j = 0; j < iters; j++) {
        const double r2 = x * x + y * y;
        const double icdist = 1. / (1 + ((k3 * r2 + k2) * r2 + k1) * r2);
        if (icdist < 0) {
            x = x0;
            y = y0;
            break;
        }
        const double dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x);
        const double dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
    const double xx = fx * x + 0. * y + cx;
    const double yy = 0. * x + fy * y + cy;
    const double ww = 1. / (0. * x + 0. * y + 1);
    out[0] = (float)(xx * ww);
    out[1] = (float)(yy * ww);
}

FR_HD void fr_keypoint_xy(const float* cam, const float* dist, float u, float v, float* out) {
    if (dist[0] == 0.f) {
        out[0] = u;
        out[1] = v;
        return;
    }
    fr_undistort(cam, dist, u, v, out);
}

FR_HD float fr_min(float a, float b) { return b < a ? b : a; }   // std::min
FR_HD float fr_max(float a, float b) { return a < b ? b : a; }   // std::max

// bounds: minx, maxx, miny, maxy
FR_HD void fr_image_bounds(int rows, int cols, const float* cam, const float* dist, float* bounds) {
    const float h = (float)rows, w = (float)cols;
    if (dist[0] == 0.f) {
        bounds[0] = 0.f;
        bounds[1] = w;
        bounds[2] = 0.f;
        bounds[3] = h;
        return;
    }
    float c0[2], c1[2], c2[2], c3[2];
    fr_undistort(cam, dist, 0.f, 0.f, c0);
    fr_undistort(cam, dist, w, 0.f, c1);
    fr_undistort(cam, dist, 0.f, h, c2);
    fr_undistort(cam, dist, w, h, c3);
    bounds[0] = fr_min(c0[0], c2[0]);
    bounds[1] = fr_max(c1[0], c3[0]);
    bounds[2] = fr_min(c0[1], c1[1]);
    bounds[3] = fr_max(c2[1], c3[1]);
}

FR_HD bool fr_pixel(float x, float y, int rows, int cols, int& u, int& v) {
    if (!(x > -1.f && x < (float)cols && y > -1.f && y < (float)rows)) return false;   // NaN fails every comparison
    u = (int)x;
    v = (int)y;
    return true;
}

// is_u16: the element is a uint16, else a float
FR_HD float fr_depth_value(const void* element, bool is_u16, float depth_factor) {
    if (is_u16) {
        uint16_t raw;
        memcpy(&raw, element, 2);
        return (float)raw * depth_factor;
    }
    float raw;
    memcpy(&raw, element, 4);
    return raw * depth_factor;
}

FR_HD bool fr_depth_positive(float d) {
    uint32_t b;
    memcpy(&b, &d, 4);
    return b - 1u < 0x7f800000u;
}

FR_HD void fr_rgbd(float d, float x_un, float bf, float& uright, float& depth) {
    if (fr_depth_positive(d)) {
        depth = d;
        uright = x_un - bf / d;
    } else {
        depth = -1.f;
        uright = -1.f;
    }
}

}  // namespace orbamd
