// MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:341-380) for one point of a slot-table map, in the reference's float
// arithmetic and one fixed order.  Compiles for host and device (-ffp-contract=off, as the whole library): orbmm.hip
// (its host entry stages through common.h's Mirror, its buffers are mm_host.h's) runs it one lane per point,
// tests/native/map_maintenance_check.cpp on the CPU, tests/map_maintenance_ref.py restates
// it in numpy.
//   Ow            (-R^T) t as CameraPose::Invt: a cv::Matx product, s = 0, s += a(i, k) b(k), k ascending, in float.
//   Normalized    (1. / cv::norm(v)) v: the squares summed in double, ascending (norm3.h); 1. / norm in double; each
//                 component narrowed after the double product.
//   normal        summed in float from zeros, in the order of the point's CSR list; then (1. / n) * normal, the
//                 quotient in double, each component narrowed after the product.
//   dist          (float)cv::norm(Xw - Ow_ref); maxDistance = scaleFactor * dist; minDistance = maxDistance / back().
// A slot, an offset or an index outside its table is skipped; a point that then has nothing to use is left as it is.
#pragma once

#include <cstdint>

#include "norm3.h"

#ifndef MM_HD
#define MM_HD N3_HD
#endif

namespace orbamd {

constexpr int MM_MAX_LEVELS = 32;

struct MmPoints {
    int K, M, kf_cap, n_obs, n_levels;
    const uint8_t* mp_bad;
    const float* mp_xw;
    const int32_t* mp_ref_kf;
    const int32_t* mp_obs_off;
    const int32_t* mp_obs_kf;
    const int32_t* mp_obs_idx;
    const int32_t* kf_n;
    const int32_t* kf_kp_octave;
    const float* kf_ow;   // [K][3]: mm_center of every keyframe
    float* mp_normal;
    float* mp_max_min;
    float scale[MM_MAX_LEVELS];
};

// pose = Rcw row-major (9), tcw (3)
MM_HD void mm_center(const float* pose, float* Ow) {
    for (int i = 0; i < 3; i++) {
        float s = 0.f;
        for (int k = 0; k < 3; k++) s += (-pose[3 * k + i]) * pose[9 + k];
        Ow[i] = s;
    }
}

// The camera centre an observer contributes: center(k) points at three floats.  MmTableCenter is kf_ow's row.
struct MmTableCenter {
    const float* ow;
    MM_HD const float* operator()(int k) const { return ow + 3 * (size_t)k; }
};

// Returns true when the point's normal and distances were written.  The centre of every observer, and of the reference
// keyframe, is center(slot): lc_propagate.h selects between two tables per observer.
template <class Center>
MM_HD bool mm_update_point_at(const MmPoints& t, int p, const Center& center) {
    if (p < 0 || p >= t.M || t.mp_bad[p]) return false;
    const int ref = t.mp_ref_kf[p];
    if (ref < 0 || ref >= t.K) return false;
    int e0 = t.mp_obs_off[p], e1 = t.mp_obs_off[p + 1];
    if (e0 < 0) e0 = 0;
    if (e1 > t.n_obs) e1 = t.n_obs;
    const float X[3] = {t.mp_xw[3 * (size_t)p], t.mp_xw[3 * (size_t)p + 1], t.mp_xw[3 * (size_t)p + 2]};
    float sum[3] = {0.f, 0.f, 0.f};
    int n = 0, ref_idx = 0;   // observations[referenceKF] of a keyframe that is no key: 0
    bool ref_seen = false;
    for (int e = e0; e < e1; e++) {
        const int k = t.mp_obs_kf[e];
        if (k < 0 || k >= t.K) continue;
        const float* Ow = center(k);
        const float d[3] = {X[0] - Ow[0], X[1] - Ow[1], X[2] - Ow[2]};
        const double inv = 1. / norm3d(d[0], d[1], d[2]);
        for (int i = 0; i < 3; i++) sum[i] += (float)(inv * (double)d[i]);
        n++;
        if (k == ref && !ref_seen) {
            ref_seen = true;
            ref_idx = t.mp_obs_idx[e];
        }
    }
    if (n == 0) return false;
    int lim = t.kf_n[ref];
    if (lim > t.kf_cap) lim = t.kf_cap;
    if (ref_idx < 0 || ref_idx >= lim) return false;
    const int octave = t.kf_kp_octave[(size_t)ref * t.kf_cap + ref_idx];
    if (octave < 0 || octave >= t.n_levels) return false;
    const float* Or = center(ref);
    const float dist = lm_norm3(X[0] - Or[0], X[1] - Or[1], X[2] - Or[2]);
    const float max_distance = t.scale[octave] * dist;
    t.mp_max_min[2 * (size_t)p] = max_distance;
    t.mp_max_min[2 * (size_t)p + 1] = max_distance / t.scale[t.n_levels - 1];
    const double inv_n = 1. / n;
    for (int i = 0; i < 3; i++) t.mp_normal[3 * (size_t)p + i] = (float)((double)sum[i] * inv_n);
    return true;
}

MM_HD bool mm_update_point(const MmPoints& t, int p) { return mm_update_point_at(t, p, MmTableCenter{t.kf_ow}); }

}  // namespace orbamd
