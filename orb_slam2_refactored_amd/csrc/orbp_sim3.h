// ORBmatcher::SearchBySim3 (included by orbp.hip after orbp_grid.h and orbp_host.h, whose grid, window
// scan and packed minimum it builds on).
//
// Reference: src/ORBmatcher.cc:1090-1277 (LoopClosing::FindLoopInCandidateKFs, LoopClosing.cc:137, th 7.5).
// The map points of keyframe 1 are taken to camera 1, through S21 = S12.Inverse() to camera 2, projected
// with keyframe 2's intrinsics, gated (depth, image, invariance distance on |Xc2|; no viewing angle, no
// chi2), and matched to the first minimum-Hamming keypoint of levels [predictedScale - 1, predictedScale]
// inside the window th * scaleFactors[predictedScale] of keyframe 2's grid, accepted at bestDist <= TH_HIGH
// (:1127-1191).  The mirror image with S12 runs from keyframe 2 to keyframe 1 (:1194-1258), and a pair
// (i1, i2) survives when each picked the other (:1261-1274).
//   pj_grid_kernel       both keyframes' FeaturesGrid (one launch each; mp_begin = the other side's
//                        kp_begin gives every slot its pair)
//   sim3_project_kernel  one thread per keypoint slot, both directions in one launch: the two-stage
//                        transform and the gates in the reference's order and float expressions
//                        -> (valid, u, v, predictedScale)
//   sim3_best_kernel     a 16-lane group per slot: the window scan, the level gate and the group minimum
//                        of (dist << 13 | scan position) -> match1 / match2
//   sim3_agree_kernel    one thread per i1: match12[i1] = match1[i1] iff match2[match1[i1]] == i1, and
//                        the per-pair count n_found
//
// No ordered walk is needed.  Unlike SearchByProjection(KeyFrame, Scw, ...), nothing is claimed during
// either loop: match1 / match2 are written, never read, until the agreement pass, the skip tests read
// only matches12 as it was on entry (alreadyMatched1 / alreadyMatched2, :1108-1121), and no map point or
// keypoint is modified.  So every slot's bestIdx is independent of the iterations before it, and the
// agreement pass reads the finished arrays.  Preconditions (the caller's side of the contract), both
// evaluated on entry:
//   mp1_valid[i1] = mappoints1[i1] && !matches12[i1] && !mappoints1[i1]->isBad()        (:1130)
//   mp2_valid[i2] = mappoints2[i2] && !alreadyMatched2[i2] && !mappoints2[i2]->isBad()  (:1197)
// The caller then writes matches12[i1] = mappoints2[match12[i1]] where match12[i1] >= 0 (:1270).
#pragma once

namespace orbamd {

struct Sim3Side {   // one keyframe of every pair: its keypoints, its map point slots, its workspace
    const int32_t* kp_begin;
    const float* kp_xy;
    const int32_t* kp_oct;
    const uint8_t* kp_desc;
    const float* bounds;    // n_pairs x 4
    const float* pose;      // n_pairs x 12: Rcw (row-major) then tcw
    const float* camera;    // n_pairs x 4: fx, fy, cx, cy
    const uint8_t* valid;   // the caller's flag, one per keypoint slot
    const float* xw;
    const float* max_min;
    const uint8_t* mp_desc;
    int total;              // keypoint slots over all pairs
    // workspace
    int32_t* grid_idx;      // this keyframe's grid (pj_grid_kernel)
    int32_t* grid_start;    // n_pairs x (PJ_CELLS + 1)
    int32_t* pair;          // total: pair of each slot
    uint8_t* out_valid;     // sim3_project_kernel's results for this side's slots (searched in the other side)
    float* out_uv;          // total x 2
    int32_t* out_level;
    int32_t* match;         // match1 (side 0) / match2 (side 1): index in the other keyframe or -1
};

struct Sim3Args {
    int n_pairs;
    Sim3Side s[2];
    const float* s12;       // n_pairs x 13: R12 (row-major), t12, s
    int n_levels;
    float scale[PJ_MAX_LEVELS];
    float log_sf, th;
    int32_t* match12;
    int32_t* n_found;
};

// a pair either of whose keyframes is over the keypoint limit is reported, not searched
__device__ __forceinline__ bool sim3_over_limit(const Sim3Args& a, int f) {
    return a.s[0].kp_begin[f + 1] - a.s[0].kp_begin[f] > PJ_MAXKP || a.s[1].kp_begin[f + 1] - a.s[1].kp_begin[f] > PJ_MAXKP;
}

// the pair of slot i of a side, -1 for a slot outside every pair (rows past kp_begin[n_pairs]: pj_grid_kernel
// labelled none of them, so the label is checked against the offsets before it is used)
__device__ __forceinline__ int sim3_pair_of(const Sim3Args& a, const Sim3Side& s, int i) {
    const int f = s.pair[i];
    if ((unsigned)f >= (unsigned)a.n_pairs) return -1;
    return i >= s.kp_begin[f] && i < s.kp_begin[f + 1] ? f : -1;
}

__global__ __launch_bounds__(256) void sim3_project_kernel(Sim3Args a) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    for (int f = j; f < a.n_pairs; f += gridDim.x * 256)   // the count sim3_agree_kernel adds to
        a.n_found[f] = sim3_over_limit(a, f) ? -1 : 0;
    if (j >= a.s[0].total + a.s[1].total) return;
    const int d = j >= a.s[0].total ? 1 : 0;   // 0: keyframe 1 -> 2 (S21); 1: keyframe 2 -> 1 (S12)
    const int i = j - (d ? a.s[0].total : 0);
    const Sim3Side& src = a.s[d];
    const Sim3Side& dst = a.s[1 - d];
    const int f = sim3_pair_of(a, src, i);
    bool ok = f >= 0 && src.valid[i] != 0;
    float u = 0.f, v = 0.f;
    int ps = 0;
    if (ok) {
        const float* P = src.pose + 12 * (size_t)f;
        const float X0 = src.xw[3 * (size_t)i], X1 = src.xw[3 * (size_t)i + 1], X2 = src.xw[3 * (size_t)i + 2];
        const float3 c = pj_world_to_camera(P, X0, X1, X2);   // WorldToCamera
        const float c0 = c.x, c1 = c.y, c2 = c.z;
        const float* S = a.s12 + 13 * (size_t)f;
        float m[9], t0, t1, t2;   // Sim3::Map: (s * R) * x + t (Sim3.h:40), the matrix scaled elementwise first
        if (d == 0) {
            // S21 = S12.Inverse() (Sim3.h:43-47): R21 = R12^T, t21 = ((-(1 / s)) * R12^T) * t12, s21 = 1 / s
            const float inv_s = 1.f / S[12], neg = -inv_s;
            t0 = ((neg * S[0]) * S[9] + (neg * S[3]) * S[10]) + (neg * S[6]) * S[11];
            t1 = ((neg * S[1]) * S[9] + (neg * S[4]) * S[10]) + (neg * S[7]) * S[11];
            t2 = ((neg * S[2]) * S[9] + (neg * S[5]) * S[10]) + (neg * S[8]) * S[11];
#pragma unroll
            for (int r = 0; r < 3; r++)
#pragma unroll
                for (int c = 0; c < 3; c++) m[3 * r + c] = inv_s * S[3 * c + r];
        } else {
            t0 = S[9]; t1 = S[10]; t2 = S[11];
#pragma unroll
            for (int e = 0; e < 9; e++) m[e] = S[12] * S[e];
        }
        const float y0 = ((m[0] * c0 + m[1] * c1) + m[2] * c2) + t0;
        const float y1 = ((m[3] * c0 + m[4] * c1) + m[5] * c2) + t1;
        const float y2 = ((m[6] * c0 + m[7] * c1) + m[8] * c2) + t2;
        ok = !(y2 < 0.f);   // :1138 (z == 0 goes on: u, v are then inf or nan and fail Contains)
        if (ok) {
            const float* K = dst.camera + 4 * (size_t)f;
            const float invZ = 1.f / y2;   // CameraToImage with the other keyframe's intrinsics
            u = invZ * K[0] * y0 + K[2];
            v = invZ * K[1] * y1 + K[3];
            const float* bd = dst.bounds + 4 * (size_t)f;
            ok = u >= bd[0] && u < bd[1] && v >= bd[2] && v < bd[3];   // IsInImage (KeyFrame.cc:496-499)
        }
        if (ok) {
            const float dist3D = pj_dist3d(y0, y1, y2);   // cv::norm(Xc) of the mapped camera-frame point, :1151
            const float maxD = src.max_min[2 * (size_t)i], minD = src.max_min[2 * (size_t)i + 1];
            ok = !(dist3D < 0.8f * minD || dist3D > 1.2f * maxD);   // :1154, MapPoint.cc:382-392
            if (ok) ps = pj_predict_scale(maxD, dist3D, a.log_sf, a.n_levels);   // PredictScale(dist3D, keyframe)
        }
    }
    src.out_valid[i] = ok ? 1 : 0;
    src.out_uv[2 * (size_t)i] = u;
    src.out_uv[2 * (size_t)i + 1] = v;
    src.out_level[i] = ps;
}

// GetFeaturesInArea(u, v, th * scaleFactors[ps]) on the other keyframe's grid (no level filter in the grid
// call), then the loop of :1172-1185 / :1239-1252: the level window and the strict-< minimum.
__global__ __launch_bounds__(256) void sim3_best_kernel(Sim3Args a) {
    const int lane = threadIdx.x & (PJ_GW - 1);
    const int j = blockIdx.x * (256 / PJ_GW) + (threadIdx.x / PJ_GW);
    if (j >= a.s[0].total + a.s[1].total) return;   // group-uniform
    const int d = j >= a.s[0].total ? 1 : 0;
    const int i = j - (d ? a.s[0].total : 0);
    const Sim3Side& src = a.s[d];
    const Sim3Side& dst = a.s[1 - d];
    const int f = sim3_pair_of(a, src, i);
    const int k0 = f >= 0 ? dst.kp_begin[f] : 0;
    uint32_t best = PJ_NONE;
    if (f >= 0 && !sim3_over_limit(a, f) && src.out_valid[i]) {
        const int ps = src.out_level[i];
        const float u = src.out_uv[2 * (size_t)i], v = src.out_uv[2 * (size_t)i + 1];
        const float radius = a.th * a.scale[ps];
        const PjWindow w = pj_window(pj_bounds(dst.bounds + 4 * (size_t)f), u, v, radius);
        const uint8_t* d1 = src.mp_desc + 32 * (size_t)i;
        pj_scan_window<PJ_GW>(w, dst.grid_start + (size_t)f * (PJ_CELLS + 1), dst.grid_idx, k0, lane, [&](int p, int idx) {
            const int k = k0 + idx;
            if (!pj_in_box(dst.kp_xy[2 * (size_t)k], dst.kp_xy[2 * (size_t)k + 1], u, v, radius)) return;
            const int scale = dst.kp_oct[k];
            if (scale < ps - 1 || scale > ps) return;
            const int dist = pj_hamming(d1, dst.kp_desc + 32 * (size_t)k);
            best = min(best, ((uint32_t)dist << PJ_IDX_BITS) | (uint32_t)p);
        });
    }
    best = pj_wave_min<PJ_GW>(best);
    if (lane == 0) {
        int idx = -1;
        if (best != PJ_NONE && (int)(best >> PJ_IDX_BITS) <= PJ_TH_HIGH)   // :1187, TH_HIGH = 100
            idx = dst.grid_idx[k0 + (int)(best & PJ_IDX_MASK)];
        src.match[i] = idx;
    }
}

// :1261-1274: i1 and match1[i1] must have picked each other.
__global__ __launch_bounds__(256) void sim3_agree_kernel(Sim3Args a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.s[0].total) return;
    const int f = sim3_pair_of(a, a.s[0], i);
    const int idx2 = a.s[0].match[i];   // -1 for every slot of an over-limit pair, so match2 is read in range
    int out = -1;
    if (f >= 0 && idx2 >= 0 && a.s[1].match[a.s[1].kp_begin[f] + idx2] == i - a.s[0].kp_begin[f]) out = idx2;
    a.match12[i] = out;
    if (out >= 0) atomicAdd(&a.n_found[f], 1);
}

// The workspace: one Sim3SideLayout per side; match1 / match2 replace the sides' own match arrays when
// the caller asks for them.
static int sim3_workspace(PjScratch& sc, Sim3Args& a, int32_t* match1, int32_t* match2) {
    orbamd_host::Sim3SideLayout l[2];
    int rc;
    if ((rc = sc.workspace([&](Carver& c) {
            for (int d = 0; d < 2; d++) l[d].carve(c, a.n_pairs, a.s[d].total);
        })))
        return rc;
    for (int d = 0; d < 2; d++) {
        Sim3Side& s = a.s[d];
        s.grid_idx = l[d].grid_idx; s.grid_start = l[d].grid_start; s.pair = l[d].pair; s.out_level = l[d].out_level;
        s.match = l[d].match; s.out_valid = l[d].out_valid; s.out_uv = l[d].out_uv;
    }
    if (match1) a.s[0].match = match1;
    if (match2) a.s[1].match = match2;
    return ORB_OK;
}

static int launch_search_by_sim3(Sim3Args& a, hipStream_t st) {
    int rc;
    for (int d = 0; d < 2; d++) {   // side d's grid; its mp_frame pass labels the other side's slots
        PjArgs g;
        std::memset(&g, 0, sizeof(g));
        g.n_frames = a.n_pairs;
        g.kp_begin = a.s[d].kp_begin;
        g.kp_xy = a.s[d].kp_xy;
        g.bounds = a.s[d].bounds;
        g.grid_idx = a.s[d].grid_idx;
        g.grid_start = a.s[d].grid_start;
        g.mp_begin = a.s[1 - d].kp_begin;
        g.mp_frame = a.s[1 - d].pair;
        if ((rc = launch_grid(g, st))) return rc;
    }
    const int total = a.s[0].total + a.s[1].total;
    hipLaunchKernelGGL(sim3_project_kernel, dim3(std::max((total + 255) / 256, 1)), dim3(256), 0, st, a);
    ORB_HIP_TRY(hipGetLastError());
    if (total > 0) {
        hipLaunchKernelGGL(sim3_best_kernel, dim3((total + 256 / PJ_GW - 1) / (256 / PJ_GW)), dim3(256), 0, st, a);
        ORB_HIP_TRY(hipGetLastError());
    }
    if (a.s[0].total > 0) {
        hipLaunchKernelGGL(sim3_agree_kernel, dim3((a.s[0].total + 255) / 256), dim3(256), 0, st, a);
        ORB_HIP_TRY(hipGetLastError());
    }
    return ORB_OK;
}

// Argument checks and the host-side fields shared by both entries.
static int sim3_common(const orbm_sim3_batch* b, Sim3Args& a) {
    ORB_CHECK_ARG(b, "null argument");
    int rc;
    if ((rc = pj_check_sizes(b->n_pairs, b->total_kp1, b->total_kp2))) return rc;
    std::memset(&a, 0, sizeof(a));
    if ((rc = pj_set_pyramid(a, b->n_levels, b->scale_factors, b->th))) return rc;
    a.n_pairs = b->n_pairs;
    a.log_sf = b->log_scale_factor;
    if (b->n_pairs == 0) return ORB_OK;
    ORB_CHECK_ARG(b->kp1_begin && b->kp2_begin && b->bounds1 && b->bounds2 && b->pose1 && b->pose2 && b->camera1 &&
                      b->camera2 && b->s12,
                  "null array");
    ORB_CHECK_ARG(b->total_kp1 == 0 || (b->kp1_xy && b->kp1_octave && b->kp1_desc && b->mp1_valid && b->mp1_xw &&
                                        b->mp1_max_min && b->mp1_desc),
                  "null keyframe 1 array");
    ORB_CHECK_ARG(b->total_kp2 == 0 || (b->kp2_xy && b->kp2_octave && b->kp2_desc && b->mp2_valid && b->mp2_xw &&
                                        b->mp2_max_min && b->mp2_desc),
                  "null keyframe 2 array");
    a.s12 = b->s12;
    a.s[0] = Sim3Side{b->kp1_begin, b->kp1_xy, b->kp1_octave, b->kp1_desc, b->bounds1, b->pose1, b->camera1, b->mp1_valid,
                      b->mp1_xw, b->mp1_max_min, b->mp1_desc, b->total_kp1};
    a.s[1] = Sim3Side{b->kp2_begin, b->kp2_xy, b->kp2_octave, b->kp2_desc, b->bounds2, b->pose2, b->camera2, b->mp2_valid,
                      b->mp2_xw, b->mp2_max_min, b->mp2_desc, b->total_kp2};
    return ORB_OK;
}

// The arrays of a host batch (scale_factors stays host)
static void sim3_mirror(Mirror& io, orbm_sim3_batch& d) {
    const size_t F = d.n_pairs, K1 = d.total_kp1, K2 = d.total_kp2;
    io.add(d.kp1_begin, F + 1, true, false); io.add(d.kp2_begin, F + 1, true, false);
    io.add(d.kp1_xy, 2 * K1, true, false); io.add(d.kp1_octave, K1, true, false); io.add(d.kp1_desc, 32 * K1, true, false);
    io.add(d.kp2_xy, 2 * K2, true, false); io.add(d.kp2_octave, K2, true, false); io.add(d.kp2_desc, 32 * K2, true, false);
    io.add(d.bounds1, 4 * F, true, false); io.add(d.pose1, 12 * F, true, false); io.add(d.camera1, 4 * F, true, false);
    io.add(d.bounds2, 4 * F, true, false); io.add(d.pose2, 12 * F, true, false); io.add(d.camera2, 4 * F, true, false);
    io.add(d.mp1_valid, K1, true, false); io.add(d.mp1_xw, 3 * K1, true, false); io.add(d.mp1_max_min, 2 * K1, true, false);
    io.add(d.mp1_desc, 32 * K1, true, false);
    io.add(d.mp2_valid, K2, true, false); io.add(d.mp2_xw, 3 * K2, true, false); io.add(d.mp2_max_min, 2 * K2, true, false);
    io.add(d.mp2_desc, 32 * K2, true, false);
    io.add(d.s12, 13 * F, true, false);
}

}  // namespace orbamd
