// SearchByProjection(Frame&, const Frame&, th, mono) and SearchByProjection(Frame&, KeyFrame*,
// alreadyFound, th, ORBdist) (included by orbp.hip after orbp_grid.h and orbp_host.h).
//
// Reference: src/ORBmatcher.cc:1279-1362 (TrackWithMotionModel) and :1364-1445 (Tracking::Relocalization).
//
// The motion-model search has the grid (pj_grid_kernel) and the claim rule of orbp_track.h (a keypoint
// whose current map point has observations is skipped, :1331-1333), but only the best distance counts
// (no ratio), so one wavefront per frame walks the last frame's points in idx1 order: each point's window
// is scanned by the lanes against the LDS claim bitmap and the wave minimum of (dist << 13 | scan
// position) is the reference's first-best.  The accepted pair of every point is kept (choice) for
// CheckOrientation, which counts overwritten pairs too (matchIds).
//   pjm_score_kernel   a 16-lane group per point: its best key against the entry claims
//   pjm_walk_kernel    one wavefront per frame: the ordered claim walk, rescanning where a claim interferes
//   pjm_orient_kernel  CheckOrientation over the accepted pairs
// launch_motion_walk runs the three; the relocalisation search (reloc_project_kernel in front) and the
// Sim3 projection search (orbp_fuse.h) feed it their own projections.
#pragma once

namespace orbamd {

struct PjmExtra {
    const int32_t* motion;
    const float* kp_angle;
    const float* mp_angle;
    int32_t* choice;   // total_mp: accepted idx2 or -1
    int max_dist;      // TH_HIGH (:1347); ORBdist for SearchByProjection(Frame&, KeyFrame*, ...) (:1425)
    int lvl_up;        // upper end of the level window when motion == 0: [octave - 1, octave + lvl_up].
                       // 1 for the motion and relocalisation entries, 0 for the Sim3 search (:592)
};

// The window scan of one last-frame point (GetFeaturesInArea + the gates of :1329-1339): each lane's
// smallest (dist << 13 | scan position), against the claim bitmap when `bits` is given.
template <int W>
__device__ __forceinline__ uint32_t pjm_scan(const PjArgs& a, const PjmExtra& e, int f, int j, const uint32_t* bits,
                                             int lane) {
    const int k0 = a.kp_begin[f];
    const int mot = e.motion ? e.motion[f] : 0;
    const PjBounds bd = pj_bounds(a.bounds + 4 * (size_t)f);   // the loads go out before the level is known
    const int32_t* cs = a.grid_start + (size_t)f * (PJ_CELLS + 1);
    const int oct = a.mp_level[j];
    uint32_t best = PJ_NONE;
    if (oct < 0 || oct >= a.n_levels) return best;   // no level to project at: no candidate
    const float r = a.th * a.scale[oct];   // :1316
    // :1318-1319 through GetFeaturesInArea's checkLevels (maxLevel < 0 -> nlevels)
    const int lo = mot == 1 ? oct : (mot == 2 ? 0 : oct - 1);
    const int hi = mot == 1 ? a.n_levels : (mot == 2 ? oct : oct + e.lvl_up);
    const float u = a.mp_proj[3 * (size_t)j], v = a.mp_proj[3 * (size_t)j + 1];
    const float uR = a.kp_ur ? a.mp_proj[3 * (size_t)j + 2] : 0.f;
    const PjWindow w = pj_window(bd, u, v, r);
    if (!w.any) return best;
    const uint8_t* d1 = a.mp_desc + 32 * (size_t)j;
    // Written out, not through pj_scan_window: in pjm_walk_kernel's rescan the point is wave-uniform, and
    // through the primitive the compiler keeps the column bounds in vector registers, which costs the
    // one-wavefront walk about 1 %.  Only the window comes from the shared code.
    for (int cx = w.mincx; cx <= w.maxcx; cx++) {
        const int p0 = cs[cx * PJ_ROWS + w.mincy], p1 = cs[cx * PJ_ROWS + w.maxcy + 1];
        for (int p = p0 + lane; p < p1; p += W) {
            const int idx = a.grid_idx[k0 + p];
            const int k = k0 + idx;
            const int level = a.kp_oct[k];
            if (level < lo || level > hi) continue;
            if (!pj_in_box(a.kp_xy[2 * (size_t)k], a.kp_xy[2 * (size_t)k + 1], u, v, r)) continue;
            if (a.kp_claimed && a.kp_claimed[k]) continue;
            if (bits && ((bits[idx >> 5] >> (idx & 31)) & 1u)) continue;
            if (a.kp_ur) {   // the stereo gate of :1335 (the relocalisation search has none)
                const float ur = a.kp_ur[k];
                if (ur > 0 && fabsf(uR - ur) > r) continue;
            }
            const int dist = pj_hamming(d1, a.kp_desc + 32 * (size_t)k);
            best = min(best, ((uint32_t)dist << PJ_IDX_BITS) | (uint32_t)p);
        }
    }
    return best;
}

// Data-parallel first pass: every point's best key against the entry claims only (a 16-lane group
// per point).  Claims made during the call only remove candidates, so the walk keeps this key
// whenever its keypoint is still unclaimed and rescans otherwise.
__global__ __launch_bounds__(256) void pjm_score_kernel(PjArgs a, PjmExtra e) {
    const int j = blockIdx.x * (256 / PJ_GW) + (threadIdx.x / PJ_GW), lane = threadIdx.x % PJ_GW;
    if (j >= a.total_mp) return;
    const int f = a.mp_frame[j];
    uint32_t best = PJ_NONE;
    if (a.kp_begin[f + 1] - a.kp_begin[f] <= PJ_MAXKP && a.mp_valid[j]) best = pjm_scan<PJ_GW>(a, e, f, j, nullptr, lane);
    best = pj_wave_min<PJ_GW>(best);
    if (lane == 0) a.mp_cnt[j] = (int32_t)best;
}

// The ordered walk: 64 points per chunk with their first-pass keys in registers; a point whose key's
// keypoint was claimed earlier in the call (an earlier point with observations took it) rescans its
// window against the LDS claim bitmap.
__global__ __launch_bounds__(64) void pjm_walk_kernel(PjArgs a, PjmExtra e) {
    __shared__ uint32_t bits[PJ_MAXKP / 32];
    const int f = blockIdx.x, lane = threadIdx.x;
    const int k0 = a.kp_begin[f], n = a.kp_begin[f + 1] - k0;
    const int m0 = a.mp_begin[f], m1 = a.mp_begin[f + 1];
    for (int i = lane; i < n; i += 64) a.kp_match[k0 + i] = -1;   // also for an over-limit frame
    if (n > PJ_MAXKP) {
        for (int j = m0 + lane; j < m1; j += 64) e.choice[j] = -1;
        if (lane == 0) a.n_matches[f] = -1;
        return;
    }
    for (int i = lane; i < PJ_MAXKP / 32; i += 64) bits[i] = 0;
    __syncthreads();
    int nm = 0;
    for (int c = m0; c < m1; c += 64) {
        const int j = c + lane;
        uint32_t key = PJ_NONE;
        int idx = -1, obs = 0;
        if (j < m1) {
            key = (uint32_t)a.mp_cnt[j];
            obs = a.mp_has_obs ? a.mp_has_obs[j] : 1;   // NULL: every accepted point claims (relocalisation)
            if (key != PJ_NONE) idx = a.grid_idx[k0 + (int)(key & PJ_IDX_MASK)];
        }
        int mych = -1;
        const int cnt = min(64, m1 - c);
        for (int i = 0; i < cnt; i++) {
            uint32_t K = (uint32_t)__shfl((int)key, i, 64);
            if (K == PJ_NONE || (int)(K >> PJ_IDX_BITS) > e.max_dist) continue;   // :1347 (a rescan only loses candidates)
            int ch = __shfl(idx, i, 64);
            if ((bits[ch >> 5] >> (ch & 31)) & 1u) {   // taken earlier in this call: rescan
                K = pj_wave_min(pjm_scan<64>(a, e, f, c + i, bits, lane));
                if (K == PJ_NONE || (int)(K >> PJ_IDX_BITS) > e.max_dist) continue;
                ch = a.grid_idx[k0 + (int)(K & PJ_IDX_MASK)];
            }
            const int ob = __shfl(obs, i, 64);   // every lane takes part in the shuffle
            if (lane == 0) {
                a.kp_match[k0 + ch] = c + i - m0;
                if (ob) bits[ch >> 5] |= 1u << (ch & 31);
            }
            if (lane == i) mych = ch;
            nm++;
            __syncthreads();   // one wavefront: the claim bit before the next point
        }
        if (j < m1) e.choice[j] = mych;
    }
    if (lane == 0) a.n_matches[f] = nm;
}

// CheckOrientation(lastFrame.keypointsUn, currFrame.keypointsUn, matchIds, currFrame.mappoints)
// (:249-309, :1358-1359): hist of every accepted (idx1, idx2), the kept bins (pjm_keep_bins),
// mappoints[idx2] erased for every pair outside them.
__global__ __launch_bounds__(256) void pjm_orient_kernel(PjArgs a, PjmExtra e) {
    __shared__ int hist[30];
    __shared__ uint32_t keep;
    const int f = blockIdx.x, tid = threadIdx.x;
    const int k0 = a.kp_begin[f], n = a.kp_begin[f + 1] - k0;
    const int m0 = a.mp_begin[f], m1 = a.mp_begin[f + 1];
    if (n > PJ_MAXKP) return;
    if (tid < 30) hist[tid] = 0;
    __syncthreads();
    for (int j = m0 + tid; j < m1; j += 256) {
        const int ch = e.choice[j];
        if (ch >= 0) atomicAdd(&hist[pjm_bin(e.mp_angle[j], e.kp_angle[k0 + ch])], 1);
    }
    __syncthreads();
    if (tid == 0) {
        int kept;
        keep = pjm_keep_bins(hist, &kept);
        a.n_matches[f] = kept;
    }
    __syncthreads();
    const uint32_t k = keep;
    for (int j = m0 + tid; j < m1; j += 256) {
        const int ch = e.choice[j];
        if (ch >= 0 && !((k >> pjm_bin(e.mp_angle[j], e.kp_angle[k0 + ch])) & 1u)) a.kp_match[k0 + ch] = -1;
    }
}

// score -> walk -> optional CheckOrientation, behind the caller's grid (and projection) launches
static int launch_motion_walk(PjArgs& a, PjmExtra& e, int check_ori, hipStream_t st) {
    if (a.total_mp > 0) {
        hipLaunchKernelGGL(pjm_score_kernel, dim3((a.total_mp + 256 / PJ_GW - 1) / (256 / PJ_GW)), dim3(256), 0, st, a, e);
        ORB_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(pjm_walk_kernel, dim3(a.n_frames), dim3(64), 0, st, a, e);
    ORB_HIP_TRY(hipGetLastError());
    if (check_ori) {
        hipLaunchKernelGGL(pjm_orient_kernel, dim3(a.n_frames), dim3(256), 0, st, a, e);
        ORB_HIP_TRY(hipGetLastError());
    }
    return ORB_OK;
}

// Argument checks and the fields of the motion-model entry.
static int motion_common(const orbm_motion_batch* b, int32_t* kp_match, int32_t* n_matches, PjArgs& a, PjmExtra& e) {
    ORB_CHECK_ARG(b, "null argument");
    int rc;
    if ((rc = pj_check_sizes(b->n_frames, b->total_kp, b->total_mp))) return rc;
    std::memset(&a, 0, sizeof(a));
    if ((rc = pj_set_pyramid(a, b->n_levels, b->scale_factors, b->th))) return rc;
    a.n_frames = b->n_frames;
    a.total_mp = b->total_mp;
    if (b->n_frames == 0) return ORB_OK;
    ORB_CHECK_ARG(b->kp_begin && b->mp_begin && b->bounds && kp_match && n_matches, "null array");
    ORB_CHECK_ARG(b->total_kp == 0 || (b->kp_xy && b->kp_octave && b->kp_uright && b->kp_desc), "null keypoint array");
    ORB_CHECK_ARG(b->total_mp == 0 || (b->mp_valid && b->mp_proj && b->mp_octave && b->mp_desc && b->mp_has_obs),
                  "null last-frame point array");
    ORB_CHECK_ARG(!b->check_orientation || (b->kp_angle && (b->total_mp == 0 || b->mp_angle)),
                  "CheckOrientation needs kp_angle / mp_angle");
    a.kp_begin = b->kp_begin; a.kp_xy = b->kp_xy; a.kp_oct = b->kp_octave; a.kp_ur = b->kp_uright;
    a.kp_desc = b->kp_desc; a.kp_claimed = b->kp_claimed; a.bounds = b->bounds;
    a.mp_begin = b->mp_begin; a.mp_valid = b->mp_valid; a.mp_proj = b->mp_proj; a.mp_level = b->mp_octave;
    a.mp_desc = b->mp_desc; a.mp_has_obs = b->mp_has_obs;
    a.kp_match = kp_match;
    a.n_matches = n_matches;
    e = PjmExtra{b->motion, b->kp_angle, b->mp_angle, nullptr, PJ_TH_HIGH, 1};
    return ORB_OK;
}

// ---------------------------------------------------------------- SearchByProjection(Frame&, KeyFrame*, alreadyFound, th, ORBdist)
// reloc_project_kernel turns each keyframe point into the motion-model walk's inputs -- validity,
// projection (u, v) and predicted scale -- with the reference's float expressions; the walk then runs as
// pjm_* with the level window predictedScale +- 1 (motion 0), no stereo gate, every accepted point
// claiming and ORBdist as the distance bound.
struct RelocExtra {
    const float* pose;      // n_frames x 12
    const float* camera;    // n_frames x 4
    const uint8_t* valid;   // caller's flag
    const float* xw;
    const float* max_min;
    float log_sf;
    uint8_t* out_valid;
    float* out_proj;        // total_mp x 3 (u, v, 0)
    int32_t* out_level;
};

__global__ __launch_bounds__(256) void reloc_project_kernel(PjArgs a, RelocExtra r) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= a.total_mp) return;
    const int f = a.mp_frame[j];
    bool ok = r.valid[j] != 0;
    float u = 0.f, v = 0.f;
    int ps = 0;
    if (ok) {
        const float* P = r.pose + 12 * (size_t)f;
        const float* K = r.camera + 4 * (size_t)f;
        const float X0 = r.xw[3 * (size_t)j], X1 = r.xw[3 * (size_t)j + 1], X2 = r.xw[3 * (size_t)j + 2];
        const float3 c = pj_world_to_camera(P, X0, X1, X2);
        const float invZ = 1.f / c.z;   // CameraToImage
        u = invZ * K[0] * c.x + K[2];
        v = invZ * K[1] * c.y + K[3];
        const float* bd = a.bounds + 4 * (size_t)f;
        ok = u >= bd[0] && u < bd[1] && v >= bd[2] && v < bd[3];   // ImageBounds::Contains (Frame.cc:51-54)
        if (ok) {
            const float3 o = pj_camera_centre(P);   // PO = Xw - Ow
            const float dist3D = pj_dist3d(X0 - o.x, X1 - o.y, X2 - o.z);
            const float maxD = r.max_min[2 * (size_t)j], minD = r.max_min[2 * (size_t)j + 1];
            ok = !(dist3D < 0.8f * minD || dist3D > 1.2f * maxD);   // :1399-1401
            if (ok) ps = pj_predict_scale(maxD, dist3D, r.log_sf, a.n_levels);   // PredictScale(dist3D, &frame)
        }
    }
    r.out_valid[j] = ok ? 1 : 0;
    r.out_proj[3 * (size_t)j] = u;
    r.out_proj[3 * (size_t)j + 1] = v;
    r.out_proj[3 * (size_t)j + 2] = 0.f;
    r.out_level[j] = ps;
}

// grid -> projection -> the motion walk over the projection's results
static int launch_reloc(PjArgs& a, RelocExtra& r, PjmExtra& e, int check_ori, hipStream_t st) {
    int rc;
    if ((rc = launch_grid(a, st))) return rc;
    a.mp_valid = r.out_valid;
    a.mp_proj = r.out_proj;
    a.mp_level = r.out_level;
    if (a.total_mp > 0) {
        hipLaunchKernelGGL(reloc_project_kernel, dim3((a.total_mp + 255) / 256), dim3(256), 0, st, a, r);
        ORB_HIP_TRY(hipGetLastError());
    }
    return launch_motion_walk(a, e, check_ori, st);
}

// Argument checks and the fields shared by both relocalisation entries.
static int reloc_common(const orbm_reloc_batch* b, int32_t* kp_match, int32_t* n_matches, PjArgs& a, RelocExtra& r,
                        PjmExtra& e) {
    ORB_CHECK_ARG(b, "null argument");
    int rc;
    if ((rc = pj_check_sizes(b->n_frames, b->total_kp, b->total_mp))) return rc;
    std::memset(&a, 0, sizeof(a));
    std::memset(&r, 0, sizeof(r));
    std::memset(&e, 0, sizeof(e));
    if ((rc = pj_set_pyramid(a, b->n_levels, b->scale_factors, b->th))) return rc;
    ORB_CHECK_ARG(b->orb_dist >= 0 && b->orb_dist < 256, "ORBdist must be in [0, 256)");
    a.n_frames = b->n_frames;
    a.total_mp = b->total_mp;
    r.log_sf = b->log_scale_factor;
    e.max_dist = b->orb_dist;
    e.lvl_up = 1;
    if (b->n_frames == 0) return ORB_OK;
    ORB_CHECK_ARG(b->kp_begin && b->mp_begin && b->bounds && b->pose && b->camera && kp_match && n_matches, "null array");
    ORB_CHECK_ARG(b->total_kp == 0 || (b->kp_xy && b->kp_octave && b->kp_desc), "null keypoint array");
    ORB_CHECK_ARG(b->total_mp == 0 || (b->mp_valid && b->mp_xw && b->mp_max_min && b->mp_desc), "null keyframe point array");
    ORB_CHECK_ARG(!b->check_orientation || (b->kp_angle && (b->total_mp == 0 || b->mp_angle)),
                  "CheckOrientation needs kp_angle / mp_angle");
    a.kp_begin = b->kp_begin; a.kp_xy = b->kp_xy; a.kp_oct = b->kp_octave; a.kp_ur = nullptr;
    a.kp_desc = b->kp_desc; a.kp_claimed = b->kp_claimed; a.bounds = b->bounds;
    a.mp_begin = b->mp_begin; a.mp_desc = b->mp_desc; a.mp_has_obs = nullptr;
    a.kp_match = kp_match;
    a.n_matches = n_matches;
    r.pose = b->pose; r.camera = b->camera; r.valid = b->mp_valid; r.xw = b->mp_xw; r.max_min = b->mp_max_min;
    e.kp_angle = b->kp_angle; e.mp_angle = b->mp_angle;
    return ORB_OK;
}

}  // namespace orbamd
