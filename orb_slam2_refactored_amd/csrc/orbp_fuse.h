// ORBmatcher::Fuse (both overloads) and the Sim3 SearchByProjection, the projection-and-search stages
// (included by orbp.hip after orbp_grid.h, orbp_host.h and orbp_motion.h, whose grid, window scan and
// motion walk it builds on).
//
// Reference: src/ORBmatcher.cc:868-980 (Fuse(KeyFrame*, const std::vector<MapPoint*>&, th),
// LocalMapping::SearchInNeighbors), :982-1088 (Fuse(KeyFrame*, const Sim3&, points, th, replacePoints),
// LoopClosing::SearchAndFuse) and :518-612 (SearchByProjection(const KeyFrame*, const Sim3&, points,
// matched, th), LoopClosing::ComputeSim3).  All three project world points through a pose, gate them
// (depth, image, invariance distance, viewing angle), predict a scale level, search the FeaturesGrid
// window th * scaleFactors[predictedScale] over the levels [predictedScale - 1, predictedScale] and keep
// the first minimum-Hamming keypoint with bestDist <= TH_LOW.
//   fuse_project_kernel  one thread per map point: the gates in the reference's order and float
//                        expressions -> (valid, u, v, ur, predictedScale)
//   fuse_best_kernel     a 16-lane group per map point: the window scan, the level and chi2 gates and
//                        the group minimum of (dist << 13 | scan position)
// The Sim3 search runs fuse_project_kernel and then the relocalisation score and claim walk
// (pjm_score_kernel / pjm_walk_kernel: a keypoint that holds a match, on entry or taken by an earlier
// point of the call, is skipped, :588).
//
// Fuse needs no ordered walk.  Its loop writes only the pointer graph (Replace, AddObservation,
// AddMapPoint, replacePoints[i]); what it reads per point -- the skip test, the point's position,
// normal, distances and descriptor, the keyframe's keypoints -- is not changed by those calls for any
// other point of the list, and no keypoint is skipped for holding a map point.  So with the skip mask
// taken on entry and distinct entries, every point's (bestIdx, bestDist) is independent of the
// iterations before it.  Preconditions (the caller's side of the contract):
//   mp_valid[m] = mappoint && !isBad() && !IsInKeyFrame(keyframe)   (:876, first overload)
//   mp_valid[m] = !isBad() && !alreadyFound.count(mappoint)         (:1002, Sim3 overload; :537)
// both evaluated on entry, over a list with distinct points (SearchInNeighbors' fuseCandidateForKF marks
// guarantee it).  The caller then applies the pointer-graph part (:957-976, :1070-1084) in list order
// from best_idx.
#pragma once

namespace orbamd {

constexpr int FUSE_TH_LOW = 50;   // ORBmatcher.cc:42

struct FuseExtra {
    const float* pose;      // n_items x 12: Rcw (row-major) then tcw
    const float* camera;    // n_items x 5: fx, fy, cx, cy, bf
    const uint8_t* valid;   // the caller's flag
    const float* xw;
    const float* max_min;
    const float* normal;
    float log_sf;
    float inv_sigma2[PJ_MAX_LEVELS];
    int chi2_gate;
    // workspace: fuse_project_kernel's results (the walk reads them as mp_valid / mp_proj / mp_level)
    uint8_t* out_valid;
    float* out_proj;        // total_mp x 3 (u, v, ur)
    int32_t* out_level;
    // Fuse outputs
    int32_t* best_idx;
    int32_t* best_dist;
    int32_t* n_fused;
};

__global__ __launch_bounds__(256) void fuse_project_kernel(PjArgs a, FuseExtra r) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (r.n_fused)   // the count fuse_best_kernel adds to; -1 reports an item over the keypoint limit
        for (int f = j; f < a.n_frames; f += gridDim.x * 256)
            r.n_fused[f] = a.kp_begin[f + 1] - a.kp_begin[f] > PJ_MAXKP ? -1 : 0;
    if (j >= a.total_mp) return;
    const int f = a.mp_frame[j];
    bool ok = r.valid[j] != 0;
    float u = 0.f, v = 0.f, ur = 0.f;
    int ps = 0;
    if (ok) {
        const float* P = r.pose + 12 * (size_t)f;
        const float* K = r.camera + 5 * (size_t)f;
        const float X0 = r.xw[3 * (size_t)j], X1 = r.xw[3 * (size_t)j + 1], X2 = r.xw[3 * (size_t)j + 2];
        const float3 c = pj_world_to_camera(P, X0, X1, X2);
        ok = !(c.z < 0.f);   // :883 (z == 0 goes on: u, v are then inf or nan and fail Contains)
        if (ok) {
            const float invZ = 1.f / c.z;   // CameraToImage
            u = invZ * K[0] * c.x + K[2];
            v = invZ * K[1] * c.y + K[3];
            const float* bd = a.bounds + 4 * (size_t)f;
            ok = u >= bd[0] && u < bd[1] && v >= bd[2] && v < bd[3];   // ImageBounds::Contains (Frame.cc:51-54)
        }
        if (ok) {
            ur = u - K[4] / c.z;   // u - DepthToDisparity(Xc.z) (:894)
            const float3 o = pj_camera_centre(P);   // PO = Xw - Ow
            const float p0 = X0 - o.x, p1 = X1 - o.y, p2 = X2 - o.z;
            const float dist3D = pj_dist3d(p0, p1, p2);
            const float maxD = r.max_min[2 * (size_t)j], minD = r.max_min[2 * (size_t)j + 1];
            ok = !(dist3D < 0.8f * minD || dist3D > 1.2f * maxD);   // :902, MapPoint.cc:382-392
            if (ok) {   // PO.dot(Pn) < 0.5 * dist3D (:907): float Matx::dot, compared in double
                const float* N = r.normal + 3 * (size_t)j;
                const float dot = ((0.f + p0 * N[0]) + p1 * N[1]) + p2 * N[2];
                ok = !((double)dot < 0.5 * (double)dist3D);
            }
            if (ok) ps = pj_predict_scale(maxD, dist3D, r.log_sf, a.n_levels);   // PredictScale(dist3D, keyframe)
        }
    }
    r.out_valid[j] = ok ? 1 : 0;
    r.out_proj[3 * (size_t)j] = u;
    r.out_proj[3 * (size_t)j + 1] = v;
    r.out_proj[3 * (size_t)j + 2] = ur;
    r.out_level[j] = ps;
}

// GetFeaturesInArea(u, v, th * scaleFactors[ps]) (no level filter in the grid call), then the loop of
// :925-954 / :1054-1067: the level window, the chi2 gates of the first overload, the strict-< minimum.
__global__ __launch_bounds__(256) void fuse_best_kernel(PjArgs a, FuseExtra r) {
    const int lane = threadIdx.x & (PJ_GW - 1);
    const int mj = blockIdx.x * (256 / PJ_GW) + (threadIdx.x / PJ_GW);
    if (mj >= a.total_mp) return;   // group-uniform
    const int f = a.mp_frame[mj];
    const int k0 = a.kp_begin[f], n = a.kp_begin[f + 1] - k0;
    uint32_t best = PJ_NONE;
    if (n <= PJ_MAXKP && r.out_valid[mj]) {
        const int ps = r.out_level[mj];
        const float u = r.out_proj[3 * (size_t)mj], v = r.out_proj[3 * (size_t)mj + 1];
        const float ur = r.out_proj[3 * (size_t)mj + 2];
        const float radius = a.th * a.scale[ps];
        const PjWindow w = pj_window(pj_bounds(a.bounds + 4 * (size_t)f), u, v, radius);
        const uint8_t* d1 = a.mp_desc + 32 * (size_t)mj;
        pj_scan_window<PJ_GW>(w, a.grid_start + (size_t)f * (PJ_CELLS + 1), a.grid_idx, k0, lane, [&](int p, int idx) {
            const int k = k0 + idx;
            const float kx = a.kp_xy[2 * (size_t)k], ky = a.kp_xy[2 * (size_t)k + 1];
            if (!pj_in_box(kx, ky, u, v, radius)) return;
            const int scale = a.kp_oct[k];
            if (scale < ps - 1 || scale > ps) return;
            if (r.chi2_gate) {
                const float dx = u - kx, dy = v - ky;   // pt - keypoint.pt (:933)
                const float kur = a.kp_ur[k];
                if (kur >= 0) {
                    const float dz = ur - kur;
                    if ((double)(((dx * dx + dy * dy) + dz * dz) * r.inv_sigma2[scale]) > 7.8) return;
                } else {
                    if ((double)((dx * dx + dy * dy) * r.inv_sigma2[scale]) > 5.99) return;
                }
            }
            const int dist = pj_hamming(d1, a.kp_desc + 32 * (size_t)k);
            best = min(best, ((uint32_t)dist << PJ_IDX_BITS) | (uint32_t)p);
        });
    }
    best = pj_wave_min<PJ_GW>(best);
    if (lane == 0) {
        const int dist = best == PJ_NONE ? 256 : (int)(best >> PJ_IDX_BITS);
        int idx = -1;
        if (best != PJ_NONE && dist <= FUSE_TH_LOW) idx = a.grid_idx[k0 + (int)(best & PJ_IDX_MASK)];
        r.best_idx[mj] = idx;
        r.best_dist[mj] = dist;
        if (idx >= 0) atomicAdd(&r.n_fused[f], 1);   // nfused++ on both branches of :957-976
    }
}

static int launch_fuse_project(PjArgs& a, FuseExtra& r, hipStream_t st) {
    int rc;
    if ((rc = launch_grid(a, st))) return rc;
    hipLaunchKernelGGL(fuse_project_kernel, dim3(std::max((a.total_mp + 255) / 256, 1)), dim3(256), 0, st, a, r);
    ORB_HIP_TRY(hipGetLastError());
    a.mp_valid = r.out_valid;
    a.mp_proj = r.out_proj;
    a.mp_level = r.out_level;
    return ORB_OK;
}

static int launch_fuse(PjArgs& a, FuseExtra& r, hipStream_t st) {
    int rc;
    if ((rc = launch_fuse_project(a, r, st))) return rc;
    if (a.total_mp > 0) {
        hipLaunchKernelGGL(fuse_best_kernel, dim3((a.total_mp + 256 / PJ_GW - 1) / (256 / PJ_GW)), dim3(256), 0, st, a, r);
        ORB_HIP_TRY(hipGetLastError());
    }
    return ORB_OK;
}

static int launch_sim3(PjArgs& a, FuseExtra& r, PjmExtra& e, hipStream_t st) {
    int rc;
    if ((rc = launch_fuse_project(a, r, st))) return rc;
    return launch_motion_walk(a, e, 0, st);   // no CheckOrientation in this search
}

// Argument checks and the fields shared by the four entries (sim3: no chi2 gate, no uright).
static int fuse_common(const orbm_fuse_batch* b, bool sim3, PjArgs& a, FuseExtra& r, PjmExtra& e) {
    ORB_CHECK_ARG(b, "null argument");
    int rc;
    if ((rc = pj_check_sizes(b->n_items, b->total_kp, b->total_mp))) return rc;
    std::memset(&a, 0, sizeof(a));
    std::memset(&r, 0, sizeof(r));
    std::memset(&e, 0, sizeof(e));
    if ((rc = pj_set_pyramid(a, b->n_levels, b->scale_factors, b->th))) return rc;
    const bool chi2 = !sim3 && b->chi2_gate;
    ORB_CHECK_ARG(!chi2 || b->inv_sigma2, "chi2_gate needs inv_sigma2");
    a.n_frames = b->n_items;
    if (chi2)
        for (int l = 0; l < b->n_levels; l++) r.inv_sigma2[l] = b->inv_sigma2[l];
    a.total_mp = b->total_mp;
    r.log_sf = b->log_scale_factor;
    r.chi2_gate = chi2 ? 1 : 0;
    e.max_dist = FUSE_TH_LOW;   // :604
    e.lvl_up = 0;               // levels [predictedScale - 1, predictedScale] (:592)
    if (b->n_items == 0) return ORB_OK;
    ORB_CHECK_ARG(b->kp_begin && b->mp_begin && b->bounds && b->pose && b->camera, "null array");
    ORB_CHECK_ARG(b->total_kp == 0 || (b->kp_xy && b->kp_octave && b->kp_desc && (!chi2 || b->kp_uright)),
                  "null keypoint array");
    ORB_CHECK_ARG(b->total_mp == 0 || (b->mp_valid && b->mp_xw && b->mp_max_min && b->mp_normal && b->mp_desc),
                  "null map point array");
    a.kp_begin = b->kp_begin; a.kp_xy = b->kp_xy; a.kp_oct = b->kp_octave; a.kp_desc = b->kp_desc;
    a.bounds = b->bounds; a.mp_begin = b->mp_begin; a.mp_desc = b->mp_desc;
    r.pose = b->pose; r.camera = b->camera; r.valid = b->mp_valid; r.xw = b->mp_xw; r.max_min = b->mp_max_min;
    r.normal = b->mp_normal;
    return ORB_OK;
}

// The grid region and the projected-point block of both device entries.
static int fuse_workspace(PjScratch& s, const orbm_fuse_batch* b, PjArgs& a, FuseExtra& r, PjmExtra& e) {
    orbamd_host::PjGridLayout g;
    orbamd_host::PjPointLayout p;
    int rc;
    if ((rc = s.workspace([&](Carver& c) {
            g.carve(c, b->n_items, b->total_kp, b->total_mp);
            p.carve(c, b->total_mp);
        })))
        return rc;
    pj_bind(a, g);
    e.choice = p.choice;
    r.out_valid = p.out_valid;
    r.out_proj = p.out_proj;
    r.out_level = p.out_level;
    return ORB_OK;
}

// The arrays of a host batch (scale_factors / inv_sigma2 stay host)
static void fuse_mirror(Mirror& io, orbm_fuse_batch& d) {
    const size_t F = d.n_items, K = d.total_kp, M = d.total_mp;
    io.add(d.kp_begin, F + 1, true, false); io.add(d.kp_xy, 2 * K, true, false); io.add(d.kp_octave, K, true, false);
    io.add(d.kp_uright, K, true, false); io.add(d.kp_desc, 32 * K, true, false); io.add(d.bounds, 4 * F, true, false);
    io.add(d.pose, 12 * F, true, false); io.add(d.camera, 5 * F, true, false); io.add(d.mp_begin, F + 1, true, false);
    io.add(d.mp_valid, M, true, false); io.add(d.mp_xw, 3 * M, true, false); io.add(d.mp_max_min, 2 * M, true, false);
    io.add(d.mp_normal, 3 * M, true, false); io.add(d.mp_desc, 32 * M, true, false);
}

}  // namespace orbamd
