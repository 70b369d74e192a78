// ORBmatcher::Fuse (both overloads) and the Sim3 SearchByProjection, the projection-and-search stages
// (included by orbp.hip after the grid, scan and walk definitions it builds on).
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
        // Rcw * Xw + tcw (cv::Matx: s = 0; s += a(i, k) * b(k) for k = 0..2)
        const float c0 = ((P[0] * X0 + P[1] * X1) + P[2] * X2) + P[9];
        const float c1 = ((P[3] * X0 + P[4] * X1) + P[5] * X2) + P[10];
        const float c2 = ((P[6] * X0 + P[7] * X1) + P[8] * X2) + P[11];
        ok = !(c2 < 0.f);   // :883 (z == 0 goes on: u, v are then inf or nan and fail Contains)
        if (ok) {
            const float invZ = 1.f / c2;   // CameraToImage
            u = invZ * K[0] * c0 + K[2];
            v = invZ * K[1] * c1 + K[3];
            const float* bd = a.bounds + 4 * (size_t)f;
            ok = u >= bd[0] && u < bd[1] && v >= bd[2] && v < bd[3];   // ImageBounds::Contains (Frame.cc:51-54)
        }
        if (ok) {
            ur = u - K[4] / c2;   // u - DepthToDisparity(Xc.z) (:894)
            // Ow = -Rcw^T * tcw (CameraPose::Invt), PO = Xw - Ow, dist3D = (float)cv::norm(PO) (double sum)
            const float o0 = -((P[0] * P[9] + P[3] * P[10]) + P[6] * P[11]);
            const float o1 = -((P[1] * P[9] + P[4] * P[10]) + P[7] * P[11]);
            const float o2 = -((P[2] * P[9] + P[5] * P[10]) + P[8] * P[11]);
            const float p0 = X0 - o0, p1 = X1 - o1, p2 = X2 - o2;
            const double d0 = (double)p0, d1 = (double)p1, d2 = (double)p2;
            const float dist3D = (float)sqrt((d0 * d0 + d1 * d1) + d2 * d2);
            const float maxD = r.max_min[2 * (size_t)j], minD = r.max_min[2 * (size_t)j + 1];
            ok = !(dist3D < 0.8f * minD || dist3D > 1.2f * maxD);   // :902, MapPoint.cc:382-392
            if (ok) {   // PO.dot(Pn) < 0.5 * dist3D (:907): float Matx::dot, compared in double
                const float* N = r.normal + 3 * (size_t)j;
                const float dot = ((0.f + p0 * N[0]) + p1 * N[1]) + p2 * N[2];
                ok = !((double)dot < 0.5 * (double)dist3D);
            }
            if (ok) {   // PredictScale(dist3D, keyframe) (MapPoint.cc:394-403)
                const float ratio = maxD / dist3D;
                const int sc = (int)ceil(log((double)ratio) / (double)r.log_sf);
                ps = max(0, min(sc, a.n_levels - 1));
            }
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
        const float* bd = a.bounds + 4 * (size_t)f;
        const float minx = bd[0], miny = bd[2];
        const float invW = PJ_COLS / (bd[1] - bd[0]), invH = PJ_ROWS / (bd[3] - bd[2]);
        const int mincx = max((int)floorf(invW * (u - radius - minx)), 0);
        const int maxcx = min((int)ceilf(invW * (u + radius - minx)), PJ_COLS - 1);
        const int mincy = max((int)floorf(invH * (v - radius - miny)), 0);
        const int maxcy = min((int)ceilf(invH * (v + radius - miny)), PJ_ROWS - 1);
        if (!(mincx >= PJ_COLS || maxcx < 0 || mincy >= PJ_ROWS || maxcy < 0)) {
            const int32_t* cs = a.grid_start + (size_t)f * (PJ_CELLS + 1);
            const uint8_t* d1 = a.mp_desc + 32 * (size_t)mj;
            for (int cx = mincx; cx <= maxcx; cx++) {
                const int p0 = cs[cx * PJ_ROWS + mincy], p1 = cs[cx * PJ_ROWS + maxcy + 1];
                for (int p = p0 + lane; p < p1; p += PJ_GW) {
                    const int k = k0 + a.grid_idx[k0 + p];
                    const float kx = a.kp_xy[2 * (size_t)k], ky = a.kp_xy[2 * (size_t)k + 1];
                    if (!(fabsf(kx - u) < radius && fabsf(ky - v) < radius)) continue;
                    const int scale = a.kp_oct[k];
                    if (scale < ps - 1 || scale > ps) continue;
                    if (r.chi2_gate) {
                        const float dx = u - kx, dy = v - ky;   // pt - keypoint.pt (:933)
                        const float kur = a.kp_ur[k];
                        if (kur >= 0) {
                            const float dz = ur - kur;
                            if ((double)(((dx * dx + dy * dy) + dz * dz) * r.inv_sigma2[scale]) > 7.8) continue;
                        } else {
                            if ((double)((dx * dx + dy * dy) * r.inv_sigma2[scale]) > 5.99) continue;
                        }
                    }
                    const int dist = pj_hamming(d1, a.kp_desc + 32 * (size_t)k);
                    best = min(best, ((uint32_t)dist << PJ_IDX_BITS) | (uint32_t)p);
                }
            }
        }
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

// The workspace of both entries: the grid and walk arrays, then choice and fuse_project_kernel's results.
static size_t fuse_workspace_bytes(int n_items, int total_kp, int total_mp) {
    const size_t M = (size_t)std::max(total_mp, 1);
    return pj_workspace_bytes(n_items, total_kp, total_mp) + align_up(M * 4, 256) + align_up(M, 256) +
           align_up(M * 12, 256) + align_up(M * 4, 256);
}

static void fuse_carve(PjArgs& a, FuseExtra& r, PjmExtra& e, char* ws, int total_kp) {
    pj_carve(a, ws, a.n_frames, total_kp, a.total_mp);
    size_t o = pj_workspace_bytes(a.n_frames, total_kp, a.total_mp);
    const size_t M = (size_t)std::max(a.total_mp, 1);
    e.choice = (int32_t*)(ws + o);
    o += align_up(M * 4, 256);
    r.out_valid = (uint8_t*)(ws + o);
    o += align_up(M, 256);
    r.out_proj = (float*)(ws + o);
    o += align_up(M * 12, 256);
    r.out_level = (int32_t*)(ws + o);
}

static int launch_fuse_project(PjArgs& a, FuseExtra& r, hipStream_t st) {
    hipLaunchKernelGGL(pj_grid_kernel, dim3(a.n_frames), dim3(256), 0, st, a);
    ORB_HIP_TRY(hipGetLastError());
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
    if (a.total_mp > 0) {
        hipLaunchKernelGGL(pjm_score_kernel, dim3((a.total_mp + 256 / PJ_GW - 1) / (256 / PJ_GW)), dim3(256), 0, st, a, e);
        ORB_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(pjm_walk_kernel, dim3(a.n_frames), dim3(64), 0, st, a, e);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

// Argument checks and the host-side fields shared by the four entries (sim3: no chi2 gate, no uright).
static int fuse_common(const orbm_fuse_batch* b, bool sim3, PjArgs& a, FuseExtra& r, PjmExtra& e) {
    ORB_CHECK_ARG(b, "null argument");
    ORB_CHECK_ARG(b->n_items >= 0 && b->total_kp >= 0 && b->total_mp >= 0, "negative sizes");
    ORB_CHECK_ARG(b->n_levels >= 1 && b->n_levels <= PJ_MAX_LEVELS && b->scale_factors, "bad scale pyramid");
    const bool chi2 = !sim3 && b->chi2_gate;
    ORB_CHECK_ARG(!chi2 || b->inv_sigma2, "chi2_gate needs inv_sigma2");
    std::memset(&a, 0, sizeof(a));
    std::memset(&r, 0, sizeof(r));
    std::memset(&e, 0, sizeof(e));
    a.n_frames = b->n_items;
    a.n_levels = b->n_levels;
    for (int l = 0; l < b->n_levels; l++) a.scale[l] = b->scale_factors[l];
    if (chi2)
        for (int l = 0; l < b->n_levels; l++) r.inv_sigma2[l] = b->inv_sigma2[l];
    a.th = b->th;
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
    return ORB_OK;
}

// kp_begin / mp_begin of a host batch (as orbm_search_by_projection checks them)
static int fuse_check_offsets(const orbm_fuse_batch* b) {
    const int F = b->n_items;
    ORB_CHECK_ARG(b->kp_begin[0] == 0 && b->mp_begin[0] == 0 && b->kp_begin[F] == b->total_kp &&
                      b->mp_begin[F] == b->total_mp,
                  "kp_begin / mp_begin must start at 0 and end at total_kp / total_mp");
    for (int f = 0; f < F; f++) {
        ORB_CHECK_ARG(b->kp_begin[f + 1] >= b->kp_begin[f] && b->mp_begin[f + 1] >= b->mp_begin[f],
                      "offsets must be non-decreasing");
        ORB_CHECK_ARG(b->kp_begin[f + 1] - b->kp_begin[f] <= PJ_MAXKP, "keyframe has more than ORBM_PROJ_MAX_KP keypoints");
    }
    return ORB_OK;
}

// A host batch copied into `io`: `d` = the batch with device pointers (scale_factors / inv_sigma2 stay
// host), d_claimed = kp_claimed's copy or NULL.
static int fuse_upload(const orbm_fuse_batch* b, const uint8_t* kp_claimed, DevBuf& io, size_t extra_bytes,
                       orbm_fuse_batch& d, const uint8_t*& d_claimed, char*& d_extra) {
    const int F = b->n_items, K = b->total_kp, M = b->total_mp;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += align_up(std::max<size_t>(bytes, 1), 256); return o; };
    const size_t o_kb = take((size_t)(F + 1) * 4), o_xy = take((size_t)K * 8), o_oc = take((size_t)K * 4),
                 o_ur = take((size_t)K * 4), o_kd = take((size_t)K * 32), o_kc = take(kp_claimed ? (size_t)K : 0),
                 o_bd = take((size_t)F * 16), o_po = take((size_t)F * 48), o_ca = take((size_t)F * 20),
                 o_mb = take((size_t)(F + 1) * 4), o_mv = take((size_t)M), o_mx = take((size_t)M * 12),
                 o_mm = take((size_t)M * 8), o_mn = take((size_t)M * 12), o_md = take((size_t)M * 32),
                 o_ex = take(extra_bytes);
    int rc;
    if ((rc = io.reserve(off))) return rc;
    char* p = io.as<char>();
    auto up = [&](size_t o, const void* src, size_t bytes) -> int {
        if (bytes && src) ORB_HIP_TRY(hipMemcpy(p + o, src, bytes, hipMemcpyHostToDevice));
        return ORB_OK;
    };
    if ((rc = up(o_kb, b->kp_begin, (size_t)(F + 1) * 4)) || (rc = up(o_xy, b->kp_xy, (size_t)K * 8)) ||
        (rc = up(o_oc, b->kp_octave, (size_t)K * 4)) || (rc = up(o_ur, b->kp_uright, (size_t)K * 4)) ||
        (rc = up(o_kd, b->kp_desc, (size_t)K * 32)) || (rc = up(o_kc, kp_claimed, (size_t)K)) ||
        (rc = up(o_bd, b->bounds, (size_t)F * 16)) || (rc = up(o_po, b->pose, (size_t)F * 48)) ||
        (rc = up(o_ca, b->camera, (size_t)F * 20)) || (rc = up(o_mb, b->mp_begin, (size_t)(F + 1) * 4)) ||
        (rc = up(o_mv, b->mp_valid, (size_t)M)) || (rc = up(o_mx, b->mp_xw, (size_t)M * 12)) ||
        (rc = up(o_mm, b->mp_max_min, (size_t)M * 8)) || (rc = up(o_mn, b->mp_normal, (size_t)M * 12)) ||
        (rc = up(o_md, b->mp_desc, (size_t)M * 32)))
        return rc;
    d = *b;
    d.kp_begin = (const int32_t*)(p + o_kb); d.kp_xy = (const float*)(p + o_xy); d.kp_octave = (const int32_t*)(p + o_oc);
    d.kp_uright = b->kp_uright ? (const float*)(p + o_ur) : nullptr; d.kp_desc = (const uint8_t*)(p + o_kd);
    d.bounds = (const float*)(p + o_bd); d.pose = (const float*)(p + o_po); d.camera = (const float*)(p + o_ca);
    d.mp_begin = (const int32_t*)(p + o_mb); d.mp_valid = (const uint8_t*)(p + o_mv); d.mp_xw = (const float*)(p + o_mx);
    d.mp_max_min = (const float*)(p + o_mm); d.mp_normal = (const float*)(p + o_mn); d.mp_desc = (const uint8_t*)(p + o_md);
    d_claimed = kp_claimed ? (const uint8_t*)(p + o_kc) : nullptr;
    d_extra = p + o_ex;
    return ORB_OK;
}

}  // namespace orbamd
