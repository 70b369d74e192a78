// orbp.hip — the FeaturesGrid and the projection searches of ORBmatcher on gfx950 (SURVEY.md §8f, next
// row 2), batched over frames: the C entries.  The kernels and their launch sequences live in one header
// per search family, included below in dependency order:
//   orbp_layout.h  the workspace regions (plain C++, shared with the CPU layout check)
//   orbp_grid.h    constants, PjArgs, pj_grid_kernel, GetFeaturesInArea's window and scan order,
//                  CheckOrientation's bin selection, the projection float sequences
//   orbp_host.h    PjScratch (workspace), the shared batch checks
//   orbp_track.h   SearchByProjection(Frame&, const std::vector<MapPoint*>&, th): pj_score / pj_walk
//   orbp_motion.h  the motion-model search (pjm_*) and the relocalisation search (reloc_*)
//   orbp_init.h    SearchForInitialization (pi_*)
//   orbp_fuse.h    Fuse and the Sim3 SearchByProjection (fuse_*)
//   orbp_sim3.h    SearchBySim3 (sim3_*)
// Every search has a device entry (arrays in HBM, enqueue only) that checks the batch, carves the
// workspace and launches, and a host entry that adds the host-only checks (offsets, per-frame limits,
// value ranges) before any copy, uploads the batch and calls the device entry on the null stream.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <initializer_list>

#include "common.h"
#include "qt_sort.h"
#include "orbp_layout.h"
#include "orbp_grid.h"
#include "orbp_host.h"
#include "orbp_track.h"
#include "orbp_motion.h"
#include "orbp_init.h"
#include "orbp_fuse.h"
#include "orbp_sim3.h"

using namespace orbamd;

thread_local PjScratch g_pj;

// ---------------------------------------------------------------- SearchByProjection(Frame&, vector<MapPoint*>)
extern "C" int orbm_search_by_projection_device(const orbm_proj_batch* b, int32_t* kp_match, int32_t* n_matches,
                                                void* stream) {
    PjArgs a;
    int rc;
    if ((rc = proj_common(b, kp_match, n_matches, a))) return rc;
    if (b->n_frames == 0) return ORB_OK;
    if ((rc = g_pj.use_current_device())) return rc;
    orbamd_host::PjGridLayout g;
    if ((rc = g_pj.workspace([&](Carver& c) { g.carve(c, b->n_frames, b->total_kp, b->total_mp); }))) return rc;
    pj_bind(a, g);
    return launch_projection(a, (hipStream_t)stream);
}

extern "C" int orbm_search_by_projection(const orbm_proj_batch* b, int32_t* kp_match, int32_t* n_matches,
                                         int device) {
    PjArgs a;
    int rc;
    if ((rc = proj_common(b, kp_match, n_matches, a))) return rc;   // the checks, before any copy
    const size_t F = b->n_frames, K = b->total_kp, M = b->total_mp;
    if (F == 0) return ORB_OK;
    if ((rc = pj_check_offsets(b->n_frames, b->kp_begin, b->total_kp, b->mp_begin, b->total_mp, false, PJ_ENDS_MSG,
                               PJ_FRAME_LIMIT_MSG)))
        return rc;
    for (size_t j = 0; j < M; j++)
        ORB_CHECK_ARG(!b->mp_valid[j] || (b->mp_level[j] >= 0 && b->mp_level[j] < b->n_levels),
                      "trackScaleLevel out of range (scaleFactors[predictedScale], ORBmatcher.cc:328)");
    orbm_proj_batch d = *b;
    Mirror io;
    io.add(d.kp_begin, F + 1, true, false); io.add(d.kp_xy, 2 * K, true, false); io.add(d.kp_octave, K, true, false);
    io.add(d.kp_uright, K, true, false); io.add(d.kp_desc, 32 * K, true, false); io.add(d.kp_claimed, K, true, false);
    io.add(d.bounds, 4 * F, true, false); io.add(d.mp_begin, F + 1, true, false); io.add(d.mp_valid, M, true, false);
    io.add(d.mp_proj, 3 * M, true, false); io.add(d.mp_view_cos, M, true, false); io.add(d.mp_level, M, true, false);
    io.add(d.mp_desc, 32 * M, true, false); io.add(d.mp_has_obs, M, true, false);
    io.add(kp_match, K, false, true); io.add(n_matches, F, false, true);
    return run_host(g_pj, device, io, [&] { return orbm_search_by_projection_device(&d, kp_match, n_matches, nullptr); });
}

// ---------------------------------------------------------------- SearchByProjection(Frame&, const Frame&, th, mono)
extern "C" int orbm_search_by_projection_motion_device(const orbm_motion_batch* b, int32_t* kp_match,
                                                       int32_t* n_matches, void* stream) {
    PjArgs a;
    PjmExtra e;
    int rc;
    if ((rc = motion_common(b, kp_match, n_matches, a, e))) return rc;
    if (b->n_frames == 0) return ORB_OK;
    if ((rc = g_pj.use_current_device())) return rc;
    orbamd_host::PjGridLayout g;
    if ((rc = g_pj.workspace([&](Carver& c) {
            g.carve(c, b->n_frames, b->total_kp, b->total_mp);
            c.take(e.choice, b->total_mp);
        })))
        return rc;
    pj_bind(a, g);
    if ((rc = launch_grid(a, (hipStream_t)stream))) return rc;
    return launch_motion_walk(a, e, b->check_orientation, (hipStream_t)stream);
}

// ---------------------------------------------------------------- SearchForInitialization
extern "C" int orbm_search_for_initialization_device(const orbm_init_batch* b, int32_t* matches12, int32_t* n_matches,
                                                     void* stream) {
    PjArgs a;
    PiExtra e;
    int rc;
    if ((rc = pi_common(b, matches12, n_matches, a, e))) return rc;
    if (b->n_pairs == 0) return ORB_OK;
    if ((rc = g_pj.use_current_device())) return rc;
    orbamd_host::PjGridLayout g;
    orbamd_host::PiLayout p;
    if ((rc = g_pj.workspace([&](Carver& c) {
            g.carve(c, b->n_pairs, b->total_kp, b->total_q);
            p.carve(c, b->total_q);
        })))
        return rc;
    pj_bind(a, g);
    e.cnt = p.cnt;
    e.cand = p.cand;
    return launch_init(a, e, (hipStream_t)stream);
}

extern "C" int orbm_search_for_initialization(const orbm_init_batch* b, int32_t* matches12, int32_t* n_matches,
                                              int device) {
    PjArgs a;
    PiExtra e;
    int rc;
    if ((rc = pi_common(b, matches12, n_matches, a, e))) return rc;   // the checks, before any copy
    const size_t P = b->n_pairs, K = b->total_kp, Q = b->total_q;
    if (P == 0) return ORB_OK;
    if ((rc = pj_check_offsets(b->n_pairs, b->kp_begin, b->total_kp, b->q_begin, b->total_q, true,
                               "kp_begin / q_begin must start at 0 and end at total_kp / total_q", PJ_FRAME_LIMIT_MSG)))
        return rc;
    if (b->check_orientation) {
        for (size_t k = 0; k < K; k++)
            ORB_CHECK_ARG(b->kp_angle[k] >= 0.f && b->kp_angle[k] < 360.f, "keypoint angle outside [0, 360) (CV_Assert in CheckOrientation)");
        for (size_t q = 0; q < Q; q++)
            ORB_CHECK_ARG(b->q_angle[q] >= 0.f && b->q_angle[q] < 360.f, "keypoint angle outside [0, 360) (CV_Assert in CheckOrientation)");
    }
    orbm_init_batch d = *b;   // d.prev_matched: the uploaded copy, which the device entry updates in place
    Mirror io;
    io.add(d.kp_begin, P + 1, true, false); io.add(d.kp_xy, 2 * K, true, false); io.add(d.kp_octave, K, true, false);
    io.add(d.kp_desc, 32 * K, true, false); io.add(d.kp_angle, K, true, false); io.add(d.bounds, 4 * P, true, false);
    io.add(d.q_begin, P + 1, true, false); io.add(d.q_octave, Q, true, false); io.add(d.q_desc, 32 * Q, true, false);
    io.add(d.q_angle, Q, true, false); io.add(d.prev_matched, 2 * Q, true, true);
    io.add(matches12, Q, false, true); io.add(n_matches, P, false, true);
    return run_host(g_pj, device, io, [&] { return orbm_search_for_initialization_device(&d, matches12, n_matches, nullptr); });
}

// ---------------------------------------------------------------- SearchByProjection(Frame&, KeyFrame*, alreadyFound, th, ORBdist)
extern "C" int orbm_search_by_projection_reloc_device(const orbm_reloc_batch* b, int32_t* kp_match, int32_t* n_matches,
                                                      void* stream) {
    PjArgs a;
    RelocExtra r;
    PjmExtra e;
    int rc;
    if ((rc = reloc_common(b, kp_match, n_matches, a, r, e))) return rc;
    if (b->n_frames == 0) return ORB_OK;
    if ((rc = g_pj.use_current_device())) return rc;
    orbamd_host::PjGridLayout g;
    orbamd_host::PjPointLayout p;
    if ((rc = g_pj.workspace([&](Carver& c) {
            g.carve(c, b->n_frames, b->total_kp, b->total_mp);
            p.carve(c, b->total_mp);
        })))
        return rc;
    pj_bind(a, g);
    e.choice = p.choice;
    r.out_valid = p.out_valid;
    r.out_proj = p.out_proj;
    r.out_level = p.out_level;
    return launch_reloc(a, r, e, b->check_orientation, (hipStream_t)stream);
}

extern "C" int orbm_search_by_projection_reloc(const orbm_reloc_batch* b, int32_t* kp_match, int32_t* n_matches,
                                               int device) {
    PjArgs a;
    RelocExtra r;
    PjmExtra e;
    int rc;
    if ((rc = reloc_common(b, kp_match, n_matches, a, r, e))) return rc;   // the checks, before any copy
    const size_t F = b->n_frames, K = b->total_kp, M = b->total_mp;
    if (F == 0) return ORB_OK;
    if ((rc = pj_check_offsets(b->n_frames, b->kp_begin, b->total_kp, b->mp_begin, b->total_mp, false, PJ_ENDS_MSG,
                               PJ_FRAME_LIMIT_MSG)))
        return rc;
    orbm_reloc_batch d = *b;
    Mirror io;
    io.add(d.kp_begin, F + 1, true, false); io.add(d.kp_xy, 2 * K, true, false); io.add(d.kp_octave, K, true, false);
    io.add(d.kp_desc, 32 * K, true, false); io.add(d.kp_angle, K, true, false); io.add(d.kp_claimed, K, true, false);
    io.add(d.bounds, 4 * F, true, false); io.add(d.pose, 12 * F, true, false); io.add(d.camera, 4 * F, true, false);
    io.add(d.mp_begin, F + 1, true, false); io.add(d.mp_valid, M, true, false); io.add(d.mp_xw, 3 * M, true, false);
    io.add(d.mp_max_min, 2 * M, true, false); io.add(d.mp_desc, 32 * M, true, false); io.add(d.mp_angle, M, true, false);
    io.add(kp_match, K, false, true); io.add(n_matches, F, false, true);
    return run_host(g_pj, device, io, [&] { return orbm_search_by_projection_reloc_device(&d, kp_match, n_matches, nullptr); });
}

// ---------------------------------------------------------------- Fuse
extern "C" int orbm_fuse_device(const orbm_fuse_batch* b, int32_t* best_idx, int32_t* best_dist, int32_t* n_fused,
                                void* stream) {
    PjArgs a;
    FuseExtra r;
    PjmExtra e;
    int rc;
    if ((rc = fuse_common(b, false, a, r, e))) return rc;
    if (b->n_items == 0) return ORB_OK;
    ORB_CHECK_ARG(n_fused && (b->total_mp == 0 || (best_idx && best_dist)), "null output array");
    a.kp_ur = b->kp_uright;
    r.best_idx = best_idx; r.best_dist = best_dist; r.n_fused = n_fused;
    if ((rc = g_pj.use_current_device())) return rc;
    if ((rc = fuse_workspace(g_pj, b, a, r, e))) return rc;
    return launch_fuse(a, r, (hipStream_t)stream);
}

extern "C" int orbm_fuse(const orbm_fuse_batch* b, int32_t* best_idx, int32_t* best_dist, int32_t* n_fused, int device) {
    PjArgs a;
    FuseExtra r;
    PjmExtra e;
    int rc;
    if ((rc = fuse_common(b, false, a, r, e))) return rc;   // the checks, before any copy
    const size_t F = b->n_items, M = b->total_mp;
    if (F == 0) return ORB_OK;
    ORB_CHECK_ARG(n_fused && (M == 0 || (best_idx && best_dist)), "null output array");
    if ((rc = pj_check_offsets(b->n_items, b->kp_begin, b->total_kp, b->mp_begin, b->total_mp, false, PJ_ENDS_MSG,
                               PJ_KEYFRAME_LIMIT_MSG)))
        return rc;
    orbm_fuse_batch d = *b;
    Mirror io;
    fuse_mirror(io, d);
    io.add(best_idx, M, false, true); io.add(best_dist, M, false, true); io.add(n_fused, F, false, true);
    return run_host(g_pj, device, io, [&] { return orbm_fuse_device(&d, best_idx, best_dist, n_fused, nullptr); });
}

// ---------------------------------------------------------------- SearchByProjection(const KeyFrame*, const Sim3&, ...)
extern "C" int orbm_search_by_projection_sim3_device(const orbm_fuse_batch* b, const uint8_t* kp_claimed,
                                                     int32_t* kp_match, int32_t* n_matches, void* stream) {
    PjArgs a;
    FuseExtra r;
    PjmExtra e;
    int rc;
    if ((rc = fuse_common(b, true, a, r, e))) return rc;
    if (b->n_items == 0) return ORB_OK;
    ORB_CHECK_ARG(n_matches && (b->total_kp == 0 || kp_match), "null output array");
    a.kp_ur = nullptr;          // no stereo gate
    a.kp_claimed = kp_claimed;
    a.mp_has_obs = nullptr;     // every accepted point claims (:606)
    a.kp_match = kp_match;
    a.n_matches = n_matches;
    if ((rc = g_pj.use_current_device())) return rc;
    if ((rc = fuse_workspace(g_pj, b, a, r, e))) return rc;
    return launch_sim3(a, r, e, (hipStream_t)stream);
}

extern "C" int orbm_search_by_projection_sim3(const orbm_fuse_batch* b, const uint8_t* kp_claimed, int32_t* kp_match,
                                              int32_t* n_matches, int device) {
    PjArgs a;
    FuseExtra r;
    PjmExtra e;
    int rc;
    if ((rc = fuse_common(b, true, a, r, e))) return rc;   // the checks, before any copy
    const size_t F = b->n_items, K = b->total_kp;
    if (F == 0) return ORB_OK;
    ORB_CHECK_ARG(n_matches && (K == 0 || kp_match), "null output array");
    if ((rc = pj_check_offsets(b->n_items, b->kp_begin, b->total_kp, b->mp_begin, b->total_mp, false, PJ_ENDS_MSG,
                               PJ_KEYFRAME_LIMIT_MSG)))
        return rc;
    orbm_fuse_batch d = *b;
    Mirror io;
    fuse_mirror(io, d);
    io.add(kp_claimed, K, true, false); io.add(kp_match, K, false, true); io.add(n_matches, F, false, true);
    return run_host(g_pj, device, io, [&] {
        return orbm_search_by_projection_sim3_device(&d, kp_claimed, kp_match, n_matches, nullptr);
    });
}

// ---------------------------------------------------------------- SearchBySim3
extern "C" int orbm_search_by_sim3_device(const orbm_sim3_batch* b, int32_t* match12, int32_t* match1, int32_t* match2,
                                          int32_t* n_found, void* stream) {
    Sim3Args a;
    int rc;
    if ((rc = sim3_common(b, a))) return rc;
    if (b->n_pairs == 0) return ORB_OK;
    ORB_CHECK_ARG(n_found && (b->total_kp1 == 0 || match12), "null output array");
    a.match12 = match12;
    a.n_found = n_found;
    if ((rc = g_pj.use_current_device())) return rc;
    if ((rc = sim3_workspace(g_pj, a, match1, match2))) return rc;
    return launch_search_by_sim3(a, (hipStream_t)stream);
}

extern "C" int orbm_search_by_sim3(const orbm_sim3_batch* b, int32_t* match12, int32_t* match1, int32_t* match2,
                                   int32_t* n_found, int device) {
    Sim3Args a;
    int rc;
    if ((rc = sim3_common(b, a))) return rc;   // the checks, before any copy
    const size_t F = b->n_pairs, K1 = b->total_kp1, K2 = b->total_kp2;
    if (F == 0) return ORB_OK;
    ORB_CHECK_ARG(n_found && (K1 == 0 || match12), "null output array");
    if ((rc = pj_check_offsets(b->n_pairs, b->kp1_begin, b->total_kp1, b->kp2_begin, b->total_kp2, true,
                               "kp1_begin / kp2_begin must start at 0 and end at total_kp1 / total_kp2",
                               PJ_KEYFRAME_LIMIT_MSG)))
        return rc;
    orbm_sim3_batch d = *b;
    Mirror io;
    sim3_mirror(io, d);
    io.add(match12, K1, false, true); io.add(match1, K1, false, true); io.add(match2, K2, false, true);
    io.add(n_found, F, false, true);
    return run_host(g_pj, device, io, [&] { return orbm_search_by_sim3_device(&d, match12, match1, match2, n_found, nullptr); });
}
