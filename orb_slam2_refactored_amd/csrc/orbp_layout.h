// The projection searches' workspace regions (orbp.hip), plain C++ so that a CPU test
// (tests/native/pj_layout_check.cpp) shares them.  As in ba_layout.h each region is one struct of typed
// pointers whose carve() takes its fields from a Carver in the order written there; a workspace is a
// sequence of regions on one Carver, and a Carver with a null base is the dry run for its byte count.
#pragma once
#include <cstddef>
#include <cstdint>

#include "carver.h"
#include "orbslam2_amd.h"

namespace orbamd_host {

constexpr int PJ_CELLS = ORBM_GRID_COLS * ORBM_GRID_ROWS;
#ifndef PJ_K_OVERRIDE
constexpr int PJ_K = 4;          // candidates kept per map point
#else
constexpr int PJ_K = PJ_K_OVERRIDE;   // diagnostic builds: K = 1 forces the rescan path
#endif
constexpr int PI_CAP = 128;      // SearchForInitialization: candidates kept per query

// The FeaturesGrid of every frame and the per-point arrays of the score and walk kernels.
struct PjGridLayout {
    int32_t* grid_idx;     // total_kp: frame-relative keypoint index at each sorted position
    int32_t* grid_start;   // n_frames x (PJ_CELLS + 1)
    int32_t* mp_cnt;       // total_mp
    int32_t* mp_frame;     // total_mp: frame of each map point (pj_grid_kernel)
    uint64_t* mp_top;      // total_mp x PJ_K: (key, index | level << 24), a uint2 on the device
    void carve(Carver& c, size_t n_frames, size_t total_kp, size_t total_mp) {
        c.take(grid_idx, total_kp); c.take(grid_start, n_frames * (PJ_CELLS + 1)); c.take(mp_cnt, total_mp);
        c.take(mp_frame, total_mp); c.take(mp_top, total_mp * PJ_K);
    }
};

// The motion walk's accepted pairs and a projection kernel's results (relocalisation, Fuse, the Sim3
// projection search), behind the grid region.
struct PjPointLayout {
    int32_t* choice;       // total_mp: accepted idx2 or -1
    uint8_t* out_valid;    // total_mp
    float* out_proj;       // total_mp x 3
    int32_t* out_level;    // total_mp
    void carve(Carver& c, size_t total_mp) {
        c.take(choice, total_mp); c.take(out_valid, total_mp); c.take(out_proj, 3 * total_mp);
        c.take(out_level, total_mp);
    }
};

// SearchForInitialization's candidate lists, behind the grid region.
struct PiLayout {
    int32_t* cnt;          // total_q
    uint32_t* cand;        // max(total_q, 1) x PI_CAP
    void carve(Carver& c, size_t total_q) {
        c.take(cnt, total_q); c.take(cand, std::max<size_t>(total_q, 1) * PI_CAP);
    }
};

// One keyframe side of SearchBySim3: its grid and its slots' projection results and matches.
struct Sim3SideLayout {
    int32_t* grid_idx;     // total
    int32_t* grid_start;   // n_pairs x (PJ_CELLS + 1)
    int32_t* pair;         // total
    int32_t* out_level;    // total
    int32_t* match;        // total
    uint8_t* out_valid;    // total
    float* out_uv;         // total x 2
    void carve(Carver& c, size_t n_pairs, size_t total) {
        c.take(grid_idx, total); c.take(grid_start, n_pairs * (PJ_CELLS + 1)); c.take(pair, total);
        c.take(out_level, total); c.take(match, total); c.take(out_valid, total); c.take(out_uv, 2 * total);
    }
};

}  // namespace orbamd_host
