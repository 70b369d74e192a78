// The host side every projection entry shares (included by orbp.hip after orbp_grid.h): the per-thread
// scratch with its workspace helper, and the batch checks (the host entries stage with common.h's Mirror).
#pragma once

namespace orbamd {

struct PjScratch : Scratch {
    // The workspace of a call: carve(Carver&) takes every field; a dry run sizes the buffer, the second
    // run hands out the pointers.
    template <class Fn>
    int workspace(Fn&& carve) {
        Carver dry{nullptr};
        carve(dry);
        int rc;
        if ((rc = ws.reserve(dry.off))) return rc;
        Carver c{ws.as<char>()};
        carve(c);
        return ORB_OK;
    }
};

static void pj_bind(PjArgs& a, const orbamd_host::PjGridLayout& g) {
    a.grid_idx = g.grid_idx;
    a.grid_start = g.grid_start;
    a.mp_cnt = g.mp_cnt;
    a.mp_frame = g.mp_frame;
    a.mp_top = reinterpret_cast<uint2*>(g.mp_top);
}

// ---------------------------------------------------------------- batch checks
static int pj_check_sizes(int n, int total_a, int total_b) {
    ORB_CHECK_ARG(n >= 0 && total_a >= 0 && total_b >= 0, "negative sizes");
    return ORB_OK;
}

// scale[] / n_levels / th of a PjArgs or Sim3Args from the batch's pyramid (scale_factors is host memory)
template <class Args>
static int pj_set_pyramid(Args& a, int n_levels, const float* scale_factors, float th) {
    ORB_CHECK_ARG(n_levels >= 1 && n_levels <= PJ_MAX_LEVELS && scale_factors, "bad scale pyramid");
    a.n_levels = n_levels;
    for (int l = 0; l < n_levels; l++) a.scale[l] = scale_factors[l];
    a.th = th;
    return ORB_OK;
}

// The two offset arrays of a host batch: from 0 to the totals, non-decreasing, at most ORBM_PROJ_MAX_KP
// keypoints per frame in kp (and in other, when it holds keypoints too).
static int pj_check_offsets(int n, const int32_t* kp, int total_kp, const int32_t* other, int total_other,
                            bool limit_other, const char* ends_msg, const char* limit_msg) {
    ORB_CHECK_ARG(kp[0] == 0 && other[0] == 0 && kp[n] == total_kp && other[n] == total_other, ends_msg);
    for (int f = 0; f < n; f++) {
        ORB_CHECK_ARG(kp[f + 1] >= kp[f] && other[f + 1] >= other[f], "offsets must be non-decreasing");
        ORB_CHECK_ARG(kp[f + 1] - kp[f] <= PJ_MAXKP && (!limit_other || other[f + 1] - other[f] <= PJ_MAXKP), limit_msg);
    }
    return ORB_OK;
}
constexpr const char* PJ_ENDS_MSG = "kp_begin / mp_begin must start at 0 and end at total_kp / total_mp";
constexpr const char* PJ_FRAME_LIMIT_MSG = "frame has more than ORBM_PROJ_MAX_KP keypoints";
constexpr const char* PJ_KEYFRAME_LIMIT_MSG = "keyframe has more than ORBM_PROJ_MAX_KP keypoints";

}  // namespace orbamd
