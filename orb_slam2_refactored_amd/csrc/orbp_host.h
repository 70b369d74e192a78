// The host side every projection entry shares (included by orbp.hip after orbp_grid.h): the per-thread
// scratch with its workspace and upload helpers, and the batch checks.
#pragma once

namespace orbamd {

using orbamd_host::Carver;

template <class T>
static void pj_set_ptr(void* dst, char* p) { *static_cast<T**>(dst) = reinterpret_cast<T*>(p); }

// One array of a host batch: n elements at src, copied to the device; *dst becomes the copy's address
// (null when src is null: an optional array stays absent).
struct PjIn {
    const void* src;
    size_t bytes;
    void* dst;                    // the address of the pointer to set, and the setter that knows its type
    void (*set)(void*, char*);
    template <class T>
    PjIn(const T* s, size_t n, const T*& d) : src(s), bytes(n * sizeof(T)), dst(&d), set(&pj_set_ptr<const T>) {}
    template <class T>
    PjIn(const T* s, size_t n, T*& d) : src(s), bytes(n * sizeof(T)), dst(&d), set(&pj_set_ptr<T>) {}
};
// One output array of n elements on the device, behind the inputs.
struct PjOut {
    size_t bytes;
    void* dst;
    void (*set)(void*, char*);
    template <class T>
    PjOut(size_t n, T*& d) : bytes(n * sizeof(T)), dst(&d), set(&pj_set_ptr<T>) {}
};

struct PjScratch {
    DevBuf ws, io;
    int device = -1;

    void use_device(int dev) {
        if (device != dev) {
            ws.release();
            io.release();
            device = dev;
        }
    }
    int use_current_device() {
        int dev = 0;
        ORB_HIP_TRY(hipGetDevice(&dev));
        use_device(dev);
        return ORB_OK;
    }

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

    // A host batch into `io` with one reserve: the non-null inputs copied in order, then room for the
    // outputs.  The callers pass the fields of a copy of the batch struct as dst, so that copy becomes the
    // device entry's argument.
    int upload(std::initializer_list<PjIn> in, std::initializer_list<PjOut> out) {
        Carver dry{nullptr};
        char* p;
        for (const PjIn& i : in) dry.take(p, i.bytes);
        for (const PjOut& o : out) dry.take(p, o.bytes);
        int rc;
        if ((rc = io.reserve(dry.off))) return rc;
        Carver c{io.as<char>()};
        for (const PjIn& i : in) {
            c.take(p, i.bytes);
            if (!i.src) p = nullptr;
            if (p && i.bytes) ORB_HIP_TRY(hipMemcpy(p, i.src, i.bytes, hipMemcpyHostToDevice));
            i.set(i.dst, p);
        }
        for (const PjOut& o : out) {
            c.take(p, o.bytes);
            o.set(o.dst, p);
        }
        return ORB_OK;
    }
};

// n elements of an output back to the host (a null host array is one the caller did not ask for)
template <class T>
static int pj_download(T* host, const T* dev, size_t n) {
    if (host && n) ORB_HIP_TRY(hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost));
    return ORB_OK;
}

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
