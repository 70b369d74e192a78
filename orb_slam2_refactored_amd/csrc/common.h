// Shared host/device helpers for the gfx950 ORB / LocalBA library.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>

#include "host_mirror.h"
#include "orbslam2_amd.h"

namespace orbamd {

// Thread-local error text behind orb_last_error().
void set_error(const std::string& msg);

#define ORB_HIP_TRY(expr)                                                                          \
    do {                                                                                           \
        hipError_t _e = (expr);                                                                    \
        if (_e != hipSuccess) {                                                                    \
            ::orbamd::set_error(std::string(#expr) + ": " + hipGetErrorString(_e));                \
            return ORB_EHIP;                                                                       \
        }                                                                                          \
    } while (0)

#define ORB_CHECK_ARG(cond, msg)                                                                   \
    do {                                                                                           \
        if (!(cond)) {                                                                             \
            ::orbamd::set_error(msg);                                                              \
            return ORB_EINVAL;                                                                     \
        }                                                                                          \
    } while (0)

// Device-side failure flags (written by kernels, read by the host after a sync).
enum DeviceFault : uint32_t {
    FAULT_NONE = 0,
    FAULT_QT_NODES = 1u << 0,     // quadtree node array capacity exceeded
    FAULT_QT_ROOT = 1u << 1,      // keypoint mapped outside the root nodes (CV_Assert :569)
    FAULT_CELL_CAP = 1u << 2,     // FAST cell slot overflow (cannot happen: strict NMS bound)
    FAULT_OUT_CAP = 1u << 3,      // per-level output capacity exceeded
    FAULT_BLOCK_SIZE = 1u << 4,   // a kernel launched with a block size other than the one it is written for
};

// Grow-only device buffer.
struct DevBuf {
    void* ptr = nullptr;
    size_t bytes = 0;
    int reserve(size_t need) {
        if (need <= bytes) return ORB_OK;
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
        hipError_t e = hipMalloc(&ptr, need);
        if (e != hipSuccess) {
            set_error(std::string("hipMalloc failed: ") + hipGetErrorString(e));
            return ORB_ENOMEM;
        }
        bytes = need;
        return ORB_OK;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
    template <class T>
    T* as() const { return reinterpret_cast<T*>(ptr); }
};

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

using orbamd_host::Carver;

// A module's per-thread device buffers: ws is the _device entries' workspace, io the slab the host entries stage in.
// Both are dropped when the thread moves to another device.
struct Scratch {
    DevBuf ws, io;
    int device = -1;
    int use_device(int dev) {
        if (device != dev) {
            ws.release();
            io.release();
            device_changed();
            device = dev;
        }
        return ORB_OK;
    }
    int use_current_device() {
        int dev = 0;
        ORB_HIP_TRY(hipGetDevice(&dev));
        return use_device(dev);
    }

protected:
    virtual void device_changed() {}   // what else a module keeps on the device
};

// host_mirror.h's plan with synchronous HIP copies.
struct Mirror : orbamd_host::Mirror {
    Mirror() : orbamd_host::Mirror(to_device, to_host) {}
    static int to_device(void* dst, const void* src, size_t bytes) {
        ORB_HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
        return ORB_OK;
    }
    static int to_host(void* dst, const void* src, size_t bytes) {
        ORB_HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
        return ORB_OK;
    }
};

// The tail of every host entry, after its checks: the fields m holds are staged in s.io, device_call() runs the _device
// entry on the null stream with the re-bound arguments, and the outputs come back after one synchronisation.
template <class Fn>
int run_host(Scratch& s, int device, Mirror& m, Fn device_call) {
    ORB_HIP_TRY(hipSetDevice(device));
    int rc;
    if ((rc = s.use_device(device))) return rc;
    if ((rc = m.upload(s.io))) return rc;
    if ((rc = device_call())) return rc;
    ORB_HIP_TRY(hipStreamSynchronize(nullptr));
    return m.download();
}

// CSR offsets off[0 .. n]: start at 0, do not decrease, end at n_obs at most.
inline int check_csr(const int32_t* off, int n, int n_obs, const char* what) {
    ORB_CHECK_ARG(off[0] == 0, std::string(what) + ": offsets must start at 0");
    for (int i = 0; i < n; i++) ORB_CHECK_ARG(off[i + 1] >= off[i], std::string(what) + ": offsets must not decrease");
    ORB_CHECK_ARG(off[n] <= n_obs, std::string(what) + ": offsets end past n_obs");
    return ORB_OK;
}

// a[0 .. n) in [lo, hi)
inline int check_range(const int32_t* a, size_t n, int lo, int hi, const char* msg) {
    for (size_t i = 0; i < n; i++) ORB_CHECK_ARG(a[i] >= lo && a[i] < hi, msg);
    return ORB_OK;
}

}  // namespace orbamd
