// orbfr.hip — a Frame's arrays from extractor output on gfx950: UndistortKeyPoints, depth.convertTo + ComputeStereoFromRGBD,
// ComputeImageBounds and the split of cv::KeyPoint into the arrays orbtf_frames, orbtl_frames and the projection batches
// take, batched over frames (include/orbslam2_amd.h, "Frame construction").
//
// Reference: src/System.cc:153-174, :177-194, :197-219, called at :455, :464-465, :512-520, :570.  The per-element
// arithmetic is csrc/fr_undistort.h's.
//
// One kernel, one launch per batch:
//   fr_build_kernel   grid (ceil(kp_cap / 256), F), one thread per keypoint slot.  A thread below the clamped count reads
//                     its 28-byte record (seven dword loads per lane: a wavefront's 64 records are one contiguous 1792-byte
//                     run, so every fetched line is used in full), runs the five fp64 iterations (about 200 flops), reads one
//                     depth element and writes its row of every requested output.  Thread 0 of a frame's first workgroup
//                     also undistorts the four corners and writes bounds and frame_n; the first workgroup of the batch
//                     writes kp_begin.  What bounds it is memory traffic, not the fp64 work: 28 bytes in, up to 57 bytes
//                     out and one scattered depth sector per keypoint (DESIGN.md has the measured time).
//                     Staging a workgroup's records through LDS with coalesced dword loads measured 22 % slower (22.6 us
//                     against 18.5 us), so the per-lane loads stayed.
#include "common.h"
#include "fr_undistort.h"

namespace orbamd {

constexpr int FR_THREADS = 256;

__global__ __launch_bounds__(FR_THREADS) void fr_build_kernel(orbfr_input in, orbfr_frames o) {
    const int f = blockIdx.y, i = blockIdx.x * FR_THREADS + threadIdx.x;
    const int n = min(max(in.counts[f], 0), in.kp_cap);
    const float* cam = in.camera + 5 * (size_t)f;
    const float* dist = in.dist + 5 * (size_t)f;
    if (blockIdx.x == 0 && f == 0 && o.kp_begin)
        for (int q = threadIdx.x; q <= in.n_frames; q += FR_THREADS) o.kp_begin[q] = q * in.kp_cap;   // below 2^29
    if (i == 0) {
        if (o.frame_n) o.frame_n[f] = n;
        if (o.bounds) fr_image_bounds(in.rows, in.cols, cam, dist, o.bounds + 4 * (size_t)f);
    }
    if (i >= n) return;   // i < n <= kp_cap
    const size_t at = (size_t)f * in.kp_cap + i;
    orbx_keypoint kp = in.kps[at];
    float xy[2];
    fr_keypoint_xy(cam, dist, kp.x, kp.y, xy);
    if (in.mode != ORBFR_STEREO) {
        float ur = -1.f, dp = -1.f;
        int u, v;
        if (in.mode == ORBFR_RGBD && fr_pixel(kp.x, kp.y, in.rows, in.cols, u, v)) {
            const bool is_u16 = in.depth_type == ORBFR_DEPTH_U16;
            const uint8_t* e = static_cast<const uint8_t*>(in.depth) + (size_t)f * in.depth_frame_stride +
                               (size_t)v * in.depth_step + (size_t)u * (is_u16 ? 2 : 4);
            fr_rgbd(fr_depth_value(e, is_u16, in.depth_factor), xy[0], cam[4], ur, dp);
        }
        if (o.kp_uright) o.kp_uright[at] = ur;
        if (o.kp_depth) o.kp_depth[at] = dp;
    }
    if (o.kp_xy) {
        o.kp_xy[2 * at] = xy[0];
        o.kp_xy[2 * at + 1] = xy[1];
    }
    if (o.kp_octave) o.kp_octave[at] = kp.octave;
    if (o.kp_angle) o.kp_angle[at] = kp.angle;
    if (o.kp_un) {
        kp.x = xy[0];
        kp.y = xy[1];
        o.kp_un[at] = kp;
    }
    if (o.frame_mappoint) o.frame_mappoint[at] = -1;
    if (o.frame_outlier) o.frame_outlier[at] = 0;
}

}  // namespace orbamd

using namespace orbamd;

namespace {

thread_local Scratch g_fr;

size_t fr_elem(int32_t depth_type) { return depth_type == ORBFR_DEPTH_U16 ? 2 : 4; }

int fr_check(const orbfr_input* in, const orbfr_frames* o) {
    ORB_CHECK_ARG(in && o, "null input or frames");
    ORB_CHECK_ARG(in->n_frames >= 0, "negative n_frames");
    ORB_CHECK_ARG(in->n_frames < 65536, "65536 frames or more in one call");
    ORB_CHECK_ARG(in->kp_cap >= 1 && in->kp_cap <= ORBM_PROJ_MAX_KP, "kp_cap must be in [1, ORBM_PROJ_MAX_KP]");
    ORB_CHECK_ARG(in->rows >= 1 && in->cols >= 1, "rows and cols must be at least 1");
    ORB_CHECK_ARG(in->mode == ORBFR_MONO || in->mode == ORBFR_STEREO || in->mode == ORBFR_RGBD, "unknown mode");
    if (in->mode == ORBFR_RGBD) {
        ORB_CHECK_ARG(in->depth_type == ORBFR_DEPTH_U16 || in->depth_type == ORBFR_DEPTH_F32, "unknown depth type");
        const size_t e = fr_elem(in->depth_type);
        ORB_CHECK_ARG(in->depth_step >= (size_t)in->cols * e && in->depth_step % e == 0,
                      "depth_step must be at least cols elements and a multiple of the element size");
        ORB_CHECK_ARG(in->depth_frame_stride % e == 0, "depth_frame_stride must be a multiple of the element size");
        ORB_CHECK_ARG(in->n_frames <= 1 || in->depth_frame_stride >= (size_t)(in->rows - 1) * in->depth_step + (size_t)in->cols * e,
                      "depth_frame_stride is shorter than a frame");
    }
    if (in->n_frames == 0) return ORB_OK;
    ORB_CHECK_ARG(in->kps && in->counts && in->camera && in->dist, "null kps, counts, camera or dist");
    if (in->mode == ORBFR_RGBD) {
        ORB_CHECK_ARG(in->depth, "null depth in ORBFR_RGBD");
        ORB_CHECK_ARG((uintptr_t)in->depth % fr_elem(in->depth_type) == 0, "depth is not aligned to its element");
    }
    ORB_CHECK_ARG((uintptr_t)in->kps % 4 == 0, "kps is not aligned");
    return ORB_OK;
}

}  // namespace

extern "C" int orbfr_build_frames_device(const orbfr_input* in, const orbfr_frames* out, void* stream) {
    int rc;
    if ((rc = fr_check(in, out))) return rc;
    if (in->n_frames == 0) return ORB_OK;
    hipLaunchKernelGGL(fr_build_kernel, dim3((in->kp_cap + FR_THREADS - 1) / FR_THREADS, in->n_frames), dim3(FR_THREADS), 0,
                       (hipStream_t)stream, *in, *out);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbfr_build_frames(const orbfr_input* in, const orbfr_frames* out, int device) {
    int rc;
    if ((rc = fr_check(in, out))) return rc;
    if (in->n_frames == 0) return ORB_OK;
    const size_t F = in->n_frames, pc = in->kp_cap;
    for (size_t f = 0; f < F; f++)
        ORB_CHECK_ARG(in->counts[f] >= 0 && in->counts[f] <= in->kp_cap, "counts outside [0, kp_cap]");
    orbfr_input d = *in;
    orbfr_frames o = *out;
    const uint8_t* depth = in->mode == ORBFR_RGBD ? static_cast<const uint8_t*>(in->depth) : nullptr;
    Mirror io;
    io.add(d.kps, F * pc, true, false); io.add(d.counts, F, true, false); io.add(d.camera, F * 5, true, false);
    io.add(d.dist, F * 5, true, false);
    if (depth)
        io.add(depth, (F - 1) * in->depth_frame_stride + (size_t)(in->rows - 1) * in->depth_step + (size_t)in->cols * fr_elem(in->depth_type),
               true, false);
    // (the rows past the count go up too, so that they come back as the caller left them)
    io.add(o.frame_n, F, false, true); io.add(o.kp_xy, F * pc * 2, true, true); io.add(o.kp_octave, F * pc, true, true);
    io.add(o.kp_angle, F * pc, true, true); io.add(o.kp_un, F * pc, true, true); io.add(o.bounds, F * 4, false, true);
    io.add(o.frame_mappoint, F * pc, true, true); io.add(o.frame_outlier, F * pc, true, true); io.add(o.kp_begin, F + 1, false, true);
    if (in->mode != ORBFR_STEREO) { io.add(o.kp_uright, F * pc, true, true); io.add(o.kp_depth, F * pc, true, true); }
    return run_host(g_fr, device, io, [&] {
        d.depth = depth;
        return orbfr_build_frames_device(&d, &o, nullptr);
    });
}

extern "C" int orbfr_image_bounds(int32_t rows, int32_t cols, const float* camera, const float* dist, float* bounds) {
    ORB_CHECK_ARG(camera && dist && bounds, "null camera, dist or bounds");
    ORB_CHECK_ARG(rows >= 1 && cols >= 1, "rows and cols must be at least 1");
    fr_image_bounds(rows, cols, camera, dist, bounds);
    return ORB_OK;
}

extern "C" int orbfr_undistort_points(const float* camera, const float* dist, const float* xy, int32_t n, float* out) {
    ORB_CHECK_ARG(n >= 0, "negative n");
    ORB_CHECK_ARG(camera && dist && (n == 0 || (xy && out)), "null camera, dist, xy or out");
    for (int32_t i = 0; i < n; i++) {
        float r[2];
        fr_keypoint_xy(camera, dist, xy[2 * i], xy[2 * i + 1], r);   // (out may be xy)
        out[2 * i] = r[0];
        out[2 * i + 1] = r[1];
    }
    return ORB_OK;
}
