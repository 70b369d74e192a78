// orbgba.hip — the map update behind a global bundle adjustment on gfx950 (GlobalBA::_Run, LoopClosing.cc:392-446;
// the arithmetic in gba_update.h).
//
// Two launches, whatever the spanning tree's depth:
//   gba_walk_kernel    one workgroup walks the tree from the origins level by level.  A child's TcwGBA depends on
//                      its parent's alone and every GetPose() of the walk reads the pose from before the update, so
//                      the level order gives the reference's queue order bit for bit: the poses are left alone
//                      during the walk and every visited keyframe gets bef = pose, pose = TcwGBA after it.  A
//                      wavefront takes a keyframe of the level, its lanes the children.
//   gba_points_kernel  one lane per map point, reading the flags and poses the walk left.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.h"
#include "gba_update.h"

namespace orbamd {

struct GbaDev {
    int K, M, n_origins;
    const int32_t* origins;
    const int32_t* child_off;
    const int32_t* child_idx;
    uint8_t* in_gba;
    float* pose;
    float* pose_gba;
    float* pose_bef;
    const uint8_t* mp_bad;
    const uint8_t* mp_in_gba;
    const float* mp_pos_gba;
    const int32_t* mp_ref_kf;
    float* mp_xw;
    // workspace: K ints each
    int* visited;
    int* front[2];
};

constexpr int GBA_WALK_THREADS = 1024;

// A slot enters a level once (its `visited` word is claimed by compare-and-swap), so a level list never holds
// more than K slots and the walk ends within K levels, whatever the tables hold; indices out of range are skipped.
__global__ __launch_bounds__(GBA_WALK_THREADS) void gba_walk_kernel(GbaDev g) {
    __shared__ int s_n[2];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    constexpr int WAVES = GBA_WALK_THREADS / 64;
    for (int k = tid; k < g.K; k += GBA_WALK_THREADS) g.visited[k] = 0;
    if (tid == 0) s_n[0] = s_n[1] = 0;
    __syncthreads();
    for (int i = tid; i < g.n_origins; i += GBA_WALK_THREADS) {
        const int o = g.origins[i];
        if (o >= 0 && o < g.K && atomicCAS(&g.visited[o], 0, 1) == 0) g.front[0][atomicAdd(&s_n[0], 1)] = o;
    }
    __syncthreads();
    const int total = g.child_idx ? max(g.child_off[g.K], 0) : 0;   // (no list: no keyframe has a child)
    int cur = 0;
    for (int level = 0; level < g.K; level++) {
        const int n = s_n[cur];
        __syncthreads();
        if (n == 0) break;
        if (tid == 0) s_n[cur ^ 1] = 0;
        __syncthreads();
        for (int fi = wave; fi < n; fi += WAVES) {
            const int f = g.front[cur][fi];
            const int beg = min(max(g.child_off[f], 0), total);
            const int end = min(max(g.child_off[f + 1], beg), total);
            for (int u = beg + lane; u < end; u += 64) {
                const int c = g.child_idx[u];
                if (c < 0 || c >= g.K) continue;
                if (atomicCAS(&g.visited[c], 0, 1) != 0) continue;
                if (!g.in_gba[c]) {
                    float T[12];
                    gba_child_pose(g.pose + 12 * c, g.pose + 12 * f, g.pose_gba + 12 * f, T);
                    for (int j = 0; j < 12; j++) g.pose_gba[12 * c + j] = T[j];
                    g.in_gba[c] = 1;
                }
                g.front[cur ^ 1][atomicAdd(&s_n[cur ^ 1], 1)] = c;
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    __syncthreads();
    // TcwBefGBA = GetPose(); SetPose(TcwGBA) (:410-411) of every keyframe the walk reached
    for (int k = tid; k < g.K; k += GBA_WALK_THREADS) {
        if (!g.visited[k]) continue;
        for (int j = 0; j < 12; j++) {
            g.pose_bef[12 * k + j] = g.pose[12 * k + j];
            g.pose[12 * k + j] = g.pose_gba[12 * k + j];
        }
    }
}

__global__ __launch_bounds__(256) void gba_points_kernel(GbaDev g) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= g.M || g.mp_bad[p]) return;
    if (g.mp_in_gba[p]) {   // optimised by the adjustment: SetWorldPos(posGBA)
        for (int j = 0; j < 3; j++) g.mp_xw[3 * p + j] = g.mp_pos_gba[3 * p + j];
        return;
    }
    const int r = g.mp_ref_kf[p];
    if (r < 0 || r >= g.K || !g.in_gba[r]) return;
    float X[3], o[3];
    for (int j = 0; j < 3; j++) X[j] = g.mp_xw[3 * p + j];
    gba_move_point(g.pose_bef + 12 * r, g.pose + 12 * r, X, o);
    for (int j = 0; j < 3; j++) g.mp_xw[3 * p + j] = o[j];
}

namespace {

thread_local Scratch g_gba;

int gba_common(const orbba_gba_map* m) {
    ORB_CHECK_ARG(m, "null argument");
    ORB_CHECK_ARG(m->n_keyframes >= 0 && m->n_mappoints >= 0 && m->n_origins >= 0, "negative sizes");
    ORB_CHECK_ARG(m->n_origins == 0 || m->origins, "null origins");
    ORB_CHECK_ARG(m->kf_child_off, "null kf_child_off");
    ORB_CHECK_ARG(m->n_keyframes == 0 || (m->kf_in_gba && m->kf_pose && m->kf_pose_gba && m->kf_pose_bef),
                  "null keyframe array");
    ORB_CHECK_ARG(m->n_mappoints == 0 || (m->mp_bad && m->mp_in_gba && m->mp_pos_gba && m->mp_ref_kf && m->mp_xw),
                  "null map point array");
    return ORB_OK;
}

bool finite_n(const float* v, int n) {
    for (int k = 0; k < n; k++)
        if (!std::isfinite(v[k])) return false;
    return true;
}

// The host entry's checks of the tables' contents (the device entry cannot read them)
int gba_check_host(const orbba_gba_map* m) {
    const int K = m->n_keyframes, M = m->n_mappoints;
    ORB_CHECK_ARG(m->kf_child_off[0] == 0, "kf_child_off must start at 0");
    for (int k = 0; k < K; k++) ORB_CHECK_ARG(m->kf_child_off[k + 1] >= m->kf_child_off[k], "kf_child_off decreases");
    const int C = m->kf_child_off[K];
    ORB_CHECK_ARG(C == 0 || m->kf_child_idx, "null kf_child_idx");
    std::vector<uint8_t> seen(K, 0);   // 1: an origin, 2: a child
    for (int i = 0; i < m->n_origins; i++) {
        const int o = m->origins[i];
        ORB_CHECK_ARG(o >= 0 && o < K, "origin out of range");
        ORB_CHECK_ARG(!seen[o], "a slot is an origin twice");
        seen[o] = 1;
    }
    for (int u = 0; u < C; u++) {
        const int c = m->kf_child_idx[u];
        ORB_CHECK_ARG(c >= 0 && c < K, "child out of range");
        ORB_CHECK_ARG(seen[c] != 1, "a slot is both an origin and a child");
        ORB_CHECK_ARG(seen[c] != 2, "a slot is a child of two parents");
        seen[c] = 2;
    }
    for (int k = 0; k < K; k++) {
        ORB_CHECK_ARG(finite_n(m->kf_pose + 12 * k, 12), "non-finite pose");
        ORB_CHECK_ARG(!m->kf_in_gba[k] || finite_n(m->kf_pose_gba + 12 * k, 12), "non-finite TcwGBA");
    }
    for (int p = 0; p < M; p++) {
        if (m->mp_bad[p]) continue;
        if (m->mp_in_gba[p]) ORB_CHECK_ARG(finite_n(m->mp_pos_gba + 3 * p, 3), "non-finite posGBA");
        else ORB_CHECK_ARG(m->mp_ref_kf[p] >= 0 && m->mp_ref_kf[p] < K, "mp_ref_kf out of range");
    }
    return ORB_OK;
}

}  // namespace
}  // namespace orbamd

using namespace orbamd;

extern "C" int orbba_gba_update_map_device(const orbba_gba_map* m, void* stream) {
    int rc;
    if ((rc = gba_common(m))) return rc;
    const int K = m->n_keyframes, M = m->n_mappoints;
    if ((rc = g_gba.use_current_device())) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t kw = align_up(std::max<size_t>(K, 1) * 4, 256);
    if ((rc = g_gba.ws.reserve(3 * kw))) return rc;
    char* w = g_gba.ws.as<char>();
    GbaDev g{K, M, m->n_origins, m->origins, m->kf_child_off, m->kf_child_idx, m->kf_in_gba, m->kf_pose, m->kf_pose_gba,
             m->kf_pose_bef, m->mp_bad, m->mp_in_gba, m->mp_pos_gba, m->mp_ref_kf, m->mp_xw, (int*)w,
             {(int*)(w + kw), (int*)(w + 2 * kw)}};
    if (K) hipLaunchKernelGGL(gba_walk_kernel, dim3(1), dim3(GBA_WALK_THREADS), 0, st, g);
    if (M) hipLaunchKernelGGL(gba_points_kernel, dim3((M + 255) / 256), dim3(256), 0, st, g);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbba_gba_update_map(const orbba_gba_map* m, int device) {
    int rc;
    if ((rc = gba_common(m)) || (rc = gba_check_host(m))) return rc;   // the checks, before any device call
    const size_t K = m->n_keyframes, M = m->n_mappoints, C = m->kf_child_off[K];
    orbba_gba_map d = *m;
    Mirror io;
    io.add(d.origins, (size_t)m->n_origins, true, false); io.add(d.kf_child_off, K + 1, true, false);
    io.add(d.kf_child_idx, C, true, false); io.add(d.kf_in_gba, K, true, true); io.add(d.kf_pose, K * 12, true, true);
    io.add(d.kf_pose_gba, K * 12, true, true); io.add(d.kf_pose_bef, K * 12, true, true); io.add(d.mp_bad, M, true, false);
    io.add(d.mp_in_gba, M, true, false); io.add(d.mp_pos_gba, M * 3, true, false); io.add(d.mp_ref_kf, M, true, false);
    io.add(d.mp_xw, M * 3, true, true);
    return run_host(g_gba, device, io, [&] { return orbba_gba_update_map_device(&d, nullptr); });
}
