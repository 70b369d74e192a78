// A grid-wide LDL^T for a reduced camera system held in HBM (Optimizer::BundleAdjustment at map size: D = 6 x free
// keyframes up to 3072, where ldlt_hbm_solve's single workgroup leaves the other CUs idle).  Right-looking, blocked,
// the algebra of ldlt_blocked.h with a block width of GB = 32; the stream orders the launches and no workgroup ever
// waits for another.  Per block column J:
//   ldlt_grid_panel_kernel     every workgroup factors the 32 x 32 diagonal block in LDS (the same operations in the
//                              same order, so the same bits everywhere; workgroup 0 stores L_JJ and 1 / d_J beside the
//                              matrix, never into it: the others may still be reading the block), then takes 256
//                              rows below it, one per thread: U_iJ = A_iJ L_JJ^-T (= L_iJ D_J), in place
//   ldlt_grid_trailing_kernel  one workgroup per 32 x 32 tile of the lower block triangle, a wavefront per 16 x 16
//                              quarter: A_IK -= U_IJ D_J^-1 U_KJ^T by ldlt_blocked.h's f64 MFMA tile, twice (k = 32)
// then both substitutions on one workgroup (ldlt_grid_substitute: O(D^2)).  Every sum runs in a fixed order: two runs
// are bit-identical.  A zero or non-finite pivot clears *ok; the launches behind it run on (on garbage, within bounds).
// The matrix is padded with identity to Dg = 32 ceil(D / 32), row stride Dg + 1.
#pragma once

#include "ldlt_blocked.h"

namespace orbamd {

constexpr int GB = 32;

__host__ __device__ constexpr int grid_dp(int D) { return (D + GB - 1) / GB * GB; }
// doubles of the workspace: the padded matrix, the diagonal blocks' unit-lower factors, 1 / d, the right-hand side,
// and the ok word
__host__ __device__ constexpr size_t ldlt_grid_doubles(int D) {
    return (size_t)grid_dp(D) * (grid_dp(D) + 1) + (size_t)grid_dp(D) * GB + 2 * (size_t)grid_dp(D) + 8;
}

struct LdltGrid {
    double* A;      // Dg x (Dg + 1)
    double* Lm;     // Dg x GB: row r holds L[r][J0 .. r) of its diagonal block, zeros from the diagonal on
    double* dinv;   // Dg
    double* y;      // Dg: right-hand side in, solution out (ldlt_grid_solve_kernel)
    int* ok;
    int D, Dg, ld;
    const int* done;   // the caller's loop has ended: every kernel returns at once (or null)
};

inline LdltGrid ldlt_grid_carve(double* base, int D, const int* done) {
    LdltGrid g;
    g.D = D; g.Dg = grid_dp(D); g.ld = g.Dg + 1;
    g.A = base;
    g.Lm = g.A + (size_t)g.Dg * g.ld;
    g.dinv = g.Lm + (size_t)g.Dg * GB;
    g.y = g.dinv + g.Dg;
    g.ok = reinterpret_cast<int*>(g.y + g.Dg);
    g.done = done;
    return g;
}

// S (D x D, row-major) and its right-hand side into the padded workspace; *ok = 1
__global__ __launch_bounds__(256) void ldlt_grid_stage_kernel(LdltGrid g, const double* S, const double* rhs) {
    if (g.done && *g.done) return;
    const long long n = (long long)g.Dg * g.Dg;
    for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < n; u += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(u / g.Dg), c = (int)(u % g.Dg);
        g.A[(long long)r * g.ld + c] = (r < g.D && c < g.D) ? S[(long long)r * g.D + c] : (r == c ? 1.0 : 0.0);
        if (c == 0) g.y[r] = r < g.D ? rhs[r] : 0.0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *g.ok = 1;
}

__global__ __launch_bounds__(256) void ldlt_grid_panel_kernel(LdltGrid g, int J0) {
    if (g.done && *g.done) return;
    __shared__ double B[GB][GB + 1];    // the diagonal block: lower triangle, U = L D below the diagonal, d on it
    __shared__ double Lm[GB][GB + 1];   // L below the diagonal
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    for (int u = tid; u < GB * GB; u += 256) B[u / GB][u % GB] = g.A[(long long)(J0 + u / GB) * g.ld + J0 + u % GB];
    if (tid == 0) s_bad = 0;
    __syncthreads();
    for (int j = 0; j < GB; j++) {   // pivot j: column j is final; the columns behind it lose its outer product
        const double rj = 1.0 / B[j][j];
        for (int u = tid; u < GB * GB; u += 256) {
            const int i = u / GB, k = u % GB;
            if (k > j && k <= i) B[i][k] -= B[i][j] * (B[k][j] * rj);
        }
        __syncthreads();
    }
    if (tid < GB) {
        const double d = B[tid][tid];
        if (!(isfinite(d) && d != 0.0)) s_bad = 1;
    }
    for (int u = tid; u < GB * GB; u += 256) {
        const int i = u / GB, k = u % GB;
        Lm[i][k] = k < i ? B[i][k] * (1.0 / B[k][k]) : 0.0;
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        for (int u = tid; u < GB * GB; u += 256) g.Lm[(long long)(J0 + u / GB) * GB + u % GB] = Lm[u / GB][u % GB];
        if (tid < GB) g.dinv[J0 + tid] = 1.0 / B[tid][tid];
        if (tid == 0 && s_bad) *g.ok = 0;
    }
    // the panel: row r of U_J = A_rJ L_JJ^-T, u_c = a_c - sum_{k < c} u_k L[c][k]
    const int r = J0 + GB + blockIdx.x * 256 + tid;
    if (r >= g.Dg) return;
    double* a = g.A + (long long)r * g.ld + J0;
    double u[GB];
#pragma unroll
    for (int c = 0; c < GB; c++) {
        double s = a[c];
#pragma unroll
        for (int k = 0; k < c; k++) s -= u[k] * Lm[c][k];
        u[c] = s;
    }
#pragma unroll
    for (int c = 0; c < GB; c++) a[c] = u[c];
}

// tile t = I (I + 1) / 2 + K of the lower block triangle behind block column J0
__global__ __launch_bounds__(256) void ldlt_grid_trailing_kernel(LdltGrid g, int J0) {
    if (g.done && *g.done) return;
    const int t = blockIdx.x;
    int I = 0;
    while ((I + 1) * (I + 2) / 2 <= t) I++;
    const int K = t - I * (I + 1) / 2;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
    const int R0 = J0 + GB;
    const int i0 = R0 + GB * I + SB * (wv >> 1), k0 = R0 + GB * K + SB * (wv & 1);
    if (k0 > i0 || i0 + SB > g.Dg) return;   // (a diagonal tile's upper quarter is never read)
#pragma unroll
    for (int h = 0; h < GB / SB; h++) {
        double dk[4];
#pragma unroll
        for (int s2 = 0; s2 < 4; s2++) dk[s2] = g.dinv[J0 + SB * h + 4 * s2 + kq];
        solve_trailing_tile_g(g.A, g.ld, J0 + SB * h, i0, k0, col, kq, dk);
    }
}

// Both substitutions on one workgroup of any size: y (LDS, Dg doubles) <- g.y, then L z = y, t = D^-1 z, L^T x = t.
// L's off-diagonal blocks are U D^-1 from the matrix, its diagonal blocks g.Lm.  Ends with a barrier.
__device__ __forceinline__ void ldlt_grid_substitute(const LdltGrid& g, double* y) {
    const int tid = threadIdx.x, NT = blockDim.x, Dg = g.Dg;
    for (int i = tid; i < Dg; i += NT) y[i] = g.y[i];
    __syncthreads();
    for (int J0 = 0; J0 < Dg; J0 += GB) {
        for (int c = 0; c < GB - 1; c++) {
            if (tid < GB && tid > c) y[J0 + tid] -= g.Lm[(long long)(J0 + tid) * GB + c] * y[J0 + c];
            __syncthreads();
        }
        for (int r = J0 + GB + tid; r < Dg; r += NT) {
            const double* a = g.A + (long long)r * g.ld + J0;
            double s = 0;
            for (int c = 0; c < GB; c++) s += a[c] * (g.dinv[J0 + c] * y[J0 + c]);
            y[r] -= s;
        }
        __syncthreads();
    }
    for (int i = tid; i < Dg; i += NT) y[i] *= g.dinv[i];
    __syncthreads();
    for (int J0 = Dg - GB; J0 >= 0; J0 -= GB) {
        for (int c = GB - 1; c > 0; c--) {
            if (tid < c) y[J0 + tid] -= g.Lm[(long long)(J0 + c) * GB + tid] * y[J0 + c];
            __syncthreads();
        }
        for (int c = tid; c < J0; c += NT) {
            double s = 0;
            for (int k = 0; k < GB; k++) s += g.A[(long long)(J0 + k) * g.ld + c] * y[J0 + k];
            y[c] -= s * g.dinv[c];
        }
        __syncthreads();
    }
}

// the substitutions alone, the solution back into g.y (orbba_debug_ldlt_grid)
__global__ __launch_bounds__(1024) void ldlt_grid_solve_kernel(LdltGrid g) {
    extern __shared__ __attribute__((aligned(16))) double ysh[];
    if (!*g.ok) return;
    ldlt_grid_substitute(g, ysh);
    for (int i = threadIdx.x; i < g.Dg; i += blockDim.x) g.y[i] = ysh[i];
}

// the factorisation's launches: 2 per block column
inline void ldlt_grid_enqueue_factor(const LdltGrid& g, hipStream_t st) {
    for (int J0 = 0; J0 < g.Dg; J0 += GB) {
        const int rows = g.Dg - J0 - GB, nb = rows / GB;
        hipLaunchKernelGGL(ldlt_grid_panel_kernel, dim3(rows > 0 ? (rows + 255) / 256 : 1), dim3(256), 0, st, g, J0);
        if (nb) hipLaunchKernelGGL(ldlt_grid_trailing_kernel, dim3(nb * (nb + 1) / 2), dim3(256), 0, st, g, J0);
    }
}
inline void ldlt_grid_enqueue_stage(const LdltGrid& g, const double* S, const double* rhs, hipStream_t st) {
    const long long n = (long long)g.Dg * g.Dg;
    hipLaunchKernelGGL(ldlt_grid_stage_kernel, dim3((unsigned)std::min<long long>((n + 255) / 256, 4096)), dim3(256), 0, st, g,
                       S, rhs);
}

}  // namespace orbamd
