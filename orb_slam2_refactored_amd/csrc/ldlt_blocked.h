// The blocked LDL^T shared by LocalBA's reduced camera system (orbba_solve.h) and OptimizeEssentialGraph's pose graph
// (orbeg.hip): the 16 x 16 diagonal block on one wavefront, the MFMA trailing tile, and the whole factorisation with
// both substitutions for a system held in HBM.  orbba_solve.h holds LocalBA's kernels around them.
#pragma once

#include <hip/hip_runtime.h>

namespace orbamd {

__device__ __forceinline__ double readlane_d(double v, int lane) {
    const long long u = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_readlane((int)(u & 0xffffffff), lane);
    const int hi = __builtin_amdgcn_readlane((int)(u >> 32), lane);
    return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// Reduced camera system solve + pose update: right-looking blocked LDL^T of the (6P)^2 system in
// LDS, padded with identity to Dp = 16*ceil(D/16) so every block is a full 16 columns (the padded
// unknowns solve to 0).  Row stride Dp+1 (odd) keeps column walks bank-conflict free.  The forward
// substitution is carried along; back substitution is blocked.  Per block J:
//   (1) wavefront 0: LDL^T of the 16x16 diagonal block in registers (lane i owns row i, pivot rows
//       broadcast with v_readlane, branch-free), z_J, and Linv_JJ = L_JJ^-1 (kept in the unused upper
//       triangle of the block: Linv[j][k] at (k, j));
//   (2) panel, one thread per row: U_iJ = A_iJ Linv_JJ^T (= L_iJ D_J) as independent dot products;
//       y_i -= L_iJ z_J;
//   (3) trailing A_ik -= U_iJ D_J^-1 U_kJ^T on the lower triangle: thread (ty, tx) of a 16x16 grid
//       owns rows R0+ty+16a, columns R0+tx+16c (c <= a), so a wavefront walks 16 consecutive rows.
constexpr int SB = 16;

__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

typedef double d4 __attribute__((ext_vector_type(4)));

__host__ __device__ constexpr int solve_dp(int D) { return (D + SB - 1) / SB * SB; }
__host__ __device__ constexpr size_t solve_lds_doubles(int D) {
    return (size_t)solve_dp(D) * (solve_dp(D) + 1) + 3 * (size_t)solve_dp(D);
}

#ifndef ORBBA_NEWTON
#define ORBBA_NEWTON 2
#endif
__device__ __forceinline__ double rcp_d(double d) {   // 1/d: v_rcp_f64 + ORBBA_NEWTON Newton steps
    double r = __builtin_amdgcn_rcp(d);
#pragma unroll
    for (int k = 0; k < ORBBA_NEWTON; k++) {
        const double e = fma(-d, r, 1.0);
        r = fma(r, e, r);
    }
    return r;
}

// v_fmac_f64 with src0 = lane J's value of each 16-lane row (DPP row_newbcast): r += bcast_J(r) * nl,
// and the plain broadcast.  The compiler's hazard recognizer does not look inside inline asm, so each
// statement carries the 2 wait states a DPP read needs after a VALU write of its source (s_nop 1);
// the code that uses them has no EXEC writes (no divergent branches), whose DPP hazard is 5 states.
// The statements are not volatile, so the scheduler may interleave independent ones.
template <int J>
__device__ __forceinline__ void fmac_bcast_t(double& r, double nl) {
    asm("s_nop 1\n\tv_fmac_f64_dpp %0, %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(r) : "v"(nl), "n"(J));
}
template <int J>
__device__ __forceinline__ double bcast_nop_t(double v) {
    double o;
    asm("s_nop 1\n\tv_mov_b64_dpp %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "=v"(o) : "v"(v), "n"(J));
    return o;
}
// j must fold to a constant after unrolling
__device__ __forceinline__ void fmac_bcast(double& r, double nl, int j) {
    switch (j) {
        case 0: fmac_bcast_t<0>(r, nl); break;
        case 1: fmac_bcast_t<1>(r, nl); break;
        case 2: fmac_bcast_t<2>(r, nl); break;
        case 3: fmac_bcast_t<3>(r, nl); break;
        case 4: fmac_bcast_t<4>(r, nl); break;
        case 5: fmac_bcast_t<5>(r, nl); break;
        case 6: fmac_bcast_t<6>(r, nl); break;
        case 7: fmac_bcast_t<7>(r, nl); break;
        case 8: fmac_bcast_t<8>(r, nl); break;
        case 9: fmac_bcast_t<9>(r, nl); break;
        case 10: fmac_bcast_t<10>(r, nl); break;
        case 11: fmac_bcast_t<11>(r, nl); break;
        case 12: fmac_bcast_t<12>(r, nl); break;
        case 13: fmac_bcast_t<13>(r, nl); break;
        case 14: fmac_bcast_t<14>(r, nl); break;
        default: fmac_bcast_t<15>(r, nl); break;
    }
}
__device__ __forceinline__ double bcast_nop(double v, int j) {
    switch (j) {
        case 0: return bcast_nop_t<0>(v);
        case 1: return bcast_nop_t<1>(v);
        case 2: return bcast_nop_t<2>(v);
        case 3: return bcast_nop_t<3>(v);
        case 4: return bcast_nop_t<4>(v);
        case 5: return bcast_nop_t<5>(v);
        case 6: return bcast_nop_t<6>(v);
        case 7: return bcast_nop_t<7>(v);
        case 8: return bcast_nop_t<8>(v);
        case 9: return bcast_nop_t<9>(v);
        case 10: return bcast_nop_t<10>(v);
        case 11: return bcast_nop_t<11>(v);
        case 12: return bcast_nop_t<12>(v);
        case 13: return bcast_nop_t<13>(v);
        case 14: return bcast_nop_t<14>(v);
        default: return bcast_nop_t<15>(v);
    }
}

// Diagonal block J0 of the blocked LDL^T on ONE wavefront, in registers: lane i (of every 16-lane
// row; the four rows hold the same copy of r and y) owns row i of the block (r), of Linv = L_JJ^-1 (x;
// 16-lane row q holds Linv's columns 4m + q, so a pivot updates j / 4 + 1 x registers instead of
// j + 1: 4.5k -> 3.7k ticks per block alone, tools/probe/diag_probe.hip) and the rhs entry y_i.  Pivot j: d_j and 1/d_j by a DPP broadcast + v_rcp_f64 and two Newton steps,
// nl_i = -L_ij (rows below the pivot, else 0), then fused broadcast-FMAs: the trailing columns
// r_k += nl * r_j[k], the forward substitution y_i += nl * z_j and the inverse rows
// x_i[c] += nl * x_j[c] (c <= j: row j of Linv is final after pivot j-1).  The next pivot's column is
// updated first, so its broadcast and reciprocal chain interleave with the rest of the step
// (ordered volatile asm from tools/gen_ba_diag.py: the in-order issue then hides the chain).
// Outputs: dinv_J, z_J (in y), Linv in the block's upper triangle (Linv[i][c] at (c, i), c < i) and
// vz_J = Linv^T D^-1 z_J; the lower triangle is not needed by the later steps.
__device__ __forceinline__ bool solve_diag_block(double* A, double* y, double* dinv, double* vz, int ld, int J0,
                                                 int lane, int nreal) {
    const int i = lane & (SB - 1);
    double r[SB], x[SB / 4];   // x[m]: Linv column 4m + q on the lanes of 16-lane row q
#pragma unroll
    for (int k = 0; k < SB; k++) r[k] = A[(J0 + max(i, k)) * ld + J0 + min(i, k)];
#pragma unroll
    for (int m = 0; m < SB / 4; m++) x[m] = 4 * m + (lane >> 4) == i ? 1.0 : 0.0;
    double yi = y[J0 + i];
    double rci = 1.0;   // 1/d_i (identity padding rows: d = 1)
    bool ok = true;
    double dj = bcast_nop(r[0], 0);
    double rc = rcp_d(dj);
    // 16 pivot steps, unrolled with the next pivot's broadcast + reciprocal interleaved into the
    // current step's broadcast-FMAs (tools/gen_ba_diag.py)
#ifndef ORBBA_DIAG_INC
#define ORBBA_DIAG_INC "orbba_diag.inc"
#endif
#include ORBBA_DIAG_INC
    if (lane < SB) {
        dinv[J0 + i] = rci;
        y[J0 + i] = yi;
    }
#pragma unroll
    for (int m = 0; m < SB / 4; m++) {   // every 16-lane row stores its Linv columns
        const int c = 4 * m + (lane >> 4);
        if (c < i) A[(J0 + c) * ld + J0 + i] = x[m];
    }
    wave_lds_sync();
    // v_c = sum_{j >= c} Linv[j][c] dinv_j z_j
    double v = dinv[J0 + i] * y[J0 + i];
#pragma unroll
    for (int j = 1; j < SB; j++) {
        const double lv = A[(J0 + min(i, j)) * ld + J0 + j];   // Linv[j][i] for j > i
        v = fma(j > i ? lv : 0.0, dinv[J0 + j] * y[J0 + j], v);
    }
    if (lane < SB) vz[J0 + i] = v;
    wave_lds_sync();
    return ok;
}

// One 16x16 tile of the trailing update: A[i0.., k0..] -= U_I D_J^-1 U_K^T (v_mfma_f64_16x16x4).
__device__ __forceinline__ void solve_trailing_tile(double* A, int ld, int J0, int i0, int k0, int col, int kq,
                                                    const double (&dk)[4]) {
    double av[4], bv[4];
#pragma unroll
    for (int s2 = 0; s2 < 4; s2++) {
        av[s2] = A[(i0 + col) * ld + J0 + 4 * s2 + kq];
        bv[s2] = A[(k0 + col) * ld + J0 + 4 * s2 + kq] * dk[s2];
    }
    d4 acc = {0, 0, 0, 0};
#pragma unroll
    for (int s2 = 0; s2 < 4; s2++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s2], bv[s2], acc, 0, 0, 0);
    const double u[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
    for (int r2 = 0; r2 < 4; r2++) A[(i0 + kq + 4 * r2) * ld + k0 + col] -= u[r2];
}

__device__ __forceinline__ void solve_trailing_tile_g(double* A, int ld, int J0, int i0, int k0, int col, int kq,
                                                      const double (&dk)[4]) {
    double av[4], bv[4];
#pragma unroll
    for (int s2 = 0; s2 < 4; s2++) {
        av[s2] = A[(long long)(i0 + col) * ld + J0 + 4 * s2 + kq];
        bv[s2] = A[(long long)(k0 + col) * ld + J0 + 4 * s2 + kq] * dk[s2];
    }
    d4 acc = {0, 0, 0, 0};
#pragma unroll
    for (int s2 = 0; s2 < 4; s2++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s2], bv[s2], acc, 0, 0, 0);
    const double u[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
    for (int r2 = 0; r2 < 4; r2++) A[(long long)(i0 + kq + 4 * r2) * ld + k0 + col] -= u[r2];
}

// The factorisation and both substitutions of LocalBA's HBM form (orbba_solve.h), for any caller that has staged the padded
// system: A (row stride Dp + 1, identity in rows and columns D .. Dp - 1) in HBM, the right-hand side in y,
// *s_ok = 1, and a barrier behind them.  y, dinv and vz are LDS arrays of Dp doubles, Ad one of SB * (SB + 1).  One
// 1024-thread workgroup; on return (after a barrier) y holds the solution if the result is nonzero.  A zero or
// non-finite pivot fails.  LocalBA's ba_solve_global_kernel and OptimizeEssentialGraph's eg_solve_kernel call it.
__device__ __forceinline__ int ldlt_hbm_solve(double* A, int D, double* y, double* dinv, double* vz, double* Ad,
                                              int* s_ok_p) {
    int& s_ok = *s_ok_p;
    const int Dp = solve_dp(D), ld = Dp + 1;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, NW = 16;
    const int col = lane & 15, kq = lane >> 4;
    for (int J0 = 0; J0 < Dp; J0 += SB) {
        const int R0 = J0 + SB;
        const int nbk = (Dp - R0) / SB;
        // (1) diagonal block in LDS; Av addresses it with the global (J0, J0) indexing of the helpers
        if (tid < SB * SB) Ad[(tid >> 4) * (SB + 1) + (tid & 15)] = A[(long long)(J0 + (tid >> 4)) * ld + J0 + (tid & 15)];
        __syncthreads();
        double* Av = Ad - ((long long)J0 * (SB + 1) + J0);
        if (wv == 0 && !solve_diag_block(Av, y, dinv, vz, SB + 1, J0, lane, D - J0) && lane == 0) s_ok = 0;
        __syncthreads();
        if (!s_ok) break;
        if (tid < SB * SB) A[(long long)(J0 + (tid >> 4)) * ld + J0 + (tid & 15)] = Ad[(tid >> 4) * (SB + 1) + (tid & 15)];
        if (nbk == 0) break;
        // (2) panel
        {
            double binv[4], bvz[4];
#pragma unroll
            for (int s2 = 0; s2 < 4; s2++) {
                const int k = 4 * s2 + kq;
                const double v = Ad[min(k, col) * (SB + 1) + max(k, col)];
                binv[s2] = col > k ? v : (col == k ? 1.0 : 0.0);
                bvz[s2] = col == 0 ? vz[J0 + 4 * s2 + kq] : 0.0;
            }
            for (int t = wv; t < nbk; t += NW) {
                const int i0 = R0 + SB * t;
                double av[4];
#pragma unroll
                for (int s2 = 0; s2 < 4; s2++) av[s2] = A[(long long)(i0 + col) * ld + J0 + 4 * s2 + kq];
                d4 acc = {0, 0, 0, 0}, accy = {0, 0, 0, 0};
#pragma unroll
                for (int s2 = 0; s2 < 4; s2++) {
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s2], binv[s2], acc, 0, 0, 0);
                    accy = __builtin_amdgcn_mfma_f64_16x16x4f64(av[s2], bvz[s2], accy, 0, 0, 0);
                }
                const double u[4] = {acc.x, acc.y, acc.z, acc.w};
                const double uy[4] = {accy.x, accy.y, accy.z, accy.w};
#pragma unroll
                for (int r2 = 0; r2 < 4; r2++) {
                    const int row = i0 + kq + 4 * r2;
                    A[(long long)row * ld + J0 + col] = u[r2];
                    if (col == 0) y[row] -= uy[r2];
                }
            }
        }
        __syncthreads();
        // (3) trailing update over the lower block triangle
        {
            double dk[4];
#pragma unroll
            for (int s2 = 0; s2 < 4; s2++) dk[s2] = dinv[J0 + 4 * s2 + kq];
            const int ntile = nbk * (nbk + 1) / 2;
            int I = 0, K = wv;   // tile t = I (I + 1) / 2 + K, walked with a stride of NW
            while (K > I) { K -= I + 1; I++; }
            for (int t = wv; t < ntile; t += NW) {
                solve_trailing_tile_g(A, ld, J0, R0 + SB * I, R0 + SB * K, col, kq, dk);
                K += NW;
                while (K > I) { K -= I + 1; I++; }
            }
        }
        __syncthreads();
    }
    __syncthreads();
    const int ok = s_ok;
    if (ok) {
        for (int i = tid; i < Dp; i += blockDim.x) y[i] *= dinv[i];   // t = D^-1 z
        __syncthreads();
        for (int J0 = Dp - SB; J0 >= 0; J0 -= SB) {
            if (wv == 0) {   // x_J = Linv_JJ^T t_J
                double xp[4] = {y[J0 + col], 0, 0, 0};
#pragma unroll
                for (int j = 1; j < SB; j++) {
                    const double lv = A[(long long)(J0 + min(col, j)) * ld + J0 + j];
                    xp[j & 3] = fma(j > col ? lv : 0.0, y[J0 + j], xp[j & 3]);
                }
                const double xc = (xp[0] + xp[1]) + (xp[2] + xp[3]);
                wave_lds_sync();
                if (lane < SB) y[J0 + col] = xc;
            }
            __syncthreads();
            double xj[SB];
#pragma unroll
            for (int k = 0; k < SB; k++) xj[k] = y[J0 + k];
            for (int c = tid; c < J0; c += blockDim.x) {
                double sp[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < SB; k++) sp[k & 3] = fma(A[(long long)(J0 + k) * ld + c], xj[k], sp[k & 3]);
                y[c] = fma(-((sp[0] + sp[1]) + (sp[2] + sp[3])), dinv[c], y[c]);
            }
            __syncthreads();
        }
    }
    return ok;
}

}  // namespace orbamd
