// LocalBA, the blocked LDL^T solve of the reduced camera system (in LDS, or in HBM for D > 128) and the
// pose update.
#pragma once

#include "ldlt_blocked.h"
#include "ldlt_grid.h"
#include "orbba_dev.h"

namespace orbamd {

#ifdef ORB_BA_STAMPS
__device__ unsigned long long g_ba_stamps[64];
#define BA_STAMP(k)                                                                              \
    do {                                                                                         \
        if (threadIdx.x == 0 && (k) < 64) g_ba_stamps[(k)] = __builtin_amdgcn_s_memtime();       \
    } while (0)
#define BA_STAMPW(k)                                                                             \
    do {                                                                                         \
        if ((threadIdx.x & 63) == 0 && (k) < 64) g_ba_stamps[(k)] = __builtin_amdgcn_s_memtime(); \
    } while (0)
#else
#define BA_STAMP(k) do {} while (0)
#define BA_STAMPW(k) do {} while (0)
#endif

// A_ik -= sum_j U_ij dinv_j U_kj for the NBK x NBK lower block-triangle below block J.
template <int NBK>
__device__ __forceinline__ void trailing_update(double* A, const double* dinv, int ld, int J0, int R0, int tid) {
    const int ty = tid >> 4, tx = tid & 15;
    double acc[NBK][NBK];
#pragma unroll
    for (int a = 0; a < NBK; a++)
#pragma unroll
        for (int c = 0; c < NBK; c++) acc[a][c] = 0;
    const double* wrow = A + (R0 + ty) * ld + J0;
    const double* lrow = A + (R0 + tx) * ld + J0;
#pragma unroll 4
    for (int j = 0; j < SB; j++) {
        const double dj = dinv[J0 + j];
        double wi[NBK], lk[NBK];
#pragma unroll
        for (int a = 0; a < NBK; a++) {
            wi[a] = wrow[SB * a * ld + j];
            lk[a] = lrow[SB * a * ld + j] * dj;
        }
#pragma unroll
        for (int a = 0; a < NBK; a++)
#pragma unroll
            for (int c = 0; c <= a; c++) acc[a][c] = fma(wi[a], lk[c], acc[a][c]);
    }
#pragma unroll
    for (int a = 0; a < NBK; a++)
#pragma unroll
        for (int c = 0; c <= a; c++) A[(R0 + ty + SB * a) * ld + R0 + tx + SB * c] -= acc[a][c];
}

// Schedule per block J (one barrier each after the panel and after the trailing step):
//   panel J (all waves) | wavefront 0: trailing tile (J+1, J+1), then the diagonal block J+1
//   (lookahead), while wavefronts 1-3 update every other trailing tile.
// Back substitution runs on wavefront 0 alone: x_J = Linv_JJ^T t_J, then t_c -= sum_i L_ic x_i for
// all earlier columns c (right-looking), block by block from the last.
// NT threads (round 6: 1024 by default, ORBBA_SOLVE_THREADS=256 the round-5 form): wavefront 0 as
// above; the other NT/64 - 1 wavefronts load S, take the panels and the trailing tiles -- with 15 of
// them instead of 3, the lookahead phase of an early block (up to 28 trailing tiles) no longer
// outlasts wavefront 0's diagonal factorisation.  The trailing tiles go to the wavefronts that do
// not share wavefront 0's SIMD first (waves w with w % 4 != 0; a workgroup's waves are dealt to the
// SIMDs in turn), so the diagonal chain keeps its SIMD's issue slots.
// S's entries (r, c), (r, c + 1) (c even: one pose block) from the Schur-block part matrices, summed
// as schur_block_count_in forms them for the global solve: part 0 (+ the pose's Hpp part + lambda I on a
// diagonal block), then parts 1 .. (round 6: S is no longer assembled in HBM by a last-arriving
// workgroup, whose agent-scope release cost ba_schur_block_kernel ~4.5 us per trial).
__device__ __forceinline__ double2 s_piece(const BADev& b, int D, int r, int c, double lam) {
    const int i1 = r / 6, rr = r - 6 * i1, i2 = c / 6, cc = c - 6 * i2;
    const long long pstride = (long long)D * D;
    const double* p = b.Spart + (long long)r * D + c;
    // Branch-free, so every piece's loads are in flight together: the Hpp matrix is zero off the
    // diagonal pose blocks, and adding +0 there changes nothing (at most -0 -> +0 in pk, which v = 0 + pk
    // turns into +0 anyway).
    const bool dg = i1 == i2;
    const double2 h = *reinterpret_cast<const double2*>(p + SB_SPLIT * pstride);
    double2 v = make_double2(0.0, 0.0);
#pragma unroll
    for (int k = 0; k < SB_SPLIT; k++) {
        double2 pk = *reinterpret_cast<const double2*>(p + k * pstride);
        if (k == 0) {
            pk.x = (pk.x + h.x) + (dg && rr == cc ? lam : 0.0);
            pk.y = (pk.y + h.y) + (dg && rr == cc + 1 ? lam : 0.0);
        }
        v.x += pk.x;
        v.y += pk.y;
    }
    return v;
}

template <int NT>
__global__ __launch_bounds__(NT) void ba_solve_kernel(BADev b, int D, int simd0_helpers) {
    BA_RETURN_IF_DONE(b);
    constexpr int NW = NT / 64;
    extern __shared__ __attribute__((aligned(16))) double A[];   // Dp x ld
    const int Dp = solve_dp(D), ld = Dp + 1;
    double* y = A + (size_t)Dp * ld;   // rhs -> z -> D^-1 z -> x
    double* dinv = y + Dp;
    double* vz = dinv + Dp;
    __shared__ int s_ok;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int col = lane & 15, kq = lane >> 4;
    BA_STAMP(41);
    // the rhs first: its load is in flight with S's
    const double bs_v = tid < D ? b.bs[tid] : 0.0;   // D <= 128 < blockDim
    const double lam = b.ctl->lambda;
    // S -> LDS, only its lower block triangle (row r: columns up to the end of its 16-column block):
    // the factorisation, the panels, the trailing updates and the back substitution read nothing
    // above the diagonal blocks, and the diagonal blocks' upper triangles receive Linv before they are
    // read.  Wavefront 0 stages block 0 (rows 0-15, with the identity padding of a system smaller
    // than one block) and factors it while wavefronts 1-3 load rows 16.. (the load is latency-bound:
    // 38 rows of 16-byte pieces in flight per lane, lane c = piece c of the row).  D = 6 np is even,
    // so every row of S starts 16-byte aligned.
    if (wv == 0) {
        double2 v[2];
#pragma unroll
        for (int k = 0; k < 2; k++) {   // 16 rows x 8 pieces over 64 lanes
            const int p = lane + 64 * k, r = p >> 3, c = 2 * (p & 7);
            // loads from a clamped (in-bounds) position, unconditionally: no branch around them
            const double2 sv = s_piece(b, D, min(r, D - 1), min(c, D - 2), lam);
            v[k] = r < D && c < D ? sv : make_double2(r == c ? 1.0 : 0.0, r == c + 1 ? 1.0 : 0.0);
        }
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int p = lane + 64 * k, r = p >> 3, c = 2 * (p & 7);
            A[r * ld + c] = v[k].x;
            A[r * ld + c + 1] = v[k].y;
        }
        if (lane < Dp) y[lane] = bs_v;
        if (lane == 0) s_ok = 1;
        wave_lds_sync();
        BA_STAMPW(0);
        if (!solve_diag_block(A, y, dinv, vz, ld, 0, lane, D) && lane == 0) s_ok = 0;
    } else {
        constexpr int RQ = (128 - SB + NW - 2) / (NW - 1);   // rows per wavefront: (NW-1) x RQ >= 128 - 16
        const int r0 = SB + wv - 1;
        double2 v[RQ];
#pragma unroll
        for (int q = 0; q < RQ; q++) {
            const int r = min(r0 + (NW - 1) * q, D - 1);
            const int npr = min(D, (r & ~(SB - 1)) + SB) >> 1;   // pieces up to the block's end
            const double2 sv = s_piece(b, D, r, min(2 * lane, D - 2), lam);   // r is clamped above
            v[q] = r0 + (NW - 1) * q < D && lane < npr ? sv : make_double2(0.0, 0.0);
        }
#pragma unroll
        for (int q = 0; q < RQ; q++) {
            const int r = r0 + (NW - 1) * q;
            const int npr = min(D, (r & ~(SB - 1)) + SB) >> 1;
            if (r < D && lane < npr) {
                A[r * ld + 2 * lane] = v[q].x;
                A[r * ld + 2 * lane + 1] = v[q].y;
            }
        }
        // identity padding of rows 16.. (no divisions): columns D..Dp-1 of every row, then rows
        // D..Dp-1; a thread per (row group, column) of each
        const int t = tid - 64, npad = Dp - D;
        for (int r = SB + t / 16; r < Dp; r += (NT - 64) / 16)
            if ((t & 15) < npad) A[r * ld + D + (t & 15)] = r == D + (t & 15) ? 1.0 : 0.0;
        for (int r = max(D, SB) + t / 64; r < Dp; r += NW - 1)
            for (int c = lane; c < D; c += 64) A[r * ld + c] = 0.0;
        if (tid < Dp) y[tid] = bs_v;
    }
    __syncthreads();
    for (int J0 = 0; J0 < Dp && s_ok; J0 += SB) {
        const int R0 = J0 + SB;
        const int nbk = (Dp - R0) / SB;
        BA_STAMP(1 + 3 * (J0 / SB));
        if (nbk == 0) break;
        // (2) panel U_I = A_IJ Linv^T per 16-row tile (MFMA); rhs y_i -= A_iJ v with v = Linv^T D^-1 z_J
        if (wv < nbk) {
            double binv[4], bvz[4];
#pragma unroll
            for (int s2 = 0; s2 < 4; s2++) {
                const int k = 4 * s2 + kq;
                const double v = A[(J0 + min(k, col)) * ld + J0 + max(k, col)];
                binv[s2] = col > k ? v : (col == k ? 1.0 : 0.0);
            }
#pragma unroll
            for (int s2 = 0; s2 < 4; s2++) bvz[s2] = col == 0 ? vz[J0 + 4 * s2 + kq] : 0.0;   // B = [v | 0]
            for (int t = wv; t < nbk; t += NW) {
                const int i0 = R0 + SB * t;
                double av[4];
#pragma unroll
                for (int s2 = 0; s2 < 4; s2++) av[s2] = A[(i0 + col) * ld + J0 + 4 * s2 + kq];
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
                    A[row * ld + J0 + col] = u[r2];
                    if (col == 0) y[row] -= uy[r2];
                }
            }
        }
        __syncthreads();
        BA_STAMP(2 + 3 * (J0 / SB));
        // (3) trailing update with lookahead
        {
            double dk[4];
#pragma unroll
            for (int s2 = 0; s2 < 4; s2++) dk[s2] = dinv[J0 + 4 * s2 + kq];
            if (wv == 0) {
                solve_trailing_tile(A, ld, J0, R0, R0, col, kq, dk);
                wave_lds_sync();
                if (J0 == 32) BA_STAMPW(44);
                if (!solve_diag_block(A, y, dinv, vz, ld, R0, lane, D - R0) && lane == 0) s_ok = 0;
                if (J0 == 32) BA_STAMPW(45);
            } else {
                const int ntile = nbk * (nbk + 1) / 2;
                // helper h: the waves off wavefront 0's SIMD first (w % 4 != 0), then its SIMD-mates
                // (simd0_helpers = 0: wavefront 0's SIMD-mates take no tiles at all when there are enough
                // other helpers, so the diagonal chain has its SIMD to itself)
                constexpr int NOFF = NW - NW / 4;   // helpers off SIMD 0
                const int NH = (simd0_helpers || NOFF == 0) ? NW - 1 : NOFF;
                const int h = (wv & 3) ? (wv >> 2) * 3 + (wv & 3) - 1 : NOFF + (wv >> 2) - 1;
                for (int t = 1 + h; h < NH && t < ntile; t += NH) {   // tile 0 = (J+1, J+1) belongs to wavefront 0
                    int I = 0;
                    while ((I + 1) * (I + 2) / 2 <= t) I++;
                    const int K = t - I * (I + 1) / 2;
                    solve_trailing_tile(A, ld, J0, R0 + SB * I, R0 + SB * K, col, kq, dk);
                }
                if (J0 == 32) BA_STAMPW(45 + wv);
            }
        }
        __syncthreads();
        BA_STAMP(3 + 3 * (J0 / SB));
    }
    const int ok = s_ok;
    // pose state for the update at the end, loaded now so its latency hides behind the back
    // substitution (loaded at the kernel start, it was live across the factorisation: with S staged
    // from the part matrices that spilled it to scratch, each load then waited for in turn)
    double q_pre[4] = {0, 0, 0, 0}, t_pre[3] = {0, 0, 0}, bp_pre[6] = {0, 0, 0, 0, 0, 0};
    if (tid < b.np) {
        const int id = b.ps_id[tid];
        for (int j = 0; j < 4; j++) q_pre[j] = b.q[4 * id + j];
        for (int j = 0; j < 3; j++) t_pre[j] = b.t[3 * id + j];
        for (int j = 0; j < 6; j++) bp_pre[j] = b.bp[6 * tid + j];
    }
    if (ok) {   // back substitution, block by block from the last: x_J on wavefront 0, then every
                // earlier column's update (one thread per column) on the whole workgroup
        for (int i = tid; i < Dp; i += blockDim.x) y[i] *= dinv[i];   // t = D^-1 z
        __syncthreads();
        for (int J0 = Dp - SB; J0 >= 0; J0 -= SB) {
            if (wv == 0) {
                // x_J = Linv_JJ^T t_J: x_c = t_c + sum_{j>c} Linv[j][c] t_j (four partial sums)
                double xp[4] = {y[J0 + col], 0, 0, 0};
#pragma unroll
                for (int j = 1; j < SB; j++) {
                    const double lv = A[(J0 + min(col, j)) * ld + J0 + j];   // Linv[j][col] for j > col
                    xp[j & 3] = fma(j > col ? lv : 0.0, y[J0 + j], xp[j & 3]);   // select, not a branch
                }
                const double xc = (xp[0] + xp[1]) + (xp[2] + xp[3]);
                wave_lds_sync();
                if (lane < SB) y[J0 + col] = xc;
            }
            __syncthreads();
            // t_c -= sum_{i in J} L_ic x_i, L_ic = U_ic dinv_c, for all earlier columns c < J0
            for (int c = tid; c < J0; c += blockDim.x) {
                double sp[4] = {0, 0, 0, 0};
#pragma unroll
                for (int k = 0; k < SB; k++) sp[k & 3] = fma(A[(J0 + k) * ld + c], y[J0 + k], sp[k & 3]);
                y[c] = fma(-((sp[0] + sp[1]) + (sp[2] + sp[3])), dinv[c], y[c]);
            }
            __syncthreads();
        }
    }
    __syncthreads();
    BA_STAMP(40);
    for (int i = tid; i < D; i += blockDim.x) b.x[i] = ok ? y[i] : 0.0;
    if (tid == 0) b.ctl->ok2 = ok;
    __syncthreads();
    // push() + oplus for the free poses, scale terms x.(lambda x + b) (lam: read at the start)
    if (tid < b.np) {   // np <= 21 < blockDim
        const int i = tid;
        const int id = b.ps_id[i];
        double xi[6], part = 0;
        for (int j = 0; j < 6; j++) {
            xi[j] = ok ? y[6 * i + j] : 0.0;
            part += xi[j] * (lam * xi[j] + bp_pre[j]);
        }
        b.part[b.nl + i] = part;
        for (int j = 0; j < 4; j++) b.q_sv[4 * id + j] = q_pre[j];
        for (int j = 0; j < 3; j++) b.t_sv[3 * id + j] = t_pre[j];
        se3_exp_update(xi, q_pre, t_pre);
        for (int j = 0; j < 4; j++) b.q[4 * id + j] = q_pre[j];
        for (int j = 0; j < 3; j++) b.t[3 * id + j] = t_pre[j];
    }
    BA_STAMP(42);
}

// The same blocked LDL^T for reduced systems too large for LDS (more than 21 free keyframes, D > 128;
// the reference's window is every covisible keyframe, Optimizer.cc:494-504, with no upper bound).
// The padded system lives in HBM / L2 (b.Sg, row stride Dp+1); y, D^-1 and the forward-substitution
// vector stay in LDS.  One 1024-thread workgroup (16 wavefronts), per block J:
//   (1) wavefronts 0 / 1 factor the 16x16 diagonal block and form its inverse in an LDS copy (the
//       same concurrent pair as the LDS kernel), then the block goes back to HBM (L below, Linv in
//       the upper triangle, as the LDS kernel keeps it);
//   (2) the panel U_iJ = A_iJ Linv^T and y_i -= U_iJ D^-1 z_J over all 16 wavefronts (MFMA);
//   (3) the trailing update A_IK -= U_IJ D_J^-1 U_KJ^T, one 16x16 tile per wavefront step (MFMA).
// Back substitution: x_J on wavefront 0, the updates of earlier rows over the whole workgroup.
// ~D^3/3 flops at a few hundred GFLOP/s (one CU): 0.1-1 ms per trial for 22-100 free keyframes.
__global__ __launch_bounds__(1024) void ba_solve_global_kernel(BADev b, int D) {
    BA_RETURN_IF_DONE(b);
    extern __shared__ __attribute__((aligned(16))) double ysh[];   // y | dinv | vz, Dp each
    __shared__ double Ad[SB * (SB + 1)];
    __shared__ int s_ok;
    const int Dp = solve_dp(D), ld = Dp + 1;
    double* A = b.Sg;
    double* y = ysh;
    double* dinv = y + Dp;
    double* vz = dinv + Dp;
    const int tid = threadIdx.x;
    for (long long u = tid; u < (long long)Dp * Dp; u += blockDim.x) {
        const int r = (int)(u / Dp), c = (int)(u % Dp);
        A[(long long)r * ld + c] = (r < D && c < D) ? b.S[(long long)r * D + c] : (r == c ? 1.0 : 0.0);
    }
    for (int i = tid; i < Dp; i += blockDim.x) y[i] = i < D ? b.bs[i] : 0.0;
    if (tid == 0) s_ok = 1;
    __syncthreads();
    const int ok = ldlt_hbm_solve(A, D, y, dinv, vz, Ad, &s_ok);
    for (int i = tid; i < D; i += blockDim.x) b.x[i] = ok ? y[i] : 0.0;
    if (tid == 0) b.ctl->ok2 = ok;
    const double lam = b.ctl->lambda;
    for (int i = tid; i < b.np; i += blockDim.x) {   // push() + oplus, scale terms x.(lambda x + b)
        const int id = b.ps_id[i];
        double q[4], t[3], xi[6], part = 0;
        for (int j = 0; j < 4; j++) q[j] = b.q[4 * id + j];
        for (int j = 0; j < 3; j++) t[j] = b.t[3 * id + j];
        for (int j = 0; j < 6; j++) {
            xi[j] = ok ? y[6 * i + j] : 0.0;
            part += xi[j] * (lam * xi[j] + b.bp[6 * i + j]);
        }
        b.part[b.nl + i] = part;
        for (int j = 0; j < 4; j++) b.q_sv[4 * id + j] = q[j];
        for (int j = 0; j < 3; j++) b.t_sv[3 * id + j] = t[j];
        se3_exp_update(xi, q, t);
        for (int j = 0; j < 4; j++) b.q[4 * id + j] = q[j];
        for (int j = 0; j < 3; j++) b.t[3 * id + j] = t[j];
    }
}

// The end of an LM trial's solve on the grid path: both substitutions on the factor ldlt_grid.h left, then what
// ba_solve_global_kernel does behind its own: x, ok2, push() + oplus of the free poses and their scale terms.
__global__ __launch_bounds__(1024) void ba_solve_grid_finish_kernel(BADev b, LdltGrid g, int D) {
    BA_RETURN_IF_DONE(b);
    extern __shared__ __attribute__((aligned(16))) double ysh[];
    const int tid = threadIdx.x;
    const int ok = *g.ok;
    if (ok) ldlt_grid_substitute(g, ysh);
    __syncthreads();
    const double* y = ysh;
    for (int i = tid; i < D; i += blockDim.x) b.x[i] = ok ? y[i] : 0.0;
    if (tid == 0) b.ctl->ok2 = ok;
    const double lam = b.ctl->lambda;
    for (int i = tid; i < b.np; i += blockDim.x) {
        const int id = b.ps_id[i];
        double q[4], t[3], xi[6], part = 0;
        for (int j = 0; j < 4; j++) q[j] = b.q[4 * id + j];
        for (int j = 0; j < 3; j++) t[j] = b.t[3 * id + j];
        for (int j = 0; j < 6; j++) {
            xi[j] = ok ? y[6 * i + j] : 0.0;
            part += xi[j] * (lam * xi[j] + b.bp[6 * i + j]);
        }
        b.part[b.nl + i] = part;
        for (int j = 0; j < 4; j++) b.q_sv[4 * id + j] = q[j];
        for (int j = 0; j < 3; j++) b.t_sv[3 * id + j] = t[j];
        se3_exp_update(xi, q, t);
        for (int j = 0; j < 4; j++) b.q[4 * id + j] = q[j];
        for (int j = 0; j < 3; j++) b.t[3 * id + j] = t[j];
    }
}

}  // namespace orbamd
