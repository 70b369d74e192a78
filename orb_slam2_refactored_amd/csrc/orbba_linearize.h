// LocalBA, linearisation: errors, Jacobians and quadratic forms per point, the pose sums, lambda's
// initial value and the points' Schur terms.
#pragma once

#include "orbba_dev.h"

namespace orbamd {

// BlockSolver::solve, landmark part (block_solver.hpp:377-419) for point l: every lane of the point's
// group forms D^-1 = (Hll + lambda I)^-1 (same values), each lane handles its edges'
// W = Hpl D^-1 and Hpl D^-1 b_l.  H / bl are the point's Hll / b_l (identical in every lane).
__device__ __forceinline__ void schur_point_terms(const BADev& b, int l, int sub, const double (&H)[9],
                                                  const double (&bl)[3], double lam) {
    double D[9], Di[9];
#pragma unroll
    for (int i = 0; i < 9; i++) D[i] = H[i];
    D[0] += lam; D[4] += lam; D[8] += lam;
    inv3(D, Di);
    if (sub == 0)
        for (int i = 0; i < 9; i++) b.Dinv[9 * l + i] = Di[i];
    double db[3];
#pragma unroll
    for (int i = 0; i < 3; i++) db[i] = Di[3 * i] * bl[0] + Di[3 * i + 1] * bl[1] + Di[3 * i + 2] * bl[2];
    for (int u = b.pt_beg[l] + sub; u < b.pt_beg[l + 1]; u += GRP) {
        const int4 rc = b.pt_rec[u];
        if (rc.w < 0) continue;
        const int k = rc.x;
        const double* Hpl = b.J + (long long)k * 72 + 54;
        double* W = b.W + (long long)k * 24;
        for (int r = 0; r < 6; r++) {
            for (int c = 0; c < 3; c++)
                W[3 * r + c] = Hpl[3 * r] * Di[c] + Hpl[3 * r + 1] * Di[3 + c] + Hpl[3 * r + 2] * Di[6 + c];
            W[18 + r] = Hpl[3 * r] * db[0] + Hpl[3 * r + 1] * db[1] + Hpl[3 * r + 2] * db[2];
        }
    }
}

// Per LM trial, point side.  On a linearising trial: errors + robust chi2 (computeActiveErrors /
// activeRobustChi2), linearizeOplus and constructQuadraticForm of every active edge
// (types_six_dof_expmap.cpp:103-139,188-234; base_binary_edge.hpp:54-120), Hll / b_l summed per
// point, pose parts stored per edge.  Then, once lambda is known (every trial but the very first of
// an optimize() call, whose lambda comes from computeLambdaInit), the point's Schur terms; a retry
// trial (rho < 0) does only those, with the new lambda.
__global__ __launch_bounds__(64) void ba_iter_kernel(BADev b) {
    if (b.ctl->done) return;
    const bool lin = b.ctl->need_lin != 0;
    const bool schur = !lin || b.ctl->it > 0;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int l = t / GRP, sub = t % GRP;
    const bool live = l < b.nl;
    double H[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, g[3] = {0, 0, 0}, chi = 0;
    if (!lin) {
        if (live) {
#pragma unroll
            for (int i = 0; i < 9; i++) H[i] = b.Hll[9 * l + i];
#pragma unroll
            for (int i = 0; i < 3; i++) g[i] = b.bl[3 * l + i];
            schur_point_terms(b, l, sub, H, g, b.ctl->lambda);
        }
        return;
    }
    if (live) {
        const double* Xl = b.X + 3 * b.pt_id[l];   // = X + 3 ep[e] for every edge of the point
        for (int u = b.pt_beg[l] + sub; u < b.pt_beg[l + 1]; u += GRP) {
            const int4 rc = b.pt_rec[u];
            const int k = rc.x, e = rc.y;
            if (b.level[e]) {   // a level-1 edge (second optimize()): no error, no terms -- its pose-side
                                // terms are zeros (written here: the call no longer clears J per optimize())
                if (rc.w >= 0) {
                    double* J = b.J + (long long)k * 72;
#pragma unroll
                    for (int i = 12; i < 72; i++) J[i] = 0.0;
                }
                continue;
            }
            const int pi = rc.z;
            const double* q4 = b.q + 4 * pi;
            double Xc[3], R[9];
            se3_map(q4, b.t + 3 * pi, Xl, Xc);
            chi += edge_error(b, e, Xc);
            q_to_R(q4, R);
            // Jacobians with one reciprocal of z (g2o divides by z / z^2 in every term; the
            // difference is rounding-level, within the LocalBA tolerance)
            const double x = Xc[0], y = Xc[1], z = Xc[2];
            const double iz = 1.0 / z, iz2 = iz * iz;
            const double* c = b.cam + b.cam_step * e;
            const double fx = c[0], fy = c[1], bf = c[4];
            const bool st = b.stereo[e];
            const int d = st ? 3 : 2;
            double A[3][3], Bm[3][6];
            if (!st) {
                const double tmp[2][3] = {{fx, 0, -x * iz * fx}, {0, fy, -y * iz * fy}};
                for (int r = 0; r < 2; r++)
                    for (int j = 0; j < 3; j++) {
                        double s = 0;
                        for (int m = 0; m < 3; m++) s += tmp[r][m] * R[3 * m + j];
                        A[r][j] = -iz * s;
                    }
                for (int j = 0; j < 3; j++) A[2][j] = 0;
            } else {
                for (int j = 0; j < 3; j++) {
                    A[0][j] = -fx * R[j] * iz + fx * x * R[6 + j] * iz2;
                    A[1][j] = -fy * R[3 + j] * iz + fy * y * R[6 + j] * iz2;
                    A[2][j] = A[0][j] - bf * R[6 + j] * iz2;
                }
            }
            Bm[0][0] = x * y * iz2 * fx; Bm[0][1] = -(1 + (x * x * iz2)) * fx; Bm[0][2] = y * iz * fx;
            Bm[0][3] = -iz * fx;         Bm[0][4] = 0;                         Bm[0][5] = x * iz2 * fx;
            Bm[1][0] = (1 + y * y * iz2) * fy; Bm[1][1] = -x * y * iz2 * fy; Bm[1][2] = -x * iz * fy;
            Bm[1][3] = 0;                      Bm[1][4] = -iz * fy;          Bm[1][5] = y * iz2 * fy;
            if (st) {
                Bm[2][0] = Bm[0][0] - bf * y * iz2; Bm[2][1] = Bm[0][1] + bf * x * iz2; Bm[2][2] = Bm[0][2];
                Bm[2][3] = Bm[0][3];                Bm[2][4] = 0;                       Bm[2][5] = Bm[0][5] - bf * iz2;
            } else {
                for (int j = 0; j < 6; j++) Bm[2][j] = 0;
            }
            double r0, r1;
            robustify(b, e, edge_chi2(b, e), r0, r1);
            const double w = r1 * b.info[e];
            // row 2 of A / Bm and om_r[2] are zero for a mono edge, so the fixed 3-row sums add exact
            // zeros to the reference's 2-row sums (same values) and every array stays in registers
            double om_r[3];
#pragma unroll
            for (int r = 0; r < 3; r++) om_r[r] = r < d ? -b.info[e] * b.err[3 * e + r] * r1 : 0.0;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                double s = 0;
#pragma unroll
                for (int r = 0; r < 3; r++) s += A[r][i] * om_r[r];
                g[i] += s;
#pragma unroll
                for (int j = 0; j < 3; j++) {
                    double h = 0;
#pragma unroll
                    for (int r = 0; r < 3; r++) h += A[r][i] * w * A[r][j];
                    H[3 * i + j] += h;
                }
            }
            if (rc.w >= 0) {   // free pose
                double* J = b.J + (long long)k * 72;
#pragma unroll
                for (int i = 0; i < 6; i++) {
                    double s = 0;
#pragma unroll
                    for (int r = 0; r < 3; r++) s += Bm[r][i] * om_r[r];
                    J[48 + i] = s;
#pragma unroll
                    for (int j = 0; j < 6; j++) {
                        double h = 0;
#pragma unroll
                        for (int r = 0; r < 3; r++) h += Bm[r][i] * w * Bm[r][j];
                        J[12 + 6 * i + j] = h;
                    }
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        double h = 0;
#pragma unroll
                        for (int r = 0; r < 3; r++) h += Bm[r][i] * w * A[r][j];
                        J[54 + 3 * i + j] = h;
                    }
                }
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = grp_sum(H[i]);
#pragma unroll
    for (int i = 0; i < 3; i++) g[i] = grp_sum(g[i]);
    chi = grp_sum(chi);
    if (b.ctl->it == 0) {   // first trial of an optimize(): computeLambdaInit's max over the points' diagonals
        double m = live && sub == 0 ? fmax(fabs(H[0]), fmax(fabs(H[4]), fabs(H[8]))) : 0.0;
        for (int o = 32; o >= GRP; o >>= 1) m = fmax(m, __shfl_xor(m, o, 64));
        if (threadIdx.x == 0 && m > 0)
            atomicMax(&b.ctl->maxdiag_bits, (unsigned long long)__double_as_longlong(m));
    }
    if (live && sub == 0) {
        for (int i = 0; i < 9; i++) b.Hll[9 * l + i] = H[i];
        for (int i = 0; i < 3; i++) b.bl[3 * l + i] = g[i];
        b.rchi[l] = chi;
    }
    // the lane's own J writes above are visible to its own reads in schur_point_terms
    if (live && schur) schur_point_terms(b, l, sub, H, g, b.ctl->lambda);
}

// One workgroup (1008 threads) per free pose: 42 sums (Hpp 36 + b 6), 24 partial groups with
// four interleaved accumulators each, combined in a fixed order.  Block np: chi2 total.
constexpr int PA_G = 24;
// (the caller staged the pose's slots with stage_pose_slots and a barrier; a pose with more than
// PA_SLOTS edges reads them from HBM)
__device__ __forceinline__ void pose_accum(const BADev& b, int i, double* sh, const int* sslot) {
    const int g = threadIdx.x / 42, c = threadIdx.x % 42;
    const int beg = b.ps_beg[i], end = b.ps_beg[i + 1];
    auto sum = [&](auto slot) {   // slot(u), u in [beg, end): LDS-staged or HBM (two instantiations)
        double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        int u = beg + g;
        for (; u + 3 * PA_G < end; u += 4 * PA_G) {
            s0 += b.J[(long long)slot(u) * 72 + 12 + c];
            s1 += b.J[(long long)slot(u + PA_G) * 72 + 12 + c];
            s2 += b.J[(long long)slot(u + 2 * PA_G) * 72 + 12 + c];
            s3 += b.J[(long long)slot(u + 3 * PA_G) * 72 + 12 + c];
        }
        for (; u < end; u += PA_G) s0 += b.J[(long long)slot(u) * 72 + 12 + c];
        sh[g * 42 + c] = (s0 + s1) + (s2 + s3);
    };
    if (g < PA_G) {
        if (end - beg <= PA_SLOTS) sum([&](int u) { return sslot[u - beg]; });
        else sum([&](int u) { return b.ps_slot[u]; });
    }
    __syncthreads();
    if (threadIdx.x < 42) {
        double s = 0;
        for (int q = 0; q < PA_G; q++) s += sh[q * 42 + threadIdx.x];
        if (threadIdx.x < 36) b.Hpp[36 * i + threadIdx.x] = s;
        else b.bp[6 * i + threadIdx.x - 36] = s;
    }
    __syncthreads();   // sh reused by the caller; Hpp / bp read back by the same workgroup
}

// The first trial of an optimize() call (computeLambdaInit needs Hpp before the Schur step);
// later linearising trials accumulate inside ba_schur_block_kernel.
__global__ __launch_bounds__(1024) void ba_pose_accum_kernel(BADev b) {
    if (b.ctl->done || !b.ctl->need_lin) return;
    __shared__ double sh[1024];
    __shared__ int sslot[PA_SLOTS];
    if ((int)blockIdx.x == b.np) chi_total(b, sh);
    else {
        stage_pose_slots(b, blockIdx.x, sslot);
        __syncthreads();
        pose_accum(b, blockIdx.x, sh, sslot);   // ends with a barrier: Hpp visible to the workgroup
        if (threadIdx.x == 0) {   // computeLambdaInit's max over this pose's diagonal
            double m = 0;
            for (int k = 0; k < 6; k++) m = fmax(m, fabs(b.Hpp[36 * blockIdx.x + 7 * k]));
            if (m > 0) atomicMax(&b.ctl->maxdiag_bits, (unsigned long long)__double_as_longlong(m));
        }
    }
}

// The first trial of an optimize() call: computeLambdaInit (levenberg.cpp:166-180: tau * max |diag H|
// over the active vertices, the max gathered by ba_iter_kernel and ba_pose_accum_kernel), then the
// Schur point terms with that lambda.
__global__ __launch_bounds__(64) void ba_schur_point_kernel(BADev b) {
    BA_RETURN_IF_DONE(b);
    const double maxdiag = __longlong_as_double((long long)b.ctl->maxdiag_bits);
    const double lam = 1e-5 * maxdiag;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0) {
        b.ctl->maxdiag = maxdiag;
        b.ctl->lambda = lam;
        b.ctl->ni = 2;
    }
    const int l = t / GRP, sub = t % GRP;
    if (l >= b.nl) return;
    double H[9], g[3];
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = b.Hll[9 * l + i];
#pragma unroll
    for (int i = 0; i < 3; i++) g[i] = b.bl[3 * l + i];
    schur_point_terms(b, l, sub, H, g, lam);
}

}  // namespace orbamd
