// The per-hypothesis arithmetic of the monocular Initializer (include/Initializer.h, src/Initializer.cc): the
// draw of eight correspondences (:83-98), ComputeH21 / ComputeF21 (:227-304), CheckHomography / CheckFundamental
// (:306-469), DecomposeE (:910-930), the eight hypotheses of ReconstructH (:585-687), Triangulate (:735-748) and
// one correspondence of CheckRT (:831-895).  Plain IEEE arithmetic that compiles for host and device
// (-ffp-contract=off, as the whole library): orbinit.hip runs it per lane, tests/native/initializer_check.cpp on
// the CPU, tests/initializer_ref.py restates it in numpy.
//
// What the reference holds in float and computes with float expressions (both Check* functions, CheckRT, the
// scalars of ReconstructH) is restated expression by expression.  Where the reference calls an OpenCV SVD or
// inv(), whose float rounding is not reproducible, a rule of the data stands, computed in fp64 from the float
// inputs and rounded to float only where the reference holds the result (H21i, H12i, F21i, R, t, x3D):
//   null vector    of an m x 9 / 4 x 4 A: the eigenvector of the smallest diagonal entry (first minimum) of
//                  A^T A after INI_SWEEPS9 / INI_SWEEPS cyclic Jacobi sweeps (rows p < q ascending).  A^T A is
//                  summed over the rows of A in ascending order.  The sign is whatever Jacobi leaves: every use
//                  is homogeneous.
//   rank 2         Fn = Fpre - (Fpre v3) v3^T with v3 the null-most eigenvector of Fpre^T Fpre: this is
//                  u diag(w1, w2, 0) vt without ever forming u.
//   inverses       adjugate / determinant (T2, H21i, K).
//   3 x 3 SVD      V and the order from Jacobi on A^T A (eigenvalues descending, stable), w_i = |A v_i|,
//                  u_1,2 = A v_i / w_i, u_3 = +-(u_1 x u_2) with the sign of (u_1 x u_2) . (A v_3): a true SVD
//                  also when w_3 is 0 (an essential matrix), where A v_3 / w_3 would be noise.
//   s              in ReconstructH: the sign of det(U) det(V), exactly +-1.
// Matrix products whose order OpenCV does not show are fixed as ((a0 b0 + a1 b1) + a2 b2), k ascending; cv::norm
// and Mat::dot accumulate in double, ascending.  No loop has a data-dependent trip count.
//
// Departures (orbinit.hip): N < 8 correspondences evaluate nothing (the reference would draw from an empty vector);
// a frame with more than ORBM_PROJ_MAX_KP keypoints is not processed; a draw outside [0, rand_max] is clamped to
// a valid position by the device entry and refused by the host entry.
#pragma once

#include <cmath>
#include <cstdint>

#include "sim3_hyp.h"

#define INI_HD S3H_HD

namespace orbamd {

constexpr int INI_SWEEPS9 = 12;   // cyclic Jacobi, symmetric 9 x 9: fp64 rounding is reached after 7 to 9
constexpr int INI_SWEEPS = 8;     // 3 x 3 and 4 x 4, as S3H_SWEEPS

// Initializer.cc:83-98 on vAvailableIndices = 0 .. n - 1 without the vector: position r holds r until a draw
// writes the then back into it; (pos, val) are those writes, the latest one of a position wins.  n >= 8.
INI_HD void ini_pick8(const int32_t* draw, int32_t rand_max, int n, int* idx) {
    int pos[8], val[8];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const int size = n - j;
        const int r = s3h_random_int(draw[j], rand_max, size);
        int vr = r, vb = size - 1;
#pragma unroll
        for (int k = 0; k < j; k++) {
            vr = pos[k] == r ? val[k] : vr;
            vb = pos[k] == size - 1 ? val[k] : vb;
        }
        idx[j] = vr;
        pos[j] = r;
        val[j] = vb;
    }
}

// Cyclic Jacobi on the symmetric A (only i <= j is read and kept), V = the rotations' product: A_in = V A V^T.
template <int N>
INI_HD void ini_jacobi(double (&A)[N][N], double (&V)[N][N], int sweeps) {
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) V[i][j] = i == j ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < sweeps; sweep++) {
#pragma unroll
        for (int p = 0; p < N - 1; p++)
#pragma unroll
            for (int q = p + 1; q < N; q++) {
                const double apq = A[p][q];
                const bool rot = apq != 0.0;
                const double tau = rot ? (A[q][q] - A[p][p]) / (2.0 * apq) : 0.0;
                const double t = rot ? (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau)) : 0.0;
                const double c = 1.0 / sqrt(1.0 + t * t);
                const double s = t * c;
                A[p][p] = A[p][p] - t * apq;
                A[q][q] = A[q][q] + t * apq;
                A[p][q] = 0.0;
#pragma unroll
                for (int k = 0; k < N; k++) {
                    if (k != p && k != q) {
                        double& akp = k < p ? A[k][p] : A[p][k];
                        double& akq = k < q ? A[k][q] : A[q][k];
                        const double x = akp, y = akq;
                        akp = c * x - s * y;
                        akq = s * x + c * y;
                    }
                    const double vx = V[k][p], vy = V[k][q];
                    V[k][p] = c * vx - s * vy;
                    V[k][q] = s * vx + c * vy;
                }
            }
    }
}

// the column of V under the smallest diagonal entry of A, first minimum
template <int N>
INI_HD void ini_min_vector(const double (&A)[N][N], const double (&V)[N][N], double* v) {
    double best = A[0][0];
#pragma unroll
    for (int k = 0; k < N; k++) v[k] = V[k][0];
#pragma unroll
    for (int j = 1; j < N; j++) {
        const bool lower = A[j][j] < best;
        best = lower ? A[j][j] : best;
#pragma unroll
        for (int k = 0; k < N; k++) v[k] = lower ? V[k][j] : v[k];
    }
}

template <int N>
INI_HD void ini_ata_zero(double (&M)[N][N]) {
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = 0; j < N; j++) M[i][j] = 0.0;
}

// M += row^T row, the upper triangle
template <int N>
INI_HD void ini_ata_add(double (&M)[N][N], const float* row) {
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
        for (int j = i; j < N; j++) M[i][j] = M[i][j] + (double)row[i] * (double)row[j];
}

// ComputeH21 (:227-267): pn1 / pn2 = the eight normalised points (x, y) of either frame; Hn = vt.row(8), fp64.
INI_HD void ini_compute_h21(const float* pn1, const float* pn2, double* Hn) {
    double M[9][9], V[9][9];
    ini_ata_zero(M);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const float u1 = pn1[2 * i], v1 = pn1[2 * i + 1], u2 = pn2[2 * i], v2 = pn2[2 * i + 1];
        const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
        const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, -u2 * u1, -u2 * v1, -u2};
        ini_ata_add(M, r0);
        ini_ata_add(M, r1);
    }
    ini_jacobi(M, V, INI_SWEEPS9);
    ini_min_vector(M, V, Hn);
}

// C = A B, 3 x 3 row-major fp64
INI_HD void ini_mul3(const double* A, const double* B, double* C) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
}

INI_HD void ini_transpose3(const double* A, double* T) {
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) T[3 * i + j] = A[3 * j + i];
}

INI_HD double ini_det3(const double* M) {
    return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// adjugate / determinant
INI_HD void ini_inv3(const double* M, double* I) {
    const double det = ini_det3(M);
    I[0] = (M[4] * M[8] - M[5] * M[7]) / det;
    I[1] = (M[2] * M[7] - M[1] * M[8]) / det;
    I[2] = (M[1] * M[5] - M[2] * M[4]) / det;
    I[3] = (M[5] * M[6] - M[3] * M[8]) / det;
    I[4] = (M[0] * M[8] - M[2] * M[6]) / det;
    I[5] = (M[2] * M[3] - M[0] * M[5]) / det;
    I[6] = (M[3] * M[7] - M[4] * M[6]) / det;
    I[7] = (M[1] * M[6] - M[0] * M[7]) / det;
    I[8] = (M[0] * M[4] - M[1] * M[3]) / det;
}

// T of Normalize (:791-795) from its four floats (sX, sY, -meanX * sX, -meanY * sY)
INI_HD void ini_t_matrix(const float* T, double* M) {
    M[0] = T[0]; M[1] = 0.0; M[2] = T[2];
    M[3] = 0.0; M[4] = T[1]; M[5] = T[3];
    M[6] = 0.0; M[7] = 0.0; M[8] = 1.0;
}

// K from (fx, fy, cx, cy)
INI_HD void ini_k_matrix(const float* cam, double* K) {
    K[0] = cam[0]; K[1] = 0.0; K[2] = cam[2];
    K[3] = 0.0; K[4] = cam[1]; K[5] = cam[3];
    K[6] = 0.0; K[7] = 0.0; K[8] = 1.0;
}

// H21i = T2inv * Hn * T1 (:161), fp64 before the narrowing
INI_HD void ini_h21i(const float* T1, const float* T2, const double* Hn, double* H) {
    double t1[9], t2[9], t2i[9], tmp[9];
    ini_t_matrix(T1, t1);
    ini_t_matrix(T2, t2);
    ini_inv3(t2, t2i);
    ini_mul3(t2i, Hn, tmp);
    ini_mul3(tmp, t1, H);
}

// H12i = H21i.inv() (:162) of the float H21i
INI_HD void ini_inv3f(const float* H, double* I) {
    double h[9];
#pragma unroll
    for (int i = 0; i < 9; i++) h[i] = H[i];
    ini_inv3(h, I);
}

// ComputeF21 (:269-304): Fpre = vt.row(8), Fn = its rank-2 projection, both fp64
INI_HD void ini_compute_f21(const float* pn1, const float* pn2, double* Fpre, double* Fn) {
    double M[9][9], V[9][9];
    ini_ata_zero(M);
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const float u1 = pn1[2 * i], v1 = pn1[2 * i + 1], u2 = pn2[2 * i], v2 = pn2[2 * i + 1];
        const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
        ini_ata_add(M, r);
    }
    ini_jacobi(M, V, INI_SWEEPS9);
    ini_min_vector(M, V, Fpre);
    double G[3][3], W[3][3], v3[3], g[3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) G[i][j] = (Fpre[i] * Fpre[j] + Fpre[3 + i] * Fpre[3 + j]) + Fpre[6 + i] * Fpre[6 + j];
    ini_jacobi(G, W, INI_SWEEPS);
    ini_min_vector(G, W, v3);
#pragma unroll
    for (int i = 0; i < 3; i++) g[i] = (Fpre[3 * i] * v3[0] + Fpre[3 * i + 1] * v3[1]) + Fpre[3 * i + 2] * v3[2];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Fn[3 * i + j] = Fpre[3 * i + j] - g[i] * v3[j];
}

// F21i = T2^T * Fn * T1 (:213), fp64 before the narrowing
INI_HD void ini_f21i(const float* T1, const float* T2, const double* Fn, double* F) {
    double t1[9], t2[9], t2t[9], tmp[9];
    ini_t_matrix(T1, t1);
    ini_t_matrix(T2, t2);
    ini_transpose3(t2, t2t);
    ini_mul3(t2t, Fn, tmp);
    ini_mul3(tmp, t1, F);
}

// One correspondence of CheckHomography (:338-386): adds to score, returns bIn.
INI_HD bool ini_check_h(const float* H21, const float* H12, float u1, float v1, float u2, float v2, float invSigmaSquare,
                        float& score) {
    const float th = 5.991f;
    bool bIn = true;
    const float w2in1inv = 1.f / ((H12[6] * u2 + H12[7] * v2) + H12[8]);
    const float u2in1 = ((H12[0] * u2 + H12[1] * v2) + H12[2]) * w2in1inv;
    const float v2in1 = ((H12[3] * u2 + H12[4] * v2) + H12[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th)
        bIn = false;
    else
        score += th - chiSquare1;
    const float w1in2inv = 1.f / ((H21[6] * u1 + H21[7] * v1) + H21[8]);
    const float u1in2 = ((H21[0] * u1 + H21[1] * v1) + H21[2]) * w1in2inv;
    const float v1in2 = ((H21[3] * u1 + H21[4] * v1) + H21[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th)
        bIn = false;
    else
        score += th - chiSquare2;
    return bIn;
}

// One correspondence of CheckFundamental (:414-466)
INI_HD bool ini_check_f(const float* F, float u1, float v1, float u2, float v2, float invSigmaSquare, float& score) {
    const float th = 3.841f, thScore = 5.991f;
    bool bIn = true;
    const float a2 = (F[0] * u1 + F[1] * v1) + F[2];
    const float b2 = (F[3] * u1 + F[4] * v1) + F[5];
    const float c2 = (F[6] * u1 + F[7] * v1) + F[8];
    const float num2 = (a2 * u2 + b2 * v2) + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th)
        bIn = false;
    else
        score += thScore - chiSquare1;
    const float a1 = (F[0] * u2 + F[3] * v2) + F[6];
    const float b1 = (F[1] * u2 + F[4] * v2) + F[7];
    const float c1 = (F[2] * u2 + F[5] * v2) + F[8];
    const float num1 = (a1 * u1 + b1 * v1) + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th)
        bIn = false;
    else
        score += thScore - chiSquare2;
    return bIn;
}

// The 3 x 3 SVD rule of the header comment: A = U diag(w) V^T, w descending.
INI_HD void ini_svd3(const double* A, double* U, double* w, double* V) {
    double G[3][3], W[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) G[i][j] = (A[i] * A[j] + A[3 + i] * A[3 + j]) + A[6 + i] * A[6 + j];
    ini_jacobi(G, W, INI_SWEEPS);
    double e[3] = {G[0][0], G[1][1], G[2][2]};
    double v[3][3];   // v[c] = column c
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < 3; k++) v[c][k] = W[k][c];
    auto order = [&](int a, int b) {   // the larger eigenvalue first; equal ones keep their places
        const bool sw = e[b] > e[a];
        const double ea = e[a], eb = e[b];
        e[a] = sw ? eb : ea;
        e[b] = sw ? ea : eb;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double x = v[a][k], y = v[b][k];
            v[a][k] = sw ? y : x;
            v[b][k] = sw ? x : y;
        }
    };
    order(0, 1);
    order(1, 2);
    order(0, 1);
    double av[3][3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int i = 0; i < 3; i++) av[c][i] = (A[3 * i] * v[c][0] + A[3 * i + 1] * v[c][1]) + A[3 * i + 2] * v[c][2];
        w[c] = sqrt((av[c][0] * av[c][0] + av[c][1] * av[c][1]) + av[c][2] * av[c][2]);
    }
    double u[3][3];
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int i = 0; i < 3; i++) u[c][i] = av[c][i] / w[c];
    u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
    u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
    u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    const double n3 = sqrt((u[2][0] * u[2][0] + u[2][1] * u[2][1]) + u[2][2] * u[2][2]);
    const double side = (u[2][0] * av[2][0] + u[2][1] * av[2][1]) + u[2][2] * av[2][2];
    const double sg = side < 0.0 ? -n3 : n3;
#pragma unroll
    for (int i = 0; i < 3; i++) u[2][i] = u[2][i] / sg;
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int i = 0; i < 3; i++) {
            U[3 * i + c] = u[c][i];
            V[3 * i + c] = v[c][i];
        }
}

INI_HD void ini_round9(const double* M, float* F) {
#pragma unroll
    for (int i = 0; i < 9; i++) F[i] = (float)M[i];
}

// E21 = K^T F21 K and DecomposeE (:480-485, :910-930): R1, R2 (proper rotations) and the unit t, in float.
INI_HD void ini_decompose_e(const float* F21, const float* cam, float* R1, float* R2, float* t) {
    double K[9], Kt[9], F[9], tmp[9], E[9], U[9], w[3], V[9], Vt[9];
    ini_k_matrix(cam, K);
    ini_transpose3(K, Kt);
#pragma unroll
    for (int i = 0; i < 9; i++) F[i] = F21[i];
    ini_mul3(Kt, F, tmp);
    ini_mul3(tmp, K, E);
    ini_svd3(E, U, w, V);
    ini_transpose3(V, Vt);
    const double tn = sqrt((U[2] * U[2] + U[5] * U[5]) + U[8] * U[8]);
    t[0] = (float)(U[2] / tn); t[1] = (float)(U[5] / tn); t[2] = (float)(U[8] / tn);
    const double Wm[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1}, Wt[9] = {0, 1, 0, -1, 0, 0, 0, 0, 1};
    double r[9];
    ini_mul3(U, Wm, tmp);
    ini_mul3(tmp, Vt, r);
    const double s1 = ini_det3(r) < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int i = 0; i < 9; i++) R1[i] = (float)(s1 * r[i]);
    ini_mul3(U, Wt, tmp);
    ini_mul3(tmp, Vt, r);
    const double s2 = ini_det3(r) < 0.0 ? -1.0 : 1.0;
#pragma unroll
    for (int i = 0; i < 9; i++) R2[i] = (float)(s2 * r[i]);
}

// The eight motion hypotheses of ReconstructH (:585-687): R[8][9], t[8][3] in float.  Returns false where the
// reference returns early (:598): d1 / d2 < 1.00001 || d2 / d3 < 1.00001, float quotients against the double.
INI_HD bool ini_decompose_h(const float* H21, const float* cam, float* R, float* t) {
    double K[9], Ki[9], H[9], tmp[9], A[9], U[9], w[3], V[9], Vt[9];
    ini_k_matrix(cam, K);
    ini_inv3(K, Ki);
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = H21[i];
    ini_mul3(Ki, H, tmp);
    ini_mul3(tmp, K, A);
    ini_svd3(A, U, w, V);
    ini_transpose3(V, Vt);
    const double s = ini_det3(U) * ini_det3(Vt) < 0.0 ? -1.0 : 1.0;
    const float d1 = (float)w[0], d2 = (float)w[1], d3 = (float)w[2];
    const bool ok = !(d1 / d2 < 1.00001 || d2 / d3 < 1.00001);
    const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[4] = {aux1, aux1, -aux1, -aux1};
    const float x3[4] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
#pragma unroll
    for (int h = 0; h < 8; h++) {
        const int i = h & 3;
        const bool second = h >= 4;
        double Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        float tp0, tp2;
        if (!second) {
            Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
            tp0 = x1[i] * (d1 - d3);
            tp2 = -x3[i] * (d1 - d3);
        } else {
            Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1; Rp[6] = sphi[i]; Rp[8] = -cphi;
            tp0 = x1[i] * (d1 + d3);
            tp2 = x3[i] * (d1 + d3);
        }
        double r[9];
        ini_mul3(U, Rp, tmp);
        ini_mul3(tmp, Vt, r);
#pragma unroll
        for (int k = 0; k < 9; k++) R[9 * h + k] = (float)(s * r[k]);
        double tv[3];
#pragma unroll
        for (int k = 0; k < 3; k++) tv[k] = U[3 * k] * (double)tp0 + U[3 * k + 2] * (double)tp2;
        const double tn = sqrt((tv[0] * tv[0] + tv[1] * tv[1]) + tv[2] * tv[2]);
#pragma unroll
        for (int k = 0; k < 3; k++) t[3 * h + k] = (float)(tv[k] / tn);
    }
    return ok;
}

// What CheckRT derives from (R, t, K) before its loop (:815-827): P1 = K [I | 0], P2 = K [R | t], O2 = -R^T t.
struct IniView {
    float P1[12], P2[12], O2[3], R[9], t[3], cam[4];
};

INI_HD void ini_view(const float* R, const float* t, const float* cam, IniView& v) {
    const float fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3];
    const float P1[12] = {fx, 0.f, cx, 0.f, 0.f, fy, cy, 0.f, 0.f, 0.f, 1.f, 0.f};
#pragma unroll
    for (int i = 0; i < 12; i++) v.P1[i] = P1[i];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const float r0 = j < 3 ? R[j] : t[0], r1 = j < 3 ? R[3 + j] : t[1], r2 = j < 3 ? R[6 + j] : t[2];
        v.P2[j] = (fx * r0 + 0.f * r1) + cx * r2;
        v.P2[4 + j] = (0.f * r0 + fy * r1) + cy * r2;
        v.P2[8 + j] = (0.f * r0 + 0.f * r1) + 1.f * r2;
    }
#pragma unroll
    for (int i = 0; i < 3; i++) v.O2[i] = ((-R[i]) * t[0] + (-R[3 + i]) * t[1]) + (-R[6 + i]) * t[2];
#pragma unroll
    for (int i = 0; i < 9; i++) v.R[i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) v.t[i] = t[i];
#pragma unroll
    for (int i = 0; i < 4; i++) v.cam[i] = cam[i];
}

// Triangulate (:735-748): x = vt.row(3)[0..2] / vt.row(3)[3], fp64 before the narrowing
INI_HD void ini_triangulate(const float* P1, const float* P2, float u1, float v1, float u2, float v2, double* x) {
    double M[4][4], V[4][4], nv[4];
    ini_ata_zero(M);
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; j++) r[j] = u1 * P1[8 + j] - P1[j];
    ini_ata_add(M, r);
#pragma unroll
    for (int j = 0; j < 4; j++) r[j] = v1 * P1[8 + j] - P1[4 + j];
    ini_ata_add(M, r);
#pragma unroll
    for (int j = 0; j < 4; j++) r[j] = u2 * P2[8 + j] - P2[j];
    ini_ata_add(M, r);
#pragma unroll
    for (int j = 0; j < 4; j++) r[j] = v2 * P2[8 + j] - P2[4 + j];
    ini_ata_add(M, r);
    ini_jacobi(M, V, INI_SWEEPS);
    ini_min_vector(M, V, nv);
#pragma unroll
    for (int k = 0; k < 3; k++) x[k] = nv[k] / nv[3];
}

// One inlier correspondence of CheckRT's loop (:836-894).  Returns whether it is counted (nGood++, vP3D set,
// cosParallax pushed); good = vbGood.
INI_HD bool ini_check_rt(const IniView& v, float u1, float v1, float u2, float v2, float th2, float* p3d, float& cosParallax,
                         bool& good) {
    good = false;
    cosParallax = 0.f;
    double xd[3];
    ini_triangulate(v.P1, v.P2, u1, v1, u2, v2, xd);
    const float X = (float)xd[0], Y = (float)xd[1], Z = (float)xd[2];
    p3d[0] = X; p3d[1] = Y; p3d[2] = Z;
    if (!std::isfinite(X) || !std::isfinite(Y) || !std::isfinite(Z)) return false;
    const float n2x = X - v.O2[0], n2y = Y - v.O2[1], n2z = Z - v.O2[2];
    const float dist1 = (float)sqrt(((double)X * X + (double)Y * Y) + (double)Z * Z);
    const float dist2 = (float)sqrt(((double)n2x * n2x + (double)n2y * n2y) + (double)n2z * n2z);
    const double dot = ((double)X * n2x + (double)Y * n2y) + (double)Z * n2z;
    cosParallax = (float)(dot / (double)(dist1 * dist2));
    if (Z <= 0 && cosParallax < 0.99998) return false;
    const float X2 = ((v.R[0] * X + v.R[1] * Y) + v.R[2] * Z) + v.t[0];
    const float Y2 = ((v.R[3] * X + v.R[4] * Y) + v.R[5] * Z) + v.t[1];
    const float Z2 = ((v.R[6] * X + v.R[7] * Y) + v.R[8] * Z) + v.t[2];
    if (Z2 <= 0 && cosParallax < 0.99998) return false;
    const float fx = v.cam[0], fy = v.cam[1], cx = v.cam[2], cy = v.cam[3];
    const float invZ1 = 1.f / Z;
    const float im1x = fx * X * invZ1 + cx, im1y = fy * Y * invZ1 + cy;
    const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
    if (squareError1 > th2) return false;
    const float invZ2 = 1.f / Z2;
    const float im2x = fx * X2 * invZ2 + cx, im2y = fy * Y2 * invZ2 + cy;
    const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
    if (squareError2 > th2) return false;
    good = cosParallax < 0.99998;
    return true;
}

// parallax = acos(cos) * 180 / CV_PI (:902), in double, narrowed
INI_HD float ini_parallax_deg(float c) { return (float)(acos((double)c) * 180 / 3.1415926535897932384626433832795); }

}  // namespace orbamd
