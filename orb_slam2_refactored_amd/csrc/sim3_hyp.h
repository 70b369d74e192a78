// One Sim3Solver hypothesis in the reference's expressions (src/Sim3Solver.cc): the draw of three
// correspondences (:307-322), ComputeSim3 (:111-163) and the reprojection error of one correspondence
// (:165-184, :333-340).  Plain IEEE arithmetic that compiles for host and device (-ffp-contract=off, as the
// whole library): orbsim3solver.hip runs it per lane; tests/sim3solver_ref.py restates it in numpy.
//
// Where the reference's checkout does not show OpenCV's accumulation order, one order is fixed here:
//   cv::reduce (centroid)      float, ((P(i,0) + P(i,1)) + P(i,2)) / 3.f
//   Pr2 * Pr1.t(), R12 * Pr2   float, ((a0 * b0 + a1 * b1) + a2 * b2), k ascending
//   Pr1.dot(P3)                the float entries widened, products and sum in double, row-major
// The rotation is not OpenCV's float Jacobi SVD (not reproducible bit for bit): it is computed in fp64 from
// the float M and rounded to float.  Three centred points give a rank-2 M, so the third singular vectors of
// M are arbitrary and U S Vh is fixed only by the determinant rule; Horn's unit-quaternion form (the
// reference's own #else branch, :67-107) names the same proper rotation as the eigenvector of the largest
// eigenvalue of the symmetric 4x4 N(M), which is simple whenever the second singular value is not 0, and
// never forms a singular vector of the null direction.  The eigenvector comes from cyclic Jacobi with a fixed
// number of sweeps (no data-dependent trip count: the lanes of a wavefront do not diverge).
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define S3H_HD __host__ __device__ __forceinline__
#else
#define S3H_HD inline
#endif

namespace orbamd {

constexpr int S3H_SWEEPS = 8;   // cyclic Jacobi on a symmetric 4x4 converges quadratically: 5 reach fp64 rounding

// DUtils::Random::RandomInt(0, d - 1) of the raw rand() value r (Random.cpp), clamped into [0, d - 1] so that
// a draw outside [0, rand_max] (the device entry cannot refuse it) still names a correspondence
S3H_HD int s3h_random_int(int32_t r, int32_t rand_max, int d) {
    const int v = (int)(((double)r / ((double)rand_max + 1.0)) * d);
    return v < 0 ? 0 : (v > d - 1 ? d - 1 : v);
}

// Sim3Solver.cc:307-322 on availableIndices = 0 .. n - 1 without the vector: position r holds r until a draw
// takes it, after which it holds what was then the back.  n >= 3.
S3H_HD void s3h_pick(const int32_t* draw, int32_t rand_max, int n, int* idx) {
    const int r0 = s3h_random_int(draw[0], rand_max, n);
    const int r1 = s3h_random_int(draw[1], rand_max, n - 1);
    const int r2 = s3h_random_int(draw[2], rand_max, n - 2);
    const int back1 = (r0 == n - 2) ? n - 1 : n - 2;   // the back when the second draw refills its position
    idx[0] = r0;
    idx[1] = (r1 == r0) ? n - 1 : r1;
    idx[2] = (r2 == r1) ? back1 : ((r2 == r0) ? n - 1 : r2);
}

// The proper rotation R (row-major, fp64) with p1 ~ R p2 for M = sum p2 p1^T, M row-major float.
S3H_HD void s3h_rotation(const float* M, double* R) {
    const double Sxx = M[0], Sxy = M[1], Sxz = M[2], Syx = M[3], Syy = M[4], Syz = M[5], Szx = M[6], Szy = M[7], Szz = M[8];
    double A[4][4], V[4][4];
    A[0][0] = (Sxx + Syy) + Szz;
    A[0][1] = Syz - Szy; A[0][2] = Szx - Sxz; A[0][3] = Sxy - Syx;
    A[1][1] = (Sxx - Syy) - Szz;
    A[1][2] = Sxy + Syx; A[1][3] = Szx + Sxz;
    A[2][2] = (-Sxx + Syy) - Szz;
    A[2][3] = Syz + Szy;
    A[3][3] = (-Sxx - Syy) + Szz;
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            V[i][j] = i == j ? 1.0 : 0.0;
            if (j < i) A[i][j] = A[j][i];
        }
    for (int sweep = 0; sweep < S3H_SWEEPS; sweep++) {
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                const double apq = A[p][q];
                double c = 1.0, s = 0.0;
                if (apq != 0.0) {   // the rotation that zeroes A[p][q] (Golub & Van Loan 8.4.2)
                    const double tau = (A[q][q] - A[p][p]) / (2.0 * apq);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = t * c;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {   // A <- A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq;
                    A[k][q] = s * akp + c * akq;
                }
#pragma unroll
                for (int k = 0; k < 4; k++) {   // A <- J^T A, V <- V J
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk;
                    A[q][k] = s * apk + c * aqk;
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq;
                    V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    double best = A[0][0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int j = 1; j < 4; j++) {
        const bool up = A[j][j] > best;
        best = up ? A[j][j] : best;
#pragma unroll
        for (int k = 0; k < 4; k++) q[k] = up ? V[k][j] : q[k];
    }
    const double nrm = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    const double w = q[0] / nrm, x = q[1] / nrm, y = q[2] / nrm, z = q[3] / nrm;
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// S.Inverse() (Sim3.h:43-47): R21 = R12^T, t21 = ((-(1.f / s)) * R12^T) * t12, s21 = 1.f / s.  13 floats each:
// R (row-major), t, s.
S3H_HD void s3h_inverse(const float* S, float* I) {
    const float inv_s = 1.f / S[12], neg = -inv_s;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        I[9 + r] = ((neg * S[r]) * S[9] + (neg * S[3 + r]) * S[10]) + (neg * S[6 + r]) * S[11];
#pragma unroll
        for (int c = 0; c < 3; c++) I[3 * r + c] = S[3 * c + r];
    }
    I[12] = inv_s;
}

// ComputeSim3 (:111-163).  P1 / P2: the three camera-frame points of either keyframe, point c at P[3 * c].
S3H_HD void s3h_compute_sim3(const float* P1, const float* P2, bool fix_scale, float* S12, float* S21) {
    float O1[3], O2[3], Pr1[9], Pr2[9];   // Pr: row i, column c at Pr[3 * i + c], as the reference's 3x3 Mat
#pragma unroll
    for (int i = 0; i < 3; i++) {
        O1[i] = ((P1[i] + P1[3 + i]) + P1[6 + i]) / 3.f;
        O2[i] = ((P2[i] + P2[3 + i]) + P2[6 + i]) / 3.f;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            Pr1[3 * i + c] = P1[3 * c + i] - O1[i];
            Pr2[3 * i + c] = P2[3 * c + i] - O2[i];
        }
    }
    float M[9];   // Pr2 * Pr1^T
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            M[3 * i + j] = (Pr2[3 * i] * Pr1[3 * j] + Pr2[3 * i + 1] * Pr1[3 * j + 1]) + Pr2[3 * i + 2] * Pr1[3 * j + 2];
    double Rd[9];
    s3h_rotation(M, Rd);
    float R[9], P3[9];
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = (float)Rd[i];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int c = 0; c < 3; c++)
            P3[3 * i + c] = (R[3 * i] * Pr2[c] + R[3 * i + 1] * Pr2[3 + c]) + R[3 * i + 2] * Pr2[6 + c];
    float s = 1.f;
    if (!fix_scale) {
        double nom = 0, den = 0;
#pragma unroll
        for (int i = 0; i < 9; i++) {
            nom += (double)Pr1[i] * (double)P3[i];
            den += P3[i] * P3[i];
        }
        s = (float)(nom / den);
    }
#pragma unroll
    for (int i = 0; i < 3; i++) {   // t12 = O1 - (s12 * R12) * O2
        const float sr0 = s * R[3 * i], sr1 = s * R[3 * i + 1], sr2 = s * R[3 * i + 2];
        S12[9 + i] = O1[i] - ((sr0 * O2[0] + sr1 * O2[1]) + sr2 * O2[2]);
    }
#pragma unroll
    for (int i = 0; i < 9; i++) S12[i] = R[i];
    S12[12] = s;
    s3h_inverse(S12, S21);
}

// The 3 x 4 that Sim3::Map applies (Sim3.h:40): s * R scaled elementwise, then t.
S3H_HD void s3h_map_matrix(const float* S, float* m) {
#pragma unroll
    for (int i = 0; i < 9; i++) m[i] = S[12] * S[i];
#pragma unroll
    for (int i = 0; i < 3; i++) m[9 + i] = S[9 + i];
}

// |point - Project(X)|^2 (:165-184, :335-338) in float; IEEE: a zero or negative depth gives inf or NaN and
// the comparison against the threshold is then false.
S3H_HD float s3h_error_sq(const float* m, const float* cam, float X0, float X1, float X2, float px, float py) {
    const float x = ((m[0] * X0 + m[1] * X1) + m[2] * X2) + m[9];
    const float y = ((m[3] * X0 + m[4] * X1) + m[5] * X2) + m[10];
    const float z = ((m[6] * X0 + m[7] * X1) + m[8] * X2) + m[11];
    const float invZ = 1.f / z;
    const float u = x * invZ, v = y * invZ;
    const float dx = px - (cam[0] * u + cam[2]), dy = py - (cam[1] * v + cam[3]);
    return dx * dx + dy * dy;
}

// FromCameraToImage (:186-204)
S3H_HD void s3h_to_image(const float* cam, float X0, float X1, float X2, float* p) {
    const float invZ = 1 / X2;
    const float u = X0 * invZ, v = X1 * invZ;
    p[0] = cam[0] * u + cam[2];
    p[1] = cam[1] * v + cam[3];
}

}  // namespace orbamd
