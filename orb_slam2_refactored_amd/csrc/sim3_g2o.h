// g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h) in fp64, in the reference's evaluation order: the constructor
// from a 7-vector (exp), operator*, inverse() and log().  Shared by OptimizeSim3 (orbsim3.hip) and
// OptimizeEssentialGraph (orbeg.hip); compiles for the host too (tests/native/essential_graph_check.cpp).
#pragma once

#include "se3.h"

namespace orbamd {

struct S3 { double q[4], t[3], s; };   // g2o::Sim3: r (x, y, z, w), t, s

// Sim3(const Vector7d& update), sim3.h:70-142
__host__ __device__ __forceinline__ void s3_exp(const double* u, S3& out) {
    const double w0 = u[0], w1 = u[1], w2 = u[2], sigma = u[6];
    const double theta = sqrt((w0 * w0 + w1 * w1) + w2 * w2);
    const double O[9] = {0, -w2, w1, w2, 0, -w0, -w1, w0, 0};
    double O2[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++)
            O2[3 * i + j] = (O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j]) + O[3 * i + 2] * O[6 + j];
    const double s = exp(sigma);
    const double eps = 0.00001;
    double A, B, C, R[9];
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.;
            B = 1. / 6.;
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + O[i]) + O2[i];
        } else {
            double sn, cs;
            sincos(theta, &sn, &cs);
            const double theta2 = theta * theta;
            A = (1 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
            const double ra = sn / theta, rb = (1 - cs) / (theta * theta);
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + ra * O[i]) + rb * O2[i];
        }
    } else {
        C = (s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + O[i]) + O2[i];
        } else {
            double sn, cs;
            sincos(theta, &sn, &cs);
            const double ra = sn / theta, rb = (1 - cs) / (theta * theta);
#pragma unroll
            for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0 ? 1.0 : 0.0) + ra * O[i]) + rb * O2[i];
            const double a = s * sn, b = s * cs;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    const Q4 r = q_from_R(R);   // Quaterniond(R), not renormalised
    out.q[0] = r.x; out.q[1] = r.y; out.q[2] = r.z; out.q[3] = r.w;
    out.s = s;
#pragma unroll
    for (int i = 0; i < 3; i++) {   // t = W * upsilon, W = A Omega + B Omega^2 + C I
        const double W0 = (A * O[3 * i] + B * O2[3 * i]) + C * (i == 0 ? 1.0 : 0.0);
        const double W1 = (A * O[3 * i + 1] + B * O2[3 * i + 1]) + C * (i == 1 ? 1.0 : 0.0);
        const double W2 = (A * O[3 * i + 2] + B * O2[3 * i + 2]) + C * (i == 2 ? 1.0 : 0.0);
        out.t[i] = (W0 * u[3] + W1 * u[4]) + W2 * u[5];
    }
}

// operator*, sim3.h:266-272
__host__ __device__ __forceinline__ void s3_mul(const S3& a, const S3& b, S3& o) {
    const double ax = a.q[0], ay = a.q[1], az = a.q[2], aw = a.q[3];
    const double bx = b.q[0], by = b.q[1], bz = b.q[2], bw = b.q[3];
    double rt[3];
    q_rotate(a.q, b.t, rt);
    const double q0 = aw * bx + ax * bw + ay * bz - az * by, q1 = aw * by + ay * bw + az * bx - ax * bz,
                 q2 = aw * bz + az * bw + ax * by - ay * bx, q3 = aw * bw - ax * bx - ay * by - az * bz;
    const double s = a.s * b.s;
#pragma unroll
    for (int i = 0; i < 3; i++) o.t[i] = a.s * rt[i] + a.t[i];
    o.q[0] = q0; o.q[1] = q1; o.q[2] = q2; o.q[3] = q3;
    o.s = s;
}

// inverse(), sim3.h:233-236
__host__ __device__ __forceinline__ void s3_inverse(const S3& a, S3& o) {
    const double m = -1. / a.s;
    const double v[3] = {m * a.t[0], m * a.t[1], m * a.t[2]};
    o.q[0] = -a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = a.q[3];
    q_rotate(o.q, v, o.t);
    o.s = 1. / a.s;
}

// W.lu().solve(t) of log(): LU with partial pivoting (the first largest |entry| of the column), the
// eliminations and both substitutions one subtraction at a time with k ascending.  Rows move by selects, so
// nothing is indexed by a runtime value.
__host__ __device__ __forceinline__ void s3_lu3_solve(const double* W, const double* t, double* x) {
    double a[3][3] = {{W[0], W[1], W[2]}, {W[3], W[4], W[5]}, {W[6], W[7], W[8]}};
    double b[3] = {t[0], t[1], t[2]};
#define S3_SWAP_ROWS(r0, r1)                                                                     \
    do {                                                                                         \
        for (int c_ = 0; c_ < 3; c_++) { const double v_ = a[r0][c_]; a[r0][c_] = a[r1][c_]; a[r1][c_] = v_; } \
        const double w_ = b[r0]; b[r0] = b[r1]; b[r1] = w_;                                      \
    } while (0)
    {
        int p = 0;
        double m = fabs(a[0][0]);
        if (fabs(a[1][0]) > m) { m = fabs(a[1][0]); p = 1; }
        if (fabs(a[2][0]) > m) p = 2;
        if (p == 1) S3_SWAP_ROWS(0, 1);
        if (p == 2) S3_SWAP_ROWS(0, 2);
    }
    a[1][0] = a[1][0] / a[0][0];
    a[2][0] = a[2][0] / a[0][0];
    a[1][1] -= a[1][0] * a[0][1]; a[1][2] -= a[1][0] * a[0][2];
    a[2][1] -= a[2][0] * a[0][1]; a[2][2] -= a[2][0] * a[0][2];
    if (fabs(a[2][1]) > fabs(a[1][1])) S3_SWAP_ROWS(1, 2);
#undef S3_SWAP_ROWS
    a[2][1] = a[2][1] / a[1][1];
    a[2][2] -= a[2][1] * a[1][2];
    const double y0 = b[0];
    const double y1 = b[1] - a[1][0] * y0;
    const double y2 = (b[2] - a[2][0] * y0) - a[2][1] * y1;
    x[2] = y2 / a[2][2];
    x[1] = (y1 - a[1][2] * x[2]) / a[1][1];
    x[0] = ((y0 - a[0][1] * x[1]) - a[0][2] * x[2]) / a[0][0];
}

// log(), sim3.h:148-230: omega (3), upsilon (3), sigma; four branches, |sigma| < 1e-5 crossed with
// d > 1 - 1e-5 (se3_ops.hpp:27-47 for skew and deltaR)
__host__ __device__ __forceinline__ void s3_log(const S3& a, double* res) {
    const double sigma = log(a.s);
    double R[9];
    q_to_R(a.q, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double eps = 0.00001;
    double A, B, C, om[3];
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) {
#pragma unroll
            for (int i = 0; i < 3; i++) om[i] = 0.5 * dR[i];
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta = acos(d);
            const double theta2 = theta * theta;
            const double f = theta / (2 * sqrt(1 - d * d));
#pragma unroll
            for (int i = 0; i < 3; i++) om[i] = f * dR[i];
            A = (1 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (a.s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
#pragma unroll
            for (int i = 0; i < 3; i++) om[i] = 0.5 * dR[i];
            A = ((sigma - 1) * a.s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * a.s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d);
            const double f = theta / (2 * sqrt(1 - d * d));
#pragma unroll
            for (int i = 0; i < 3; i++) om[i] = f * dR[i];
            const double theta2 = theta * theta;
            const double sa = a.s * sin(theta);
            const double sb = a.s * cos(theta);
            const double c = theta2 + sigma * sigma;
            A = (sa * sigma + (1 - sb) * theta) / (theta * c);
            B = (C - ((sb - 1) * sigma + sa * theta) / c) * 1. / theta2;
        }
    }
    const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    double W[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double o2 = (O[3 * i] * O[j] + O[3 * i + 1] * O[3 + j]) + O[3 * i + 2] * O[6 + j];
            W[3 * i + j] = (A * O[3 * i + j] + B * o2) + C * (i == j ? 1.0 : 0.0);
        }
    double ups[3];
    s3_lu3_solve(W, a.t, ups);
#pragma unroll
    for (int i = 0; i < 3; i++) { res[i] = om[i]; res[3 + i] = ups[i]; }
    res[6] = sigma;
}

}  // namespace orbamd
