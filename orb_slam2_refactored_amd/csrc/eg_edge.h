// Per-edge and per-vertex arithmetic of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:743-942): the float
// Sim3 class of include/Sim3.h (cv::Matx expressions: a matrix product is float s = 0; s += a(i,k) * b(k,j), k
// ascending; scalar * matrix rounds every entry), ToG2OSim3 / FromG2OSim3 (Optimizer.cc:183-195), EdgeSim3's
// error (types_seven_dof_expmap.h:106-114) and VertexSim3Expmap::oplusImpl (:60-69).  Plain IEEE arithmetic
// for host and device (-ffp-contract=off): orbeg.hip runs it per lane, tests/native/essential_graph_check.cpp on
// the CPU, tests/essential_graph_ref.py restates it in numpy.
#pragma once

#include "sim3_g2o.h"

namespace orbamd {

struct F3 { float R[9], t[3], s; };   // ORB_SLAM2::Sim3: R row-major, t, s

__host__ __device__ __forceinline__ void f3_load(const float* row, F3& o) {
#pragma unroll
    for (int i = 0; i < 9; i++) o.R[i] = row[i];
#pragma unroll
    for (int i = 0; i < 3; i++) o.t[i] = row[9 + i];
    o.s = row[12];
}

// Matx33f * Matx31f
__host__ __device__ __forceinline__ void f3_matvec(const float* M, const float* v, float* o) {
#pragma unroll
    for (int i = 0; i < 3; i++) {
        float s = 0.f;
#pragma unroll
        for (int k = 0; k < 3; k++) s += M[3 * i + k] * v[k];
        o[i] = s;
    }
}

// Inverse(), Sim3.h:43-47: R^T, (-(1.f / s) * R^T) * t, 1.f / s
__host__ __device__ __forceinline__ void f3_inverse(const F3& a, F3& o) {
    const float m = -(1.f / a.s);
    float Rt[9], mR[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Rt[3 * i + j] = a.R[3 * j + i];
#pragma unroll
    for (int i = 0; i < 9; i++) mR[i] = Rt[i] * m;
    f3_matvec(mR, a.t, o.t);
#pragma unroll
    for (int i = 0; i < 9; i++) o.R[i] = Rt[i];
    o.s = 1.f / a.s;
}

// operator*, Sim3.h:49-64: t = (s1 * R1) * t2 + t1, R = R1 * R2, s = s1 * s2
__host__ __device__ __forceinline__ void f3_mul(const F3& a, const F3& b, F3& o) {
    float sR[9], v[3];
#pragma unroll
    for (int i = 0; i < 9; i++) sR[i] = a.R[i] * a.s;
    f3_matvec(sR, b.t, v);
#pragma unroll
    for (int i = 0; i < 3; i++) o.t[i] = v[i] + a.t[i];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            float s = 0.f;
#pragma unroll
            for (int k = 0; k < 3; k++) s += a.R[3 * i + k] * b.R[3 * k + j];
            o.R[3 * i + j] = s;
        }
    o.s = a.s * b.s;
}

// Map(), Sim3.h:40: (s * R) * x + t
__host__ __device__ __forceinline__ void f3_map(const F3& a, const float* x, float* o) {
    float sR[9], v[3];
#pragma unroll
    for (int i = 0; i < 9; i++) sR[i] = a.R[i] * a.s;
    f3_matvec(sR, x, v);
#pragma unroll
    for (int i = 0; i < 3; i++) o[i] = v[i] + a.t[i];
}

// ToG2OSim3 (Optimizer.cc:183-188): widened, the rotation through Quaterniond(R), not renormalised
__host__ __device__ __forceinline__ void f3_to_g2o(const F3& a, S3& o) {
    double Rm[9];
#pragma unroll
    for (int i = 0; i < 9; i++) Rm[i] = a.R[i];
    const Q4 q = q_from_R(Rm);
    o.q[0] = q.x; o.q[1] = q.y; o.q[2] = q.z; o.q[3] = q.w;
#pragma unroll
    for (int i = 0; i < 3; i++) o.t[i] = a.t[i];
    o.s = a.s;
}

// FromG2OSim3 (Optimizer.cc:190-195)
__host__ __device__ __forceinline__ void f3_from_g2o(const S3& a, F3& o) {
    double R[9];
    q_to_R(a.q, R);
#pragma unroll
    for (int i = 0; i < 9; i++) o.R[i] = (float)R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) o.t[i] = (float)a.t[i];
    o.s = (float)a.s;
}

// The measurement of an edge (i, j): Sji = Sjw * Swi in float (Optimizer.cc:808-818, :835-846), then ToG2OSim3
__host__ __device__ __forceinline__ void eg_measurement(const float* Siw, const float* Sjw, S3& meas) {
    F3 si, sj, swi, sji;
    f3_load(Siw, si);
    f3_load(Sjw, sj);
    f3_inverse(si, swi);
    f3_mul(sj, swi, sji);
    f3_to_g2o(sji, meas);
}

// EdgeSim3::computeError: log(C * v1 * v2^-1), v1 = vertex 0 (keyframe i), v2 = vertex 1 (keyframe j)
__host__ __device__ __forceinline__ void eg_error(const S3& C, const S3& v1, const S3& v2, double* e) {
    S3 v2i, a, b;
    s3_inverse(v2, v2i);
    s3_mul(C, v1, a);
    s3_mul(a, v2i, b);
    s3_log(b, e);
}

// oplusImpl: Sim3(update) * estimate, update[6] zeroed under _fix_scale
__host__ __device__ __forceinline__ void eg_oplus(const double* update, int fix_scale, const S3& est, S3& o) {
    double u[7];
#pragma unroll
    for (int i = 0; i < 7; i++) u[i] = update[i];
    if (fix_scale) u[6] = 0;
    S3 U;
    s3_exp(u, U);
    s3_mul(U, est, o);
}

// Optimizer.cc:911-921 for one keyframe: correctedSiw = FromG2OSim3(estimate), the pose (R, (1. / s) * t) with
// the product in double per component, and correctedSwc = correctedSiw.Inverse()
__host__ __device__ __forceinline__ void eg_recover_pose(const S3& est, float* pose12, F3& Swc) {
    F3 siw;
    f3_from_g2o(est, siw);
    f3_inverse(siw, Swc);
    const double invs = 1. / siw.s;
#pragma unroll
    for (int i = 0; i < 9; i++) pose12[i] = siw.R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) pose12[9 + i] = (float)(siw.t[i] * invs);
}

// Optimizer.cc:933-939 for one point: (correctedSwr * Srw).Map(P)
__host__ __device__ __forceinline__ void eg_correct_point(const F3& Swr, const float* Srw13, const float* P, float* o) {
    F3 srw, corr;
    f3_load(Srw13, srw);
    f3_mul(Swr, srw, corr);
    f3_map(corr, P, o);
}

}  // namespace orbamd
