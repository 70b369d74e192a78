// EPnP (PnPsolver::compute_pose, src/PnPsolver.cc:375-955) in fp64, scalar code for one lane or the host.
// orbpnp.hip runs epnp_pose_serial<true> per hypothesis lane and the pieces below around its wave sums in
// Refine(); every function also compiles for the host, where epnp_pose_serial<false> is Refine()'s EPnP.
//
// The four places where the reference asks OpenCV's SVD for something its rounding decides are rules of the
// data here (PnPsolver):
//   control-point axes   eigenvectors of the symmetric 3x3 PW0^T PW0 by a fixed-sweep Jacobi, eigenvalues
//                        descending, every vector signed so that its largest-magnitude component (lowest index
//                        on a tie) is positive; the inverse of CC is then row j = axis j / k_j
//   minimal-set basis    n = 4: the 8 rows of M orthonormalised (Gram-Schmidt, two passes), the projector
//                        P = I - U^T U onto the null space never formed: four pivoted Gram-Schmidt steps on its
//                        columns, each pivoting on the largest remaining diagonal (lowest index on a tie); the
//                        pivot component of each vector is positive; v[0..3] in pivot order
//   Refine null vectors  n >= 6: the eigenvectors of the four smallest eigenvalues of MtM by a fixed-sweep
//                        12x12 Jacobi, ascending, signed like the axes
//   R of ABt             the orthogonal polar factor by a scaled Newton iteration of fixed length, then the
//                        reference's det < 0 rule (row 2 negated)
// The three cv::solve(DECOMP_SVD) calls are least-squares solves by Householder QR, the same routine as the
// reference's qr_solve (a singular column gives x = 0 where the reference leaves x as it was).
#pragma once

#include <cmath>
#include <cstdint>

#include <hip/hip_runtime.h>

namespace orbamd {

#define EPNP_HD __host__ __device__ inline

constexpr int EPNP_SWEEPS3 = 8;     // 3x3 Jacobi sweeps
constexpr int EPNP_SWEEPS12 = 12;   // 12x12 Jacobi sweeps
constexpr int EPNP_POLAR_STEPS = 12;

// One Jacobi rotation of the symmetric n x n A (row-major, full) in the (p, q) plane, accumulated into the
// columns of V.  A rotation whose off-diagonal is below 1e-20 of the two diagonals is skipped (it would not
// change a bit of either).
EPNP_HD void epnp_rotate(double* A, double* V, int n, int p, int q) {
    const double apq = A[p * n + q], app = A[p * n + p], aqq = A[q * n + q];
    if (!(fabs(apq) > 1e-20 * (fabs(app) + fabs(aqq)))) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double tt = (theta < 0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(tt * tt + 1.0), s = tt * c;
    for (int k = 0; k < n; k++) {
        const double akp = A[k * n + p], akq = A[k * n + q];
        A[k * n + p] = c * akp - s * akq;
        A[k * n + q] = s * akp + c * akq;
    }
    for (int k = 0; k < n; k++) {
        const double apk = A[p * n + k], aqk = A[q * n + k];
        A[p * n + k] = c * apk - s * aqk;
        A[q * n + k] = s * apk + c * aqk;
    }
    for (int k = 0; k < n; k++) {
        const double vkp = V[k * n + p], vkq = V[k * n + q];
        V[k * n + p] = c * vkp - s * vkq;
        V[k * n + q] = s * vkp + c * vkq;
    }
}

// Cyclic Jacobi, pairs (p, q) row by row, a fixed number of sweeps.  On return A[i][i] are the eigenvalues
// and column i of V its eigenvector.
EPNP_HD void epnp_jacobi(double* A, double* V, int n, int sweeps) {
    for (int i = 0; i < n * n; i++) V[i] = 0.0;
    for (int i = 0; i < n; i++) V[i * n + i] = 1.0;
    for (int sw = 0; sw < sweeps; sw++)
        for (int p = 0; p < n - 1; p++)
            for (int q = p + 1; q < n; q++) epnp_rotate(A, V, n, p, q);
}

// Column `col` of V (n x n) into out, signed so that its largest-magnitude component is positive.
EPNP_HD void epnp_signed_column(const double* V, int n, int col, double* out) {
    double big = 0.0, at = 1.0;
    for (int i = 0; i < n; i++) {
        const double x = V[i * n + col];
        if (fabs(x) > big) { big = fabs(x); at = x; }
    }
    const double sg = at < 0 ? -1.0 : 1.0;
    for (int i = 0; i < n; i++) out[i] = sg * V[i * n + col];
}

// choose_control_points (:375-409) from the centroid c0, the six sums S = (xx, xy, xz, yy, yz, zz) of
// PW0^T PW0 and n; and the inverse of CC that compute_barycentric_coordinates (:411-434) uses.
EPNP_HD void epnp_control_points(const double S[6], int n, const double c0[3], double cws[12], double ci[9]) {
    double A[9] = {S[0], S[1], S[2], S[1], S[3], S[4], S[2], S[4], S[5]}, V[9];
    epnp_jacobi(A, V, 3, EPNP_SWEEPS3);
    int ord[3] = {0, 1, 2};   // descending, stable
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 2 - i; j++)
            if (A[4 * ord[j + 1]] > A[4 * ord[j]]) { const int t = ord[j]; ord[j] = ord[j + 1]; ord[j + 1] = t; }
    for (int j = 0; j < 3; j++) cws[j] = c0[j];
    for (int i = 0; i < 3; i++) {
        double e[3];
        epnp_signed_column(V, 3, ord[i], e);
        const double k = sqrt(fmax(A[4 * ord[i]], 0.0) / n);
        for (int j = 0; j < 3; j++) {
            cws[3 * (i + 1) + j] = c0[j] + k * e[j];
            ci[3 * i + j] = e[j] / k;
        }
    }
}

EPNP_HD void epnp_alphas(const double ci[9], const double c0[3], const double p[3], double a[4]) {
    for (int j = 0; j < 3; j++)
        a[1 + j] = ci[3 * j] * (p[0] - c0[0]) + ci[3 * j + 1] * (p[1] - c0[1]) + ci[3 * j + 2] * (p[2] - c0[2]);
    a[0] = 1.0 - a[1] - a[2] - a[3];
}

// fill_M (:436-451): the two rows of a correspondence.  cam = fu, fv, uc, vc.
EPNP_HD void epnp_rows(const double a[4], double u, double v, const double cam[4], double m1[12], double m2[12]) {
    for (int i = 0; i < 4; i++) {
        m1[3 * i] = a[i] * cam[0]; m1[3 * i + 1] = 0.0; m1[3 * i + 2] = a[i] * (cam[2] - u);
        m2[3 * i] = 0.0; m2[3 * i + 1] = a[i] * cam[1]; m2[3 * i + 2] = a[i] * (cam[3] - v);
    }
}

EPNP_HD double epnp_dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// The minimal-set basis: W holds the 8 rows of M in rows 0..7 of a 12 x 12 array; on return rows 8..11 are
// v[0..3].
EPNP_HD void epnp_null_basis_minimal(double* W) {
    for (int r = 0; r < 12; r++) {
        double* w = W + 12 * r;
        int piv = 0;
        if (r >= 8) {   // the column of the remaining projector with the largest diagonal
            double best = -1.0;
            for (int i = 0; i < 12; i++) {
                double d = 1.0;
                for (int s = 0; s < r; s++) d -= W[12 * s + i] * W[12 * s + i];
                if (d > best) { best = d; piv = i; }
            }
            for (int i = 0; i < 12; i++) w[i] = i == piv ? 1.0 : 0.0;
        }
        for (int pass = 0; pass < 2; pass++)
            for (int s = 0; s < r; s++) {
                const double* ws = W + 12 * s;
                double d = 0.0;
                for (int i = 0; i < 12; i++) d += ws[i] * w[i];
                for (int i = 0; i < 12; i++) w[i] -= d * ws[i];
            }
        double nn = 0.0;
        for (int i = 0; i < 12; i++) nn += w[i] * w[i];
        double inv = 1.0 / sqrt(nn);
        if (r >= 8 && w[piv] < 0) inv = -inv;
        for (int i = 0; i < 12; i++) w[i] *= inv;
    }
}

// The Refine basis: A = MtM (12 x 12, destroyed), V work; v (4 x 12) = the eigenvectors of the four smallest
// eigenvalues, ascending (lowest index first on a tie).
EPNP_HD void epnp_null_basis_refine(double* A, double* V, double* v) {
    epnp_jacobi(A, V, 12, EPNP_SWEEPS12);
    int used = 0;
    for (int t = 0; t < 4; t++) {
        int at = -1;
        for (int i = 0; i < 12; i++)
            if (!((used >> i) & 1) && (at < 0 || A[13 * i] < A[13 * at])) at = i;
        used |= 1 << at;
        epnp_signed_column(V, 12, at, v + 12 * t);
    }
}

// Least squares min |A x - b| of the 6 x NC A (row-major, destroyed; b destroyed) by Householder QR with the
// column scaled by its largest magnitude, as qr_solve (:864-955).
template <int NC>
EPNP_HD void epnp_qr_solve(double* A, double* b, double* x) {
    constexpr int NR = 6;
    double A1[NC], A2[NC];
    for (int i = 0; i < NC; i++) x[i] = 0.0;
    for (int k = 0; k < NC; k++) {
        double eta = 0.0;
        for (int i = k; i < NR; i++) eta = fmax(eta, fabs(A[i * NC + k]));
        if (!(eta > 0.0)) return;
        const double inv_eta = 1.0 / eta;
        double sum = 0.0;
        for (int i = k; i < NR; i++) {
            A[i * NC + k] *= inv_eta;
            sum += A[i * NC + k] * A[i * NC + k];
        }
        double sigma = sqrt(sum);
        if (A[k * NC + k] < 0) sigma = -sigma;
        A[k * NC + k] += sigma;
        A1[k] = sigma * A[k * NC + k];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < NC; j++) {
            double s = 0.0;
            for (int i = k; i < NR; i++) s += A[i * NC + k] * A[i * NC + j];
            const double tau = s / A1[k];
            for (int i = k; i < NR; i++) A[i * NC + j] -= tau * A[i * NC + k];
        }
    }
    for (int j = 0; j < NC; j++) {   // b <- Q^T b
        double tau = 0.0;
        for (int i = j; i < NR; i++) tau += A[i * NC + j] * b[i];
        tau /= A1[j];
        for (int i = j; i < NR; i++) b[i] -= tau * A[i * NC + j];
    }
    for (int i = NC - 1; i >= 0; i--) {   // x = R^-1 b
        double s = 0.0;
        for (int j = i + 1; j < NC; j++) s += A[i * NC + j] * x[j];
        x[i] = (b[i] - s) / A2[i];
    }
}

// compute_L_6x10 (:764-804) and compute_rho (:806-814).
EPNP_HD void epnp_L_rho(const double* v, const double cws[12], double L[60], double rho[6]) {
    double dv[4][6][3];
    for (int i = 0; i < 4; i++) {
        int a = 0, b = 1;
        for (int j = 0; j < 6; j++) {
            for (int c = 0; c < 3; c++) dv[i][j][c] = v[12 * i + 3 * a + c] - v[12 * i + 3 * b + c];
            if (++b > 3) { a++; b = a + 1; }
        }
    }
    for (int i = 0; i < 6; i++) {
        double* row = L + 10 * i;
        row[0] = epnp_dot3(dv[0][i], dv[0][i]);
        row[1] = 2.0 * epnp_dot3(dv[0][i], dv[1][i]);
        row[2] = epnp_dot3(dv[1][i], dv[1][i]);
        row[3] = 2.0 * epnp_dot3(dv[0][i], dv[2][i]);
        row[4] = 2.0 * epnp_dot3(dv[1][i], dv[2][i]);
        row[5] = epnp_dot3(dv[2][i], dv[2][i]);
        row[6] = 2.0 * epnp_dot3(dv[0][i], dv[3][i]);
        row[7] = 2.0 * epnp_dot3(dv[1][i], dv[3][i]);
        row[8] = 2.0 * epnp_dot3(dv[2][i], dv[3][i]);
        row[9] = epnp_dot3(dv[3][i], dv[3][i]);
    }
    int a = 0, b = 1;
    for (int j = 0; j < 6; j++) {
        double d = 0.0;
        for (int c = 0; c < 3; c++) d += (cws[3 * a + c] - cws[3 * b + c]) * (cws[3 * a + c] - cws[3 * b + c]);
        rho[j] = d;
        if (++b > 3) { a++; b = a + 1; }
    }
}

// find_betas_approx_1 / _2 / _3 (:665-762), which = 1, 2, 3.
EPNP_HD void epnp_betas_approx(int which, const double L[60], const double rho[6], double betas[4]) {
    double b[6];
    for (int i = 0; i < 6; i++) b[i] = rho[i];
    if (which == 1) {
        double A[24], x[4];
        const int col[4] = {0, 1, 3, 6};
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 4; j++) A[4 * i + j] = L[10 * i + col[j]];
        epnp_qr_solve<4>(A, b, x);
        const double sg = x[0] < 0 ? -1.0 : 1.0;
        betas[0] = sqrt(sg * x[0]);
        for (int j = 1; j < 4; j++) betas[j] = sg * x[j] / betas[0];
    } else if (which == 2) {
        double A[18], x[3];
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 3; j++) A[3 * i + j] = L[10 * i + j];
        epnp_qr_solve<3>(A, b, x);
        if (x[0] < 0) { betas[0] = sqrt(-x[0]); betas[1] = x[2] < 0 ? sqrt(-x[2]) : 0.0; }
        else { betas[0] = sqrt(x[0]); betas[1] = x[2] > 0 ? sqrt(x[2]) : 0.0; }
        if (x[1] < 0) betas[0] = -betas[0];
        betas[2] = 0.0; betas[3] = 0.0;
    } else {
        double A[30], x[5];
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 5; j++) A[5 * i + j] = L[10 * i + j];
        epnp_qr_solve<5>(A, b, x);
        if (x[0] < 0) { betas[0] = sqrt(-x[0]); betas[1] = x[2] < 0 ? sqrt(-x[2]) : 0.0; }
        else { betas[0] = sqrt(x[0]); betas[1] = x[2] > 0 ? sqrt(x[2]) : 0.0; }
        if (x[1] < 0) betas[0] = -betas[0];
        betas[2] = x[3] / betas[0];
        betas[3] = 0.0;
    }
}

// gauss_newton (:816-862): five steps.
EPNP_HD void epnp_gauss_newton(const double L[60], const double rho[6], double be[4]) {
    for (int it = 0; it < 5; it++) {
        double A[24], b[6], x[4];
        for (int i = 0; i < 6; i++) {
            const double* r = L + 10 * i;
            A[4 * i] = 2 * r[0] * be[0] + r[1] * be[1] + r[3] * be[2] + r[6] * be[3];
            A[4 * i + 1] = r[1] * be[0] + 2 * r[2] * be[1] + r[4] * be[2] + r[7] * be[3];
            A[4 * i + 2] = r[3] * be[0] + r[4] * be[1] + 2 * r[5] * be[2] + r[8] * be[3];
            A[4 * i + 3] = r[6] * be[0] + r[7] * be[1] + r[8] * be[2] + 2 * r[9] * be[3];
            b[i] = rho[i] - (r[0] * be[0] * be[0] + r[1] * be[0] * be[1] + r[2] * be[1] * be[1] + r[3] * be[0] * be[2] +
                             r[4] * be[1] * be[2] + r[5] * be[2] * be[2] + r[6] * be[0] * be[3] + r[7] * be[1] * be[3] +
                             r[8] * be[2] * be[3] + r[9] * be[3] * be[3]);
        }
        epnp_qr_solve<4>(A, b, x);
        for (int i = 0; i < 4; i++) be[i] += x[i];
    }
}

// The three candidates' betas (compute_pose, :507-517).
EPNP_HD void epnp_all_betas(const double* v, const double cws[12], double betas[12]) {
    double L[60], rho[6];
    epnp_L_rho(v, cws, L, rho);
    for (int w = 1; w <= 3; w++) {
        epnp_betas_approx(w, L, rho, betas + 4 * (w - 1));
        epnp_gauss_newton(L, rho, betas + 4 * (w - 1));
    }
}

// compute_ccs (:453-464).
EPNP_HD void epnp_ccs(const double be[4], const double* v, double ccs[12]) {
    for (int j = 0; j < 12; j++) ccs[j] = 0.0;
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 12; j++) ccs[j] += be[i] * v[12 * i + j];
}

EPNP_HD void epnp_pc(const double a[4], const double ccs[12], double pc[3]) {
    for (int j = 0; j < 3; j++) pc[j] = a[0] * ccs[j] + a[1] * ccs[3 + j] + a[2] * ccs[6 + j] + a[3] * ccs[9 + j];
}

EPNP_HD void epnp_inv3t(const double X[9], double Y[9]) {   // Y = X^-T
    const double c00 = X[4] * X[8] - X[5] * X[7], c01 = X[5] * X[6] - X[3] * X[8], c02 = X[3] * X[7] - X[4] * X[6];
    const double det = X[0] * c00 + X[1] * c01 + X[2] * c02, id = 1.0 / det;
    Y[0] = c00 * id; Y[1] = c01 * id; Y[2] = c02 * id;
    Y[3] = (X[2] * X[7] - X[1] * X[8]) * id; Y[4] = (X[0] * X[8] - X[2] * X[6]) * id; Y[5] = (X[1] * X[6] - X[0] * X[7]) * id;
    Y[6] = (X[1] * X[5] - X[2] * X[4]) * id; Y[7] = (X[2] * X[3] - X[0] * X[5]) * id; Y[8] = (X[0] * X[4] - X[1] * X[3]) * id;
}

// estimate_R_and_t (:609-627) from ABt and the two centroids.
EPNP_HD void epnp_R_t(const double abt[9], const double pc0[3], const double pw0[3], double R[9], double t[3]) {
    double X[9], Y[9];
    double f = 0.0;
    for (int i = 0; i < 9; i++) f += abt[i] * abt[i];
    f = 1.0 / sqrt(f);
    for (int i = 0; i < 9; i++) X[i] = abt[i] * f;
    for (int it = 0; it < EPNP_POLAR_STEPS; it++) {
        epnp_inv3t(X, Y);
        double nx = 0.0, ny = 0.0;
        for (int i = 0; i < 9; i++) { nx += X[i] * X[i]; ny += Y[i] * Y[i]; }
        const double g = sqrt(sqrt(ny / nx));
        for (int i = 0; i < 9; i++) X[i] = 0.5 * (g * X[i] + Y[i] / g);
    }
    for (int i = 0; i < 9; i++) R[i] = X[i];
    const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] -
                       R[0] * R[5] * R[7];
    if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
    for (int i = 0; i < 3; i++) t[i] = pc0[i] - epnp_dot3(R + 3 * i, pw0);
}

// One term of reprojection_error (:551-568).
EPNP_HD double epnp_reproj(const double R[9], const double t[3], const double cam[4], const double pw[3], double u, double v) {
    const double Xc = epnp_dot3(R, pw) + t[0], Yc = epnp_dot3(R + 3, pw) + t[1], inv_Zc = 1.0 / (epnp_dot3(R + 6, pw) + t[2]);
    const double ue = cam[2] + cam[0] * Xc * inv_Zc, ve = cam[3] + cam[1] * Yc * inv_Zc;
    return sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
}

// compute_pose on n correspondences, one after another.  pw (n x 3), us (n x 2); alphas: n x 4 work; W: 144
// work; V: 144 work (not touched when MINIMAL).  MINIMAL: n == 4 and the projector basis; else n >= 6 and the
// eigenvectors of MtM.
template <bool MINIMAL>
EPNP_HD void epnp_pose_serial(int n, const double* pw, const double* us, const double cam[4], double* alphas, double* W, double* V,
                              double R[9], double t[3]) {
    double c0[3] = {0, 0, 0}, S[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < n; i++)
        for (int j = 0; j < 3; j++) c0[j] += pw[3 * i + j];
    for (int j = 0; j < 3; j++) c0[j] /= n;
    for (int i = 0; i < n; i++) {
        const double x = pw[3 * i] - c0[0], y = pw[3 * i + 1] - c0[1], z = pw[3 * i + 2] - c0[2];
        S[0] += x * x; S[1] += x * y; S[2] += x * z; S[3] += y * y; S[4] += y * z; S[5] += z * z;
    }
    double cws[12], ci[9], v[48];
    epnp_control_points(S, n, c0, cws, ci);
    for (int i = 0; i < n; i++) epnp_alphas(ci, c0, pw + 3 * i, alphas + 4 * i);
    if (MINIMAL) {
        for (int i = 0; i < 4; i++) epnp_rows(alphas + 4 * i, us[2 * i], us[2 * i + 1], cam, W + 24 * i, W + 24 * i + 12);
        epnp_null_basis_minimal(W);
        for (int i = 0; i < 48; i++) v[i] = W[96 + i];
    } else {
        for (int i = 0; i < 144; i++) W[i] = 0.0;
        for (int i = 0; i < n; i++) {
            double m1[12], m2[12];
            epnp_rows(alphas + 4 * i, us[2 * i], us[2 * i + 1], cam, m1, m2);
            for (int r = 0; r < 12; r++)
                for (int c = r; c < 12; c++) W[12 * r + c] += m1[r] * m1[c] + m2[r] * m2[c];
        }
        for (int r = 0; r < 12; r++)
            for (int c = 0; c < r; c++) W[12 * r + c] = W[12 * c + r];
        epnp_null_basis_refine(W, V, v);
    }
    double betas[12];
    epnp_all_betas(v, cws, betas);
    double best = 0.0;
    for (int w = 0; w < 3; w++) {
        double ccs[12], pc[3];
        epnp_ccs(betas + 4 * w, v, ccs);
        epnp_pc(alphas, ccs, pc);
        if (pc[2] < 0.0)   // solve_for_sign (:637-650)
            for (int j = 0; j < 12; j++) ccs[j] = -ccs[j];
        double pc0[3] = {0, 0, 0}, pw0[3] = {0, 0, 0}, abt[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < n; i++) {
            epnp_pc(alphas + 4 * i, ccs, pc);
            for (int j = 0; j < 3; j++) { pc0[j] += pc[j]; pw0[j] += pw[3 * i + j]; }
        }
        for (int j = 0; j < 3; j++) { pc0[j] /= n; pw0[j] /= n; }
        for (int i = 0; i < n; i++) {
            epnp_pc(alphas + 4 * i, ccs, pc);
            for (int j = 0; j < 3; j++)
                for (int c = 0; c < 3; c++) abt[3 * j + c] += (pc[j] - pc0[j]) * (pw[3 * i + c] - pw0[c]);
        }
        double Rw[9], tw[3], err = 0.0;
        epnp_R_t(abt, pc0, pw0, Rw, tw);
        for (int i = 0; i < n; i++) err += epnp_reproj(Rw, tw, cam, pw + 3 * i, us[2 * i], us[2 * i + 1]);
        err /= n;
        if (w == 0 || err < best) {   // N = 1; if (e2 < e1) N = 2; if (e3 < e[N]) N = 3 (:519-521)
            best = err;
            for (int i = 0; i < 9; i++) R[i] = Rw[i];
            for (int i = 0; i < 3; i++) t[i] = tw[i];
        }
    }
}

// DUtils::Random::RandomInt(0, d - 1) of the raw rand() value r, clamped into [0, d - 1] (the device entry cannot
// refuse a draw outside [0, rand_max]).
EPNP_HD int epnp_random_int(int32_t r, int32_t rand_max, int d) {
    const int v = (int)(((double)r / ((double)rand_max + 1.0)) * d);
    return v < 0 ? 0 : (v > d - 1 ? d - 1 : v);
}

// The four draws of a hypothesis (:188-201) on mvAllIndices = 0 .. n - 1 without the vector: a position holds
// its own index until a draw takes it, after which it holds what was then the back.  n >= 4.
EPNP_HD void epnp_pick4(const int32_t* draw, int32_t rand_max, int n, int* idx) {
    int pos[4], val[4];
    for (int c = 0; c < 4; c++) {
        const int d = n - c, r = epnp_random_int(draw[c], rand_max, d);
        int at = r, back = d - 1;
        for (int j = 0; j < c; j++) {   // the latest refill of a position wins
            if (pos[j] == r) at = val[j];
            if (pos[j] == d - 1) back = val[j];
        }
        idx[c] = at;
        pos[c] = r;
        val[c] = back;
    }
}

// CheckInliers (:308-339) for one correspondence: float and double mixed as the reference writes them.
// X, p: P3Dw and P2D in float; cam: fu, fv, uc, vc in double (the solver's members are double, set from floats).
EPNP_HD bool epnp_is_inlier(const double R[9], const double t[3], const double cam[4], const float X[3], const float p[2], float max_error) {
    const float Xc = static_cast<float>(R[0] * X[0] + R[1] * X[1] + R[2] * X[2] + t[0]);
    const float Yc = static_cast<float>(R[3] * X[0] + R[4] * X[1] + R[5] * X[2] + t[1]);
    const float invZc = static_cast<float>(1 / (R[6] * X[0] + R[7] * X[1] + R[8] * X[2] + t[2]));
    const double ue = cam[2] + cam[0] * Xc * invZc;
    const double ve = cam[3] + cam[1] * Yc * invZc;
    const float distX = static_cast<float>(p[0] - ue);
    const float distY = static_cast<float>(p[1] - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < max_error;
}

}  // namespace orbamd
