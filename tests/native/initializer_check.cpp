// csrc/init_hyp.h on the CPU (tests/test_initializer_native.py): reads commands from stdin, one per record, and
// prints what the header computes, fp64 values before the narrowing as %.17g and floats as %.9g.
//   P rand_max n d0..d7                       -> the eight indices
//   H pn1(16) pn2(16) T1(4) T2(4)             -> Hn(9) H21i(9) H12i(9, of the float H21i)
//   F pn1(16) pn2(16) T1(4) T2(4)             -> Fpre(9) Fn(9) F21i(9)
//   I M(9)                                    -> the inverse of the float M, fp64
//   S model sigma M(9) Minv(9) n pts(4n)      -> score, then the mask
//   T R(9) t(3) cam(4) n pts(4n)              -> per point: x(3), counted, good, cosParallax, p3d(3)
//   E F21(9) cam(4)                           -> R1(9) R2(9) t(3)
//   D H21(9) cam(4)                           -> ok, then R(9) t(3) of the eight hypotheses
#include <cstdio>
#include <vector>

#include "init_hyp.h"

using namespace orbamd;

static bool rd(float* v, int n) {
    for (int i = 0; i < n; i++) {
        double d;
        if (std::scanf("%lf", &d) != 1) return false;
        v[i] = (float)d;
    }
    return true;
}
static void pd(const double* v, int n) { for (int i = 0; i < n; i++) std::printf("%.17g ", v[i]); }
static void pf(const float* v, int n) { for (int i = 0; i < n; i++) std::printf("%.9g ", v[i]); }

int main() {
    char op;
    while (std::scanf(" %c", &op) == 1) {
        if (op == 'P') {
            int rand_max, n, d[8], idx[8];
            if (std::scanf("%d %d", &rand_max, &n) != 2) return 2;
            for (int j = 0; j < 8; j++) if (std::scanf("%d", &d[j]) != 1) return 2;
            ini_pick8(d, rand_max, n, idx);
            for (int j = 0; j < 8; j++) std::printf("%d ", idx[j]);
        } else if (op == 'H' || op == 'F') {
            float pn1[16], pn2[16], T1[4], T2[4];
            if (!rd(pn1, 16) || !rd(pn2, 16) || !rd(T1, 4) || !rd(T2, 4)) return 2;
            if (op == 'H') {
                double Hn[9], H[9], Hi[9];
                float Hf[9];
                ini_compute_h21(pn1, pn2, Hn);
                ini_h21i(T1, T2, Hn, H);
                ini_round9(H, Hf);
                ini_inv3f(Hf, Hi);
                pd(Hn, 9); pd(H, 9); pd(Hi, 9);
            } else {
                double Fpre[9], Fn[9], F[9];
                ini_compute_f21(pn1, pn2, Fpre, Fn);
                ini_f21i(T1, T2, Fn, F);
                pd(Fpre, 9); pd(Fn, 9); pd(F, 9);
            }
        } else if (op == 'I') {
            float M[9];
            double I[9];
            if (!rd(M, 9)) return 2;
            ini_inv3f(M, I);
            pd(I, 9);
        } else if (op == 'S') {
            int model, n;
            float sigma, M[9], Mi[9];
            if (std::scanf("%d", &model) != 1 || !rd(&sigma, 1) || !rd(M, 9) || !rd(Mi, 9) || std::scanf("%d", &n) != 1) return 2;
            std::vector<float> pts(4 * (size_t)n);
            if (!rd(pts.data(), 4 * n)) return 2;
            const float inv = 1.f / (sigma * sigma);
            float score = 0;
            std::vector<int> in(n);
            for (int c = 0; c < n; c++) {
                const float* q = &pts[4 * (size_t)c];
                in[c] = model == 0 ? ini_check_h(M, Mi, q[0], q[1], q[2], q[3], inv, score) : ini_check_f(M, q[0], q[1], q[2], q[3], inv, score);
            }
            std::printf("%.9g ", score);
            for (int c = 0; c < n; c++) std::printf("%d ", in[c]);
        } else if (op == 'T') {
            float R[9], t[3], cam[4];
            int n;
            if (!rd(R, 9) || !rd(t, 3) || !rd(cam, 4) || std::scanf("%d", &n) != 1) return 2;
            std::vector<float> pts(4 * (size_t)n);
            if (!rd(pts.data(), 4 * n)) return 2;
            IniView v;
            ini_view(R, t, cam, v);
            for (int c = 0; c < n; c++) {
                const float* q = &pts[4 * (size_t)c];
                double x[3];
                ini_triangulate(v.P1, v.P2, q[0], q[1], q[2], q[3], x);
                float p3d[3], cp;
                bool good;
                const bool counted = ini_check_rt(v, q[0], q[1], q[2], q[3], 4.f, p3d, cp, good);
                pd(x, 3);
                std::printf("%d %d %.9g ", counted ? 1 : 0, good ? 1 : 0, cp);
                pf(p3d, 3);
            }
        } else if (op == 'E') {
            float F[9], cam[4], R1[9], R2[9], t[3];
            if (!rd(F, 9) || !rd(cam, 4)) return 2;
            ini_decompose_e(F, cam, R1, R2, t);
            pf(R1, 9); pf(R2, 9); pf(t, 3);
        } else if (op == 'D') {
            float H[9], cam[4], R[72], t[24];
            if (!rd(H, 9) || !rd(cam, 4)) return 2;
            const bool ok = ini_decompose_h(H, cam, R, t);
            std::printf("%d ", ok ? 1 : 0);
            for (int h = 0; h < 8; h++) { pf(R + 9 * h, 9); pf(t + 3 * h, 3); }
        } else {
            return 3;
        }
        std::printf("\n");
    }
    return 0;
}
