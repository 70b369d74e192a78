// csrc/eg_edge.h and csrc/sim3_g2o.h on the CPU for tests/test_essential_graph_native.py.  One command per line:
//   L q0 q1 q2 q3 t0 t1 t2 s                         -> log (7)
//   E C(8) v1(8) v2(8) fix_scale                     -> error (7), then both Jacobians (2 x 49, error row major)
//   M Siw(13) Sjw(13)                                -> the measurement (8)
//   R est(8) Srw(13) P(3)                            -> pose (12), corrected point (3)
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "eg_edge.h"

using namespace orbamd;

static S3 read_s3(std::istream& is) {
    S3 s;
    for (int k = 0; k < 4; k++) is >> s.q[k];
    for (int k = 0; k < 3; k++) is >> s.t[k];
    is >> s.s;
    return s;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream is(line);
        char cmd;
        is >> cmd;
        if (cmd == 'L') {
            const S3 a = read_s3(is);
            double r[7];
            s3_log(a, r);
            for (double v : r) std::printf("%.17g ", v);
        } else if (cmd == 'E') {
            const S3 C = read_s3(is), v1 = read_s3(is), v2 = read_s3(is);
            int fix = 0;
            is >> fix;
            double e[7];
            eg_error(C, v1, v2, e);
            for (double v : e) std::printf("%.17g ", v);
            const double delta = 1e-9, scalar = 1 / (2 * delta);
            for (int a = 0; a < 2; a++) {
                double J[7][7];
                for (int d = 0; d < 7; d++) {
                    double ep[7], em[7], u[7] = {0, 0, 0, 0, 0, 0, 0};
                    S3 P;
                    u[d] = delta;
                    eg_oplus(u, fix, a ? v2 : v1, P);
                    eg_error(C, a ? v1 : P, a ? P : v2, ep);
                    u[d] = -delta;
                    eg_oplus(u, fix, a ? v2 : v1, P);
                    eg_error(C, a ? v1 : P, a ? P : v2, em);
                    for (int r = 0; r < 7; r++) J[r][d] = scalar * (ep[r] - em[r]);
                }
                for (int r = 0; r < 7; r++)
                    for (int d = 0; d < 7; d++) std::printf("%.17g ", J[r][d]);
            }
        } else if (cmd == 'M') {
            float a[13], b[13];
            for (float& v : a) is >> v;
            for (float& v : b) is >> v;
            S3 m;
            eg_measurement(a, b, m);
            for (int k = 0; k < 4; k++) std::printf("%.17g ", m.q[k]);
            for (int k = 0; k < 3; k++) std::printf("%.17g ", m.t[k]);
            std::printf("%.17g ", m.s);
        } else if (cmd == 'R') {
            const S3 est = read_s3(is);
            float srw[13], P[3], pose[12], o[3];
            for (float& v : srw) is >> v;
            for (float& v : P) is >> v;
            F3 swc;
            eg_recover_pose(est, pose, swc);
            eg_correct_point(swc, srw, P, o);
            for (float v : pose) std::printf("%.9g ", v);
            for (float v : o) std::printf("%.9g ", v);
        }
        std::printf("\n");
    }
    return 0;
}
