// csrc/lm_newpoint.h on the CPU (tests/test_newpoints_native.py).  One request per line of stdin, one answer per line:
//   P Tcw1(12) cam1(6) Tcw2(12) cam2(6)                     -> F12(9) ep2(2) baseline
//   D Tcw2(12) cam2(6) monocular baseline n xyz(3n)         -> n median skip
//   M Tcw1 cam1 Tcw2 cam2 L scale1(L) sigma1(L) scale2(L) sigma2(L) ratio_factor kp1(5) kp2(5)
//                                                           -> status branch xw(3) normal(3) min_distance max_distance
// kp = u v uright depth octave.  Floats travel as 9 significant digits, which round-trip.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "lm_newpoint.h"

using namespace orbamd;

static void read_frame(std::istream& in, LmFrame& f) {
    float T[12], cam[6];
    for (float& v : T) in >> v;
    for (float& v : cam) in >> v;
    lm_frame(T, cam, f);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        char op;
        in >> op;
        if (op == 'P') {
            LmFrame f1, f2;
            read_frame(in, f1);
            read_frame(in, f2);
            float F12[9], ep2[2], baseline;
            lm_pair(f1, f2, F12, ep2, baseline);
            for (float v : F12) std::printf("%.9g ", v);
            std::printf("%.9g %.9g %.9g\n", ep2[0], ep2[1], baseline);
        } else if (op == 'D') {
            LmFrame f2;
            read_frame(in, f2);
            int mono, n;
            float baseline;
            in >> mono >> baseline >> n;
            std::vector<float> d(n);
            for (int i = 0; i < n; i++) {
                float X[3];
                in >> X[0] >> X[1] >> X[2];
                d[i] = lm_depth(f2, X);
            }
            std::sort(d.begin(), d.end());
            const float median = n ? d[(n - 1) / 2] : 0.f;
            std::printf("%d %.9g %d\n", n, median, lm_skip(mono != 0, baseline, f2, n, median) ? 1 : 0);
        } else if (op == 'M') {
            LmFrame f1, f2;
            read_frame(in, f1);
            read_frame(in, f2);
            LmTables t{};
            in >> t.n_levels;
            if (t.n_levels < 1 || t.n_levels > LM_MAX_LEVELS) return 2;
            for (int l = 0; l < t.n_levels; l++) in >> t.scale1[l];
            for (int l = 0; l < t.n_levels; l++) in >> t.sigma1[l];
            for (int l = 0; l < t.n_levels; l++) in >> t.scale2[l];
            for (int l = 0; l < t.n_levels; l++) in >> t.sigma2[l];
            in >> t.ratio_factor;
            float k[2][4];
            int o[2];
            for (int s = 0; s < 2; s++) in >> k[s][0] >> k[s][1] >> k[s][2] >> k[s][3] >> o[s];
            LmPoint r;
            lm_match(f1, f2, t, k[0][0], k[0][1], k[0][2], k[0][3], o[0], k[1][0], k[1][1], k[1][2], k[1][3], o[1], r);
            std::printf("%d %d %.9g %.9g %.9g %.9g %.9g %.9g %.9g %.9g\n", r.status, r.branch, r.xw[0], r.xw[1], r.xw[2], r.normal[0],
                        r.normal[1], r.normal[2], r.min_distance, r.max_distance);
        } else {
            return 2;
        }
        if (!in) return 3;
    }
    return 0;
}
