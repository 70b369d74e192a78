// csrc/fr_undistort.h on the CPU (tests/test_frame_native.py): one request per line, floats as hex (a depth element as its
// bits), answered with the floats as their bits.
//   U <camera 4> <dist 5> <u> <v> <iters>          -> fr_undistort with that many iterations: x y
//   K <camera 4> <dist 5> <u> <v>                  -> fr_keypoint_xy (the k1 == 0 rule): x y
//   B <rows> <cols> <camera 4> <dist 5>            -> fr_image_bounds: minx maxx miny maxy
//   D <is_u16> <element bits> <factor> <x_un> <bf> -> fr_depth_value + fr_rgbd: uright depth
//   P <x> <y> <rows> <cols>                        -> fr_pixel: ok u v
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "fr_undistort.h"

using namespace orbamd;

static bool floats(std::istringstream& in, float* v, int n) {
    std::string tok;
    for (int i = 0; i < n; i++) {
        if (!(in >> tok)) return false;
        v[i] = (float)std::strtod(tok.c_str(), nullptr);
    }
    return true;
}

static uint32_t bits(float x) {
    uint32_t b;
    memcpy(&b, &x, 4);
    return b;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        if (op == "U" || op == "K") {
            float v[11], r[2];
            int iters = FR_ITERS;
            if (!floats(in, v, 11) || (op == "U" && !(in >> iters))) return 2;
            if (op == "U")
                fr_undistort(v, v + 4, v[9], v[10], r, iters);
            else
                fr_keypoint_xy(v, v + 4, v[9], v[10], r);
            std::printf("%u %u\n", bits(r[0]), bits(r[1]));
        } else if (op == "B") {
            int rows, cols;
            float v[9], b[4];
            if (!(in >> rows >> cols) || !floats(in, v, 9)) return 2;
            fr_image_bounds(rows, cols, v, v + 4, b);
            std::printf("%u %u %u %u\n", bits(b[0]), bits(b[1]), bits(b[2]), bits(b[3]));
        } else if (op == "D") {
            int is_u16;
            uint32_t raw;
            float v[3], ur, dp;
            if (!(in >> is_u16 >> raw) || !floats(in, v, 3)) return 2;
            const uint16_t raw16 = (uint16_t)raw;
            const float d = is_u16 ? fr_depth_value(&raw16, true, v[0]) : fr_depth_value(&raw, false, v[0]);
            fr_rgbd(d, v[1], v[2], ur, dp);
            std::printf("%u %u\n", bits(ur), bits(dp));
        } else if (op == "P") {
            float v[2];
            int rows, cols, pu = -1, pv = -1;
            if (!floats(in, v, 2) || !(in >> rows >> cols)) return 2;
            const bool ok = fr_pixel(v[0], v[1], rows, cols, pu, pv);
            std::printf("%d %d %d\n", ok ? 1 : 0, ok ? pu : -1, ok ? pv : -1);
        } else {
            return 2;
        }
    }
    return 0;
}
