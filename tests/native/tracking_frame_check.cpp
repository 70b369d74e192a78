// csrc/tf_frame.h on the CPU (tests/test_tracking_frame_native.py): one request per line, floats as hex, answered with
// the floats as their bits.
//   P <velocity 12> <last pose 12> <baseline> <monocular>     -> the 12 floats of the product, then the motion
//   J <pose 12> <camera 5> <bounds 4> <Xw 3>                   -> valid u v ur
//   U <pose 12> <camera 5> <u> <v> <Z> <vo>                    -> the world point
//   R <th_depth> <by_index> <n> <n depths as uint32 bits>      -> n_processed, then the rank of each depth (-1: left out)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "tf_frame.h"

using namespace orbamd;

static bool floats(std::istringstream& in, float* v, int n) {
    std::string tok;
    for (int i = 0; i < n; i++) {
        if (!(in >> tok)) return false;
        v[i] = (float)std::strtod(tok.c_str(), nullptr);
    }
    return true;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        if (op == "P") {
            float v[25], C[12];
            int mono;
            if (!floats(in, v, 25) || !(in >> mono)) return 2;
            tf_pose_product(v, v + 12, C);
            for (int i = 0; i < 12; i++) std::printf("%u ", tf_bits(C[i]));
            std::printf("%d\n", tf_motion(v + 12, C, v[24], mono != 0));
        } else if (op == "J") {
            float v[24];
            if (!floats(in, v, 24)) return 2;
            const TfProj r = tf_project(v, v + 12, v + 17, v + 21);
            std::printf("%d %u %u %u\n", r.valid, tf_bits(r.u), tf_bits(r.v), tf_bits(r.ur));
        } else if (op == "U") {
            float v[20], X[3];
            int vo;
            if (!floats(in, v, 20) || !(in >> vo)) return 2;
            tf_unproject(v, v + 12, v[17], v[18], v[19], vo != 0, X);
            std::printf("%u %u %u\n", tf_bits(X[0]), tf_bits(X[1]), tf_bits(X[2]));
        } else if (op == "R") {
            float th;
            int by_index, n;
            if (!floats(in, &th, 1) || !(in >> by_index >> n) || n < 0) return 2;
            std::vector<uint32_t> z(n), w(n);
            int n_valid = 0, n_close = 0;
            for (int i = 0; i < n; i++) {
                if (!(in >> z[i])) return 2;
                w[i] = tf_depth_word(z[i], by_index != 0);
                if (w[i] != TF_WORD_NONE) {
                    n_valid++;
                    if (!tf_depth_far(z[i], th)) n_close++;
                }
            }
            std::printf("%d", by_index ? n_valid : tf_n_processed(n_valid, n_close));
            for (int i = 0; i < n; i++) {
                int rank = 0;
                for (int j = 0; j < n; j++) rank += tf_depth_before(w[j], j, w[i], i) ? 1 : 0;
                std::printf(" %d", w[i] == TF_WORD_NONE ? -1 : rank);
            }
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
