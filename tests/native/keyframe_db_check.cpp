// csrc/db_score.h stand-alone on the CPU (tests/test_keyframe_db_native.py): one request per input line, one answer per
// output line.  Floating-point values travel as hexadecimal literals, answers as raw bits.
//   S n1 n2 w1[n1] v1[n1] w2[n2] v2[n2]        -> <score as double bits> <common words>
//   W maxw                                      -> <minw>
//   G k score_k K covis[10] member[K] val[K]    -> <acc as float bits> <bestk>
//   R acc best_acc                              -> <0|1>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "db_score.h"

static double next_double(std::istringstream& in) {
    std::string t;
    in >> t;
    return std::strtod(t.c_str(), nullptr);
}

int main() {
    using namespace orbamd;
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        char op;
        in >> op;
        if (op == 'S') {
            int n1, n2;
            in >> n1 >> n2;
            std::vector<uint32_t> w1(n1), w2(n2);
            std::vector<double> v1(n1), v2(n2);
            for (auto& x : w1) in >> x;
            for (auto& x : v1) x = next_double(in);
            for (auto& x : w2) in >> x;
            for (auto& x : v2) x = next_double(in);
            int common = -1;
            const double s = db_score(w1.data(), v1.data(), n1, w2.data(), v2.data(), n2, &common);
            uint64_t bits;
            std::memcpy(&bits, &s, 8);
            std::printf("%" PRIu64 " %d\n", bits, common);
        } else if (op == 'W') {
            int maxw;
            in >> maxw;
            std::printf("%d\n", db_minw(maxw));
        } else if (op == 'G') {
            int k, K;
            in >> k;
            const float score_k = (float)next_double(in);
            in >> K;
            int32_t covis[DB_COVIS];
            for (auto& x : covis) in >> x;
            std::vector<uint8_t> member(K);
            std::vector<float> val(K);
            for (auto& x : member) { int m; in >> m; x = (uint8_t)m; }
            for (auto& x : val) x = (float)next_double(in);
            const DbGroup g = db_group_walk(k, score_k, covis, K, member.data(), val.data());
            uint32_t bits;
            std::memcpy(&bits, &g.acc, 4);
            std::printf("%u %d\n", bits, g.bestk);
        } else if (op == 'R') {
            const float acc = (float)next_double(in), best = (float)next_double(in);
            std::printf("%d\n", db_retained(acc, best) ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}
