// csrc/gba_update.h on the CPU (tests/test_global_ba_native.py).  One case per input line, its numbers as hex
// floats: "C" child pose, parent pose, parent TcwGBA (12 each) -> the child's TcwGBA; "P" TcwBefGBA, new pose
// (12 each), X (3) -> the moved point.  Prints the results' float bits.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "gba_update.h"

static uint32_t bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op, tok;
        if (!(in >> op)) continue;
        std::vector<float> v;
        while (in >> tok) v.push_back((float)std::strtod(tok.c_str(), nullptr));
        float o[12];
        int n = 0;
        if (op == "C" && v.size() == 36) {
            orbamd::gba_child_pose(&v[0], &v[12], &v[24], o);
            n = 12;
        } else if (op == "P" && v.size() == 27) {
            orbamd::gba_move_point(&v[0], &v[12], &v[24], o);
            n = 3;
        } else {
            std::fprintf(stderr, "bad line: %s\n", line.c_str());
            return 2;
        }
        for (int k = 0; k < n; k++) std::printf("%u%c", bits(o[k]), k + 1 == n ? '\n' : ' ');
    }
    return 0;
}
