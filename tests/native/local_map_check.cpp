// csrc/tl_frustum.h on the CPU (tests/test_local_map_native.py): one line per point,
//   <29 hex floats: pose 12, camera 5, bounds 4, Xw 3, normal 3, maxDistance, minDistance> <min_view_cos> <log_sf> <n_levels>
// answered by "fail u v ur view_cos level" with the floats as their bits.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "tl_frustum.h"

static unsigned bits(float x) {
    unsigned u;
    std::memcpy(&u, &x, 4);
    return u;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string tok;
        float v[31];
        for (int i = 0; i < 31; i++) {
            if (!(in >> tok)) return 2;
            v[i] = (float)std::strtod(tok.c_str(), nullptr);
        }
        int n_levels;
        if (!(in >> n_levels)) return 2;
        const orbamd::TlPoint r = orbamd::tl_frustum(v, v + 12, v + 17, v + 21, v + 24, v[27], v[28], v[29], v[30], n_levels);
        std::printf("%d %u %u %u %u %d\n", r.fail, bits(r.u), bits(r.v), bits(r.ur), bits(r.view_cos), r.level);
    }
    return 0;
}
