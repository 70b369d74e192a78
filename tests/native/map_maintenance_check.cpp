// csrc/mm_normal.h and csrc/mm_connect.h on the CPU (tests/test_map_maintenance_native.py), with the one-lane group MmOne.
//   map_maintenance_check connect|normal [time] < tables
// The tables are lines "name count v0 v1 ..." of int32 values (floats as their bits; uint8 arrays widened).  "connect" reads a
// graph and `item`, runs the batch as orbmm.hip does (the counters, the item summaries, then one walk and commit per
// keyframe) and prints the state arrays and status; "normal" reads the point tables, `scale` and optionally `point`, and
// prints mp_normal and mp_max_min as bits.  With "time" only the milliseconds of the computation are printed.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "mm_connect.h"
#include "mm_normal.h"

using namespace orbamd;
using Tables = std::map<std::string, std::vector<int32_t>>;

static std::vector<uint8_t> bytes(const std::vector<int32_t>& v) { return std::vector<uint8_t>(v.begin(), v.end()); }

static std::vector<float> floats(const std::vector<int32_t>& v) {
    std::vector<float> f(v.size());
    if (!v.empty()) std::memcpy(f.data(), v.data(), 4 * v.size());
    return f;
}

static void print_bits(const char* name, const std::vector<float>& f) {
    std::printf("%s %zu", name, f.size());
    for (float x : f) {
        int32_t b;
        std::memcpy(&b, &x, 4);
        std::printf(" %d", b);
    }
    std::printf("\n");
}

static void print(const char* name, const int32_t* v, size_t n) {
    std::printf("%s %zu", name, n);
    for (size_t i = 0; i < n; i++) std::printf(" %d", v[i]);
    std::printf("\n");
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

static int connect(Tables& t, bool time) {
    MmGraph g{};
    g.K = (int)t["kf_id"].size();
    g.M = (int)t["mp_bad"].size();
    g.kf_cap = g.K ? (int)(t["kf_mappoint"].size() / g.K) : 1;
    g.conn_cap = g.K ? (int)(t["conn_slot"].size() / g.K) : 1;
    g.n_obs = (int)t["mp_obs_kf"].size();
    std::vector<uint8_t> bad = bytes(t["mp_bad"]), first = bytes(t["kf_first_connection"]);
    std::vector<int32_t> status(g.K, 0);
    g.kf_id = t["kf_id"].data(); g.kf_n = t["kf_n"].data(); g.kf_mappoint = t["kf_mappoint"].data(); g.mp_bad = bad.data();
    g.mp_obs_off = t["mp_obs_off"].data(); g.mp_obs_kf = t["mp_obs_kf"].data();
    g.conn_slot = t["conn_slot"].data(); g.conn_weight = t["conn_weight"].data(); g.n_conn = t["n_conn"].data();
    g.ord_slot = t["ord_slot"].data(); g.ord_weight = t["ord_weight"].data(); g.n_ord = t["n_ord"].data();
    g.first = first.data(); g.parent = t["kf_parent"].data(); g.covis = t["kf_covis"].data(); g.status = status.data();
    const std::vector<int32_t>& item = t["item"];
    const int B = (int)item.size(), K = g.K;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> cnt((size_t)B * K, 0), ws(g.conn_cap), ww(g.conn_cap);
    std::vector<MmItem> items(B);
    const MmOne one;
    for (int i = 0; i < B; i++) {
        const int k = item[i];
        int32_t* row = cnt.data() + (size_t)i * K;
        if (k >= 0 && k < K)
            for (int j = 0; j < g.kf_cap; j++) {
                const int p = mm_counted_point(g, k, j);
                if (p < 0) continue;
                int e0, e1;
                mm_obs_range(g, p, e0, e1);
                for (int e = e0; e < e1; e++)
                    if (mm_counted_observer(g, k, g.mp_obs_kf[e])) row[g.mp_obs_kf[e]]++;
            }
        items[i] = mm_item_summary(one, row, K, k);
    }
    for (int X = 0; X < K; X++) {
        const MmWalk r = mm_walk(one, g, X, B, items.data(), cnt.data(), ws.data(), ww.data());
        mm_commit(one, g, X, items.data(), ws.data(), ww.data(), r);
    }
    if (time) {
        std::printf("%.3f\n", ms_since(t0));
        return 0;
    }
    std::vector<int32_t> f(first.begin(), first.end());
    for (const char* name : {"conn_slot", "conn_weight", "n_conn", "ord_slot", "ord_weight", "n_ord", "kf_parent", "kf_covis"})
        print(name, t[name].data(), t[name].size());
    print("kf_first_connection", f.data(), f.size());
    print("status", status.data(), status.size());
    return 0;
}

static int normal(Tables& t, bool time) {
    MmPoints p{};
    p.K = (int)t["kf_n"].size();
    p.M = (int)t["mp_bad"].size();
    p.kf_cap = p.K ? (int)(t["kf_kp_octave"].size() / p.K) : 1;
    p.n_obs = (int)t["mp_obs_kf"].size();
    p.n_levels = (int)t["scale"].size();
    if (p.n_levels < 1 || p.n_levels > MM_MAX_LEVELS) return 2;
    std::vector<uint8_t> bad = bytes(t["mp_bad"]);
    static_assert(sizeof(float) == sizeof(int32_t), "");
    std::vector<float> ow(3 * (size_t)p.K), xw = floats(t["mp_xw"]), pose = floats(t["kf_pose"]), nrm = floats(t["mp_normal"]),
                       mm = floats(t["mp_max_min"]), scale = floats(t["scale"]);
    p.mp_bad = bad.data(); p.mp_xw = xw.data(); p.mp_ref_kf = t["mp_ref_kf"].data();
    p.mp_obs_off = t["mp_obs_off"].data(); p.mp_obs_kf = t["mp_obs_kf"].data(); p.mp_obs_idx = t["mp_obs_idx"].data();
    p.kf_n = t["kf_n"].data(); p.kf_kp_octave = t["kf_kp_octave"].data(); p.kf_ow = ow.data();
    p.mp_normal = nrm.data(); p.mp_max_min = mm.data();
    for (int l = 0; l < p.n_levels; l++) p.scale[l] = scale[l];
    const auto t0 = std::chrono::steady_clock::now();
    for (int k = 0; k < p.K; k++) mm_center(pose.data() + 12 * (size_t)k, ow.data() + 3 * (size_t)k);
    if (t.count("point"))
        for (int32_t q : t["point"]) mm_update_point(p, q);
    else
        for (int q = 0; q < p.M; q++) mm_update_point(p, q);
    if (time) {
        std::printf("%.3f\n", ms_since(t0));
        return 0;
    }
    print_bits("mp_normal", nrm);
    print_bits("mp_max_min", mm);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    Tables t;
    std::string name;
    size_t n;
    while (std::cin >> name >> n) {
        std::vector<int32_t>& v = t[name];
        v.resize(n);
        for (size_t i = 0; i < n; i++) {
            long long x;
            if (!(std::cin >> x)) return 2;
            v[i] = (int32_t)x;
        }
    }
    const bool time = argc > 2 && std::string(argv[2]) == "time";
    return std::string(argv[1]) == "connect" ? connect(t, time) : normal(t, time);
}
