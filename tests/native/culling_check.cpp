// csrc/mm_cull.h on the CPU (tests/test_culling_native.py), with the one-lane group MmOne for both of its groups.
//   culling_check points|keyframes|compact [time] < tables
// The tables are lines "name count v0 v1 ..." of int32 values (floats as their bits; uint8 arrays widened), scalars as
// arrays of one.  "points" reads the map, `recent`, `cur_kf_id` and `monocular` and prints mp_bad, kf_mappoint, mp_obs_kf,
// recent and n_recent; "keyframes" reads the map, `cur`, `monocular` and `th_depth` and prints every updated table, culled,
// n_culled and status; "compact" prints the compacted CSR.  With "time" only the milliseconds of the computation are
// printed.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "mm_cull.h"

using namespace orbamd;
using Tables = std::map<std::string, std::vector<int32_t>>;

static std::vector<uint8_t> bytes(const std::vector<int32_t>& v) { return std::vector<uint8_t>(v.begin(), v.end()); }

static std::vector<float> floats(const std::vector<int32_t>& v) {
    static_assert(sizeof(float) == sizeof(int32_t), "");
    std::vector<float> f(v.size());
    if (!v.empty()) std::memcpy(f.data(), v.data(), 4 * v.size());
    return f;
}

static float as_float(int32_t b) {
    float f;
    std::memcpy(&f, &b, 4);
    return f;
}

static void print(const char* name, const int32_t* v, size_t n) {
    std::printf("%s %zu", name, n);
    for (size_t i = 0; i < n; i++) std::printf(" %d", v[i]);
    std::printf("\n");
}

static void print_bytes(const char* name, const std::vector<uint8_t>& v) {
    std::vector<int32_t> w(v.begin(), v.end());
    print(name, w.data(), w.size());
}

static void print_bits(const char* name, const std::vector<float>& f) {
    std::vector<int32_t> b(f.size());
    if (!f.empty()) std::memcpy(b.data(), f.data(), 4 * f.size());
    print(name, b.data(), b.size());
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct Map {
    MmCull c{};
    std::vector<uint8_t> kf_bad, not_erase, to_be_erased, mp_bad;
    std::vector<float> uright, depth, pose, tcp;
    explicit Map(Tables& t) {
        c.K = (int)t["kf_n"].size();
        c.M = (int)t["mp_bad"].size();
        c.kf_cap = c.K ? (int)(t["kf_mappoint"].size() / c.K) : 1;
        c.conn_cap = c.K && t.count("conn_slot") ? (int)(t["conn_slot"].size() / c.K) : 1;
        c.n_obs = (int)t["mp_obs_kf"].size();
        kf_bad = bytes(t["kf_bad"]); not_erase = bytes(t["kf_not_erase"]); to_be_erased = bytes(t["kf_to_be_erased"]);
        mp_bad = bytes(t["mp_bad"]);
        uright = floats(t["kf_uright"]); depth = floats(t["kf_depth"]); pose = floats(t["kf_pose"]); tcp = floats(t["kf_tcp"]);
        c.kf_id = t["kf_id"].data(); c.kf_n = t["kf_n"].data(); c.kf_mappoint = t["kf_mappoint"].data();
        c.kf_kp_octave = t["kf_kp_octave"].data(); c.kf_uright = uright.data(); c.kf_depth = depth.data();
        c.kf_pose = pose.data(); c.kf_bad = kf_bad.data(); c.kf_not_erase = not_erase.data();
        c.kf_to_be_erased = to_be_erased.data(); c.kf_tcp = tcp.data(); c.mp_bad = mp_bad.data();
        c.mp_nobs = t["mp_nobs"].data(); c.mp_found = t["mp_found"].data(); c.mp_visible = t["mp_visible"].data();
        c.mp_first_kf_id = t["mp_first_kf_id"].data(); c.mp_ref_kf = t["mp_ref_kf"].data();
        c.mp_obs_off = t["mp_obs_off"].data(); c.mp_obs_kf = t["mp_obs_kf"].data(); c.mp_obs_idx = t["mp_obs_idx"].data();
        c.conn_slot = t["conn_slot"].data(); c.conn_weight = t["conn_weight"].data(); c.n_conn = t["n_conn"].data();
        c.ord_slot = t["ord_slot"].data(); c.ord_weight = t["ord_weight"].data(); c.n_ord = t["n_ord"].data();
        c.kf_parent = t["kf_parent"].data(); c.kf_covis = t["kf_covis"].data();
    }
};

static int points(Tables& t, bool time) {
    Map m(t);
    std::vector<int32_t>& recent = t["recent"];
    if (t["cur_kf_id"].empty() || t["monocular"].empty()) return 2;
    const int cur_kf_id = t["cur_kf_id"][0], min_obs = t["monocular"][0] ? 2 : 3;
    const auto t0 = std::chrono::steady_clock::now();
    int32_t n = 0;
    for (size_t i = 0; i < recent.size(); i++) {
        const int p = recent[i], d = cull_point_decision(m.c, p, cur_kf_id, min_obs);
        if (d == CULL_BAD) cull_set_bad(m.c, p);
        if (d == CULL_KEEP) recent[n++] = p;
    }
    if (time) {
        std::printf("%.3f\n", ms_since(t0));
        return 0;
    }
    print_bytes("mp_bad", m.mp_bad);
    print("kf_mappoint", t["kf_mappoint"].data(), t["kf_mappoint"].size());
    print("mp_obs_kf", t["mp_obs_kf"].data(), t["mp_obs_kf"].size());
    print("recent", recent.data(), recent.size());
    print("n_recent", &n, 1);
    return 0;
}

static int keyframes(Tables& t, bool time) {
    Map m(t);
    if (t["cur"].empty() || t["monocular"].empty() || t["th_depth"].empty()) return 2;
    std::vector<int32_t> culled(m.c.conn_cap, 0), scratch(cull_scratch_entries(m.c.K, m.c.conn_cap, 1), 0);
    int32_t n_culled = -1, status = -1;
    const MmOne one;
    const auto t0 = std::chrono::steady_clock::now();
    cull_keyframes(one, one, 0, 1, m.c, t["cur"][0], t["monocular"][0] != 0, as_float(t["th_depth"][0]), culled.data(), &n_culled,
                   &status, scratch.data());
    if (time) {
        std::printf("%.3f\n", ms_since(t0));
        return 0;
    }
    print_bytes("kf_bad", m.kf_bad);
    print_bytes("kf_to_be_erased", m.to_be_erased);
    print_bits("kf_tcp", m.tcp);
    print_bytes("mp_bad", m.mp_bad);
    for (const char* name : {"kf_mappoint", "mp_nobs", "mp_ref_kf", "mp_obs_kf", "conn_slot", "conn_weight", "n_conn", "ord_slot",
                             "ord_weight", "n_ord", "kf_parent", "kf_covis"})
        print(name, t[name].data(), t[name].size());
    print("culled", culled.data(), culled.size());
    print("n_culled", &n_culled, 1);
    print("status", &status, 1);
    return 0;
}

static int compact(Tables& t, bool time) {
    const std::vector<int32_t>&off = t["mp_obs_off"], &kf = t["mp_obs_kf"], &idx = t["mp_obs_idx"];
    if (off.empty() || kf.size() != idx.size()) return 2;
    const int M = (int)off.size() - 1, n_obs = (int)kf.size();
    std::vector<int32_t> out_off(M + 1, 0), out_kf(kf), out_idx(idx);
    const auto t0 = std::chrono::steady_clock::now();
    int at = 0;
    for (int p = 0; p < M; p++) {
        out_off[p] = at;
        at += cull_compact_point(n_obs, off.data(), kf.data(), idx.data(), p, at, out_kf.data(), out_idx.data());
    }
    out_off[M] = at;
    if (time) {
        std::printf("%.3f\n", ms_since(t0));
        return 0;
    }
    print("mp_obs_off", out_off.data(), out_off.size());
    print("mp_obs_kf", out_kf.data(), out_kf.size());
    print("mp_obs_idx", out_idx.data(), out_idx.size());
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
    const std::string mode = argv[1];
    if (mode == "points") return points(t, time);
    if (mode == "keyframes") return keyframes(t, time);
    if (mode == "compact") return compact(t, time);
    return 2;
}
