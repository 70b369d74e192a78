// csrc/mm_observe.h on the CPU (tests/test_observe_native.py), with the one-lane group MmOne.
//   observe_check apply|new|grow [time] < tables
// The tables are lines "name count v0 v1 ..." of int32 values (floats as their bits; uint8 arrays widened), scalars as
// arrays of one.  "apply" reads the map, `mode`, item_kf, mp_begin, point, best_idx, replace_point, n_fused, touched,
// n_touched and progress and prints every updated table and output; "new" reads the map and `cur` and prints mp_nobs,
// the CSR, added, recent_out, counts and status; "grow" reads the CSR, `slack`, `n_obs_out` and optionally `extra` and
// prints the grown CSR and status.  With "time" only the milliseconds of the computation are printed.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "mm_observe.h"

using namespace orbamd;
using Tables = std::map<std::string, std::vector<int32_t>>;

static void print(const char* name, const int32_t* v, size_t n) {
    std::printf("%s %zu", name, n);
    for (size_t i = 0; i < n; i++) std::printf(" %d", v[i]);
    std::printf("\n");
}

static void print(const char* name, const std::vector<int32_t>& v) { print(name, v.data(), v.size()); }

static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

struct Map {
    MmObserve o{};
    std::vector<uint8_t> mp_bad;
    std::vector<float> uright;
    explicit Map(Tables& t) {
        o.K = (int)t["kf_n"].size();
        o.M = (int)t["mp_bad"].size();
        o.kf_cap = o.K ? (int)(t["kf_mappoint"].size() / o.K) : 1;
        o.n_obs = (int)t["mp_obs_kf"].size();
        mp_bad.assign(t["mp_bad"].begin(), t["mp_bad"].end());
        uright.resize(t["kf_uright"].size());
        if (!uright.empty()) std::memcpy(uright.data(), t["kf_uright"].data(), 4 * uright.size());
        o.kf_n = t["kf_n"].data(); o.kf_mappoint = t["kf_mappoint"].data(); o.kf_uright = uright.data();
        o.mp_bad = mp_bad.data(); o.mp_nobs = t["mp_nobs"].data(); o.mp_found = t["mp_found"].data();
        o.mp_visible = t["mp_visible"].data(); o.mp_replaced = t["mp_replaced"].data(); o.mp_obs_off = t["mp_obs_off"].data();
        o.mp_obs_kf = t["mp_obs_kf"].data(); o.mp_obs_idx = t["mp_obs_idx"].data();
    }
    void print_bad() const {
        std::vector<int32_t> w(mp_bad.begin(), mp_bad.end());
        print("mp_bad", w);
    }
};

static int apply(Tables& t, bool time) {
    Map m(t);
    if (t["mode"].empty() || t["progress"].size() != 4 || t["n_touched"].empty() || t["mp_begin"].empty()) return 2;
    MmApply a{};
    a.mode = t["mode"][0];
    a.n_items = (int)t["item_kf"].size();
    a.n_entries = (int)t["point"].size();
    if (t["mp_begin"].size() != (size_t)a.n_items + 1 || t["best_idx"].size() != t["point"].size() ||
        t["replace_point"].size() != t["point"].size() || t["n_fused"].size() != (size_t)a.n_items)
        return 2;
    t["touched"].resize(m.o.M, 0);
    int32_t status = -1;
    a.item_kf = t["item_kf"].data(); a.mp_begin = t["mp_begin"].data(); a.point = t["point"].data(); a.best_idx = t["best_idx"].data();
    a.replace_point = t["replace_point"].data(); a.n_fused = t["n_fused"].data(); a.touched = t["touched"].data();
    a.n_touched = t["n_touched"].data(); a.progress = t["progress"].data(); a.status = &status;
    std::vector<int32_t> ws(obs_scratch_entries(m.o.M, m.o.n_obs) + 1, 0);
    int32_t chunk[1] = {0};
    const MmOne one;
    const auto t0 = std::chrono::steady_clock::now();
    obs_fuse_apply(one, m.o, a, chunk, ws.data());
    if (time) {
        std::printf("%.3f\n", ms_since(t0));
        return 0;
    }
    m.print_bad();
    for (const char* name : {"kf_mappoint", "mp_nobs", "mp_found", "mp_visible", "mp_replaced", "mp_obs_kf", "mp_obs_idx", "n_fused",
                             "replace_point", "touched", "n_touched", "progress"})
        print(name, t[name]);
    print("status", &status, 1);
    return 0;
}

static int new_keyframe(Tables& t, bool time) {
    Map m(t);
    if (t["cur"].empty()) return 2;
    const int cur = t["cur"][0], cap = m.o.kf_cap;
    std::vector<int32_t> added(cap, -1), recent(cap, -1), status(cap, 0), counts(2, 0);
    const auto t0 = std::chrono::steady_clock::now();
    if (cur >= 0 && cur < m.o.K)
        for (int i = 0; i < cap; i++) {
            const int kind = obs_new_keyframe_entry(m.o, cur, i, status[i]);
            if (kind == OBS_ADDED) added[counts[0]++] = t["kf_mappoint"][(size_t)cur * cap + i];
            if (kind == OBS_RECENT) recent[counts[1]++] = t["kf_mappoint"][(size_t)cur * cap + i];
        }
    if (time) {
        std::printf("%.3f\n", ms_since(t0));
        return 0;
    }
    for (const char* name : {"mp_nobs", "mp_obs_kf", "mp_obs_idx"}) print(name, t[name]);
    print("added", added);
    print("recent_out", recent);
    print("counts", counts);
    print("status", status);
    return 0;
}

static int grow(Tables& t, bool time) {
    const std::vector<int32_t>&off = t["mp_obs_off"], &kf = t["mp_obs_kf"], &idx = t["mp_obs_idx"];
    if (off.empty() || kf.size() != idx.size() || t["slack"].empty() || t["n_obs_out"].empty()) return 2;
    const int M = (int)off.size() - 1, n_obs = (int)kf.size(), slack = t["slack"][0], n_out = t["n_obs_out"][0];
    const bool per_point = t.count("extra") && t["extra"].size() == (size_t)M;
    std::vector<int32_t> out_off(M + 1, 0), out_kf(n_out, 0), out_idx(n_out, 0);
    const auto t0 = std::chrono::steady_clock::now();
    long long at = 0;
    for (int p = 0; p < M; p++) {
        out_off[p] = (int32_t)(at < n_out + 1LL ? at : n_out + 1LL);
        const int s = per_point ? mm_clamp(t["extra"][p], 0, n_out) : slack;
        at += obs_grow_point(n_obs, off.data(), kf.data(), idx.data(), p, s, at, n_out, out_kf.data(), out_idx.data()) + s;
    }
    out_off[M] = (int32_t)(at < n_out + 1LL ? at : n_out + 1LL);
    const int32_t status = at > n_out ? MM_OBS_OVERFLOW : MM_OK;
    if (time) {
        std::printf("%.3f\n", ms_since(t0));
        return 0;
    }
    print("mp_obs_off", out_off);
    print("mp_obs_kf", out_kf);
    print("mp_obs_idx", out_idx);
    print("status", &status, 1);
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
    if (mode == "apply") return apply(t, time);
    if (mode == "new") return new_keyframe(t, time);
    if (mode == "grow") return grow(t, time);
    return 2;
}
