// csrc/lc_propagate.h on the CPU (tests/test_loop_correct_native.py): the passes of orblc.hip's propagation as loops.
//   loop_correct_check < tables
// The tables are lines "name count v0 v1 ..." of int32 values (floats as their bits; uint8 arrays widened), scalars as
// arrays of one: the map, `scale`, `cur`, `scw` (13) and `connected`.  Prints every updated table, vertex_sim3, edge_sim3
// and point_ref.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "lc_propagate.h"

using namespace orbamd;
using Tables = std::map<std::string, std::vector<int32_t>>;

static std::vector<float> floats(const std::vector<int32_t>& v) {
    static_assert(sizeof(float) == sizeof(int32_t), "");
    std::vector<float> f(v.size());
    if (!v.empty()) std::memcpy(f.data(), v.data(), 4 * v.size());
    return f;
}

static void print(const char* name, const int32_t* v, size_t n) {
    std::printf("%s %zu", name, n);
    for (size_t i = 0; i < n; i++) std::printf(" %d", v[i]);
    std::printf("\n");
}

static void print_bits(const char* name, const std::vector<float>& f) {
    std::vector<int32_t> b(f.size());
    if (!f.empty()) std::memcpy(b.data(), f.data(), 4 * f.size());
    print(name, b.data(), b.size());
}

int main() {
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
    if (t["cur"].empty() || t["scw"].size() != 13 || t["scale"].empty() || t["scale"].size() > (size_t)MM_MAX_LEVELS) return 2;
    const int K = (int)t["kf_n"].size(), M = (int)t["mp_bad"].size(), cur = t["cur"][0];
    if (K == 0 || cur < 0 || cur >= K) return 2;
    std::vector<uint8_t> mp_bad(t["mp_bad"].begin(), t["mp_bad"].end()), is_conn(K, 0);
    std::vector<float> xw = floats(t["mp_xw"]), pose = floats(t["kf_pose"]), normal = floats(t["mp_normal"]),
                       max_min = floats(t["mp_max_min"]), scale = floats(t["scale"]), scw = floats(t["scw"]);
    std::vector<float> ow_entry(3 * (size_t)K), ow_corr(3 * (size_t)K), new_pose(12 * (size_t)K), vertex(13 * (size_t)K),
        edge(13 * (size_t)K);
    std::vector<int32_t> claim(M, LC_UNCLAIMED), point_ref(M, 0);
    const std::vector<int32_t>& connected = t["connected"];
    LcMap m{};
    m.pts.K = K; m.pts.M = M; m.pts.kf_cap = (int)(t["kf_mappoint"].size() / K); m.pts.n_obs = (int)t["mp_obs_kf"].size();
    m.pts.n_levels = (int)scale.size();
    m.pts.mp_bad = mp_bad.data(); m.pts.mp_xw = xw.data(); m.pts.mp_ref_kf = t["mp_ref_kf"].data();
    m.pts.mp_obs_off = t["mp_obs_off"].data(); m.pts.mp_obs_kf = t["mp_obs_kf"].data(); m.pts.mp_obs_idx = t["mp_obs_idx"].data();
    m.pts.kf_n = t["kf_n"].data(); m.pts.kf_kp_octave = t["kf_kp_octave"].data(); m.pts.kf_ow = ow_entry.data();
    m.pts.mp_normal = normal.data(); m.pts.mp_max_min = max_min.data();
    for (size_t l = 0; l < scale.size(); l++) m.pts.scale[l] = scale[l];
    m.conn_cap = 1; m.kf_id = t["kf_id"].data(); m.kf_mappoint = t["kf_mappoint"].data(); m.mp_xw = xw.data();
    m.kf_pose = pose.data(); m.mp_corrected_by = t["mp_corrected_by"].data(); m.mp_corrected_ref = t["mp_corrected_ref"].data();
    const LcWork w{ow_entry.data(), ow_corr.data(), new_pose.data(), is_conn.data(), claim.data()};
    const int C = (int)connected.size(), cur_id = m.kf_id[cur];
    for (int k = 0; k < K; k++) lc_keyframe(m, w, k, cur, scw.data(), connected.data(), C, vertex.data(), edge.data());
    for (int j = 0; j < C; j++) {
        const int k = connected[j];
        if (k < 0 || k >= K) continue;
        for (int i = 0; i < m.pts.kf_cap; i++) {
            const int p = lc_claimed_point(m, k, i, cur_id);
            if (p >= 0 && k < claim[p]) claim[p] = k;
        }
    }
    for (int p = 0; p < M; p++) lc_point(m, w, p, cur_id, vertex.data(), edge.data(), point_ref.data());
    for (int k = 0; k < K; k++)
        if (is_conn[k]) std::memcpy(&pose[12 * (size_t)k], &new_pose[12 * (size_t)k], 12 * sizeof(float));
    print_bits("mp_xw", xw);
    print_bits("kf_pose", pose);
    print_bits("mp_normal", normal);
    print_bits("mp_max_min", max_min);
    print("mp_corrected_by", t["mp_corrected_by"].data(), t["mp_corrected_by"].size());
    print("mp_corrected_ref", t["mp_corrected_ref"].data(), t["mp_corrected_ref"].size());
    print_bits("vertex_sim3", vertex);
    print_bits("edge_sim3", edge);
    print("point_ref", point_ref.data(), point_ref.size());
    return 0;
}
