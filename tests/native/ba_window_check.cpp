// csrc/ba_window.h on the CPU (tests/test_local_ba_window_native.py): baw_gather_seq and baw_apply_seq, the rules the
// kernels of orbbamap.hip run per element, one after another.
//   ba_window_check gather|apply < tables
// The tables are lines "name count v0 v1 ..." of int32 values (floats as their bits, doubles as two words, keypoints as
// seven words, uint8 arrays widened), scalars as arrays of one.  "gather" reads the map, `cur` and `caps` (poses, points,
// edges) and prints counts and, when everything fits, the window's arrays.  "apply" reads the map, `cur`, `outlier`,
// `pose_R`, `pose_t` and `points`, gathers at full capacity, writes back, runs UpdateNormalAndDepth (mm_normal.h) over the
// window's points and prints every updated table.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "ba_window.h"

using namespace orbamd;
using Tables = std::map<std::string, std::vector<int32_t>>;

static std::vector<uint8_t> bytes(const std::vector<int32_t>& v) { return std::vector<uint8_t>(v.begin(), v.end()); }

template <class T>
static std::vector<T> recast(const std::vector<int32_t>& v) {
    std::vector<T> f(v.size() * 4 / sizeof(T));
    if (!f.empty()) std::memcpy(f.data(), v.data(), f.size() * sizeof(T));
    return f;
}

static void print(const char* name, const int32_t* v, size_t n) {
    std::printf("%s %zu", name, n);
    for (size_t i = 0; i < n; i++) std::printf(" %d", v[i]);
    std::printf("\n");
}
static void print_bytes(const char* name, const uint8_t* v, size_t n) {
    std::vector<int32_t> w(v, v + n);
    print(name, w.data(), n);
}
static void print_bits(const char* name, const float* f, size_t n) {
    std::vector<int32_t> b(n);
    if (n) std::memcpy(b.data(), f, 4 * n);
    print(name, b.data(), n);
}

struct Map {
    BaMap t{};
    std::vector<uint8_t> kf_bad, mp_bad;
    std::vector<float> uright, camera, pose, xw, normal, max_min, scale;
    std::vector<BaKeypoint> kp;
    explicit Map(Tables& m) {
        t.K = (int)m["kf_n"].size();
        t.M = (int)m["mp_bad"].size();
        t.kf_cap = t.K ? (int)(m["kf_mappoint"].size() / t.K) : 1;
        t.conn_cap = t.K ? (int)(m["ord_slot"].size() / t.K) : 1;
        t.n_obs = (int)m["mp_obs_kf"].size();
        t.n_levels = (int)m["inv_sigma2"].size();
        kf_bad = bytes(m["kf_bad"]); mp_bad = bytes(m["mp_bad"]);
        uright = recast<float>(m["kf_uright"]); camera = recast<float>(m["kf_camera"]); pose = recast<float>(m["kf_pose"]);
        xw = recast<float>(m["mp_xw"]); normal = recast<float>(m["mp_normal"]); max_min = recast<float>(m["mp_max_min"]);
        scale = recast<float>(m["scale_factors"]);
        kp = recast<BaKeypoint>(m["kf_keypoint"]);
        const std::vector<float> inv = recast<float>(m["inv_sigma2"]);
        for (int l = 0; l < t.n_levels && l < MM_MAX_LEVELS; l++) t.inv_sigma2[l] = inv[l];
        t.kf_id = m["kf_id"].data(); t.kf_n = m["kf_n"].data(); t.kf_bad = kf_bad.data(); t.kf_mappoint = m["kf_mappoint"].data();
        t.kf_keypoint = kp.data(); t.kf_uright = uright.data(); t.kf_camera = camera.data(); t.kf_pose = pose.data();
        t.ord_slot = m["ord_slot"].data(); t.n_ord = m["n_ord"].data(); t.mp_bad = mp_bad.data(); t.mp_xw = xw.data();
        t.mp_nobs = m["mp_nobs"].data(); t.mp_ref_kf = m["mp_ref_kf"].data(); t.mp_obs_off = m["mp_obs_off"].data();
        t.mp_obs_kf = m["mp_obs_kf"].data(); t.mp_obs_idx = m["mp_obs_idx"].data();
    }
};

struct Window {
    BaWindow w{};
    std::vector<int32_t> counts, pose_kf, point, ep, ek, ekf, eidx;
    std::vector<uint8_t> fixed;
    std::vector<float> obs, info, cam;
    Window(int P, int N, int E)
        : counts(BAW_COUNTS, -1), pose_kf(P), point(N), ep(E), ek(E), ekf(E), eidx(E), fixed(P), obs(3 * (size_t)E), info(E),
          cam(5 * (size_t)E) {
        w = BaWindow{P, N, E, counts.data(), pose_kf.data(), fixed.data(), point.data(), ep.data(), ek.data(), ekf.data(),
                     eidx.data(), obs.data(), info.data(), cam.data()};
    }
};

struct Scratch {
    std::vector<int32_t> mark, vertex, seen, list_kf, list_pt, list_fixed;
    BaSeqScratch s;
    explicit Scratch(const BaMap& t)
        : mark(t.K), vertex(t.K), seen(t.M), list_kf((size_t)t.conn_cap + 1), list_pt(t.M), list_fixed(t.K),
          s{mark.data(), vertex.data(), seen.data(), list_kf.data(), list_pt.data(), list_fixed.data()} {}
};

static int gather(Tables& m) {
    Map map(m);
    if (m["cur"].empty() || m["caps"].size() != 3) return 2;
    Window win(m["caps"][0], m["caps"][1], m["caps"][2]);
    Scratch sc(map.t);
    const int status = baw_gather_seq(map.t, m["cur"][0], win.w, sc.s);
    print("counts", win.counts.data(), BAW_COUNTS);
    if (status != BAW_OK) return 0;
    const int P = win.counts[BAW_N_LOCAL] + win.counts[BAW_N_FIXED], N = win.counts[BAW_N_POINTS], E = win.counts[BAW_N_EDGES];
    print("pose_kf", win.pose_kf.data(), P);
    print_bytes("pose_fixed", win.fixed.data(), P);
    print("point", win.point.data(), N);
    print("edge_point", win.ep.data(), E);
    print("edge_pose", win.ek.data(), E);
    print("edge_kf", win.ekf.data(), E);
    print("edge_idx", win.eidx.data(), E);
    print_bits("edge_obs", win.obs.data(), 3 * (size_t)E);
    print_bits("edge_inv_sigma2", win.info.data(), E);
    print_bits("edge_cam", win.cam.data(), 5 * (size_t)E);
    return 0;
}

static int apply(Tables& m) {
    Map map(m);
    if (m["cur"].empty()) return 2;
    const BaMap& t = map.t;
    Window win(t.K, t.M, t.n_obs);
    Scratch sc(t);
    if (baw_gather_seq(t, m["cur"][0], win.w, sc.s) != BAW_OK) return 2;
    const int P = win.counts[BAW_N_LOCAL] + win.counts[BAW_N_FIXED], N = win.counts[BAW_N_POINTS], E = win.counts[BAW_N_EDGES];
    const std::vector<uint8_t> outlier = bytes(m["outlier"]);
    const std::vector<double> R = recast<double>(m["pose_R"]), tr = recast<double>(m["pose_t"]), X = recast<double>(m["points"]);
    if ((int)outlier.size() < E || (int)R.size() < 9 * P || (int)tr.size() < 3 * P || (int)X.size() < 3 * N) return 2;
    baw_apply_seq(t, win.w, outlier.data(), R.data(), tr.data(), X.data());
    // UpdateNormalAndDepth over the local points (:734)
    std::vector<float> ow(3 * (size_t)t.K);
    for (int k = 0; k < t.K; k++) mm_center(t.kf_pose + 12 * (size_t)k, ow.data() + 3 * (size_t)k);
    MmPoints up{};
    up.K = t.K; up.M = t.M; up.kf_cap = t.kf_cap; up.n_obs = t.n_obs; up.n_levels = t.n_levels;
    up.mp_bad = t.mp_bad; up.mp_xw = t.mp_xw; up.mp_ref_kf = t.mp_ref_kf; up.mp_obs_off = t.mp_obs_off; up.mp_obs_kf = t.mp_obs_kf;
    up.mp_obs_idx = t.mp_obs_idx; up.kf_n = t.kf_n; up.kf_kp_octave = m["kf_kp_octave"].data(); up.kf_ow = ow.data();
    up.mp_normal = map.normal.data(); up.mp_max_min = map.max_min.data();
    for (int l = 0; l < t.n_levels && l < MM_MAX_LEVELS; l++) up.scale[l] = map.scale[l];
    for (int j = 0; j < N; j++) mm_update_point(up, win.point[j]);
    print("kf_mappoint", m["kf_mappoint"].data(), m["kf_mappoint"].size());
    print_bits("kf_pose", map.pose.data(), map.pose.size());
    print_bytes("mp_bad", map.mp_bad.data(), map.mp_bad.size());
    print_bits("mp_xw", map.xw.data(), map.xw.size());
    print("mp_nobs", m["mp_nobs"].data(), m["mp_nobs"].size());
    print("mp_ref_kf", m["mp_ref_kf"].data(), m["mp_ref_kf"].size());
    print("mp_obs_kf", m["mp_obs_kf"].data(), m["mp_obs_kf"].size());
    print_bits("mp_normal", map.normal.data(), map.normal.size());
    print_bits("mp_max_min", map.max_min.data(), map.max_min.size());
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
    const std::string mode = argv[1];
    if (mode == "gather") return gather(t);
    if (mode == "apply") return apply(t);
    return 2;
}
