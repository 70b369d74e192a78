// csrc/mk_create.h on the CPU (tests/test_creation_native.py): the rules the kernels of orbmk.hip run, one after another.
//   creation_check create|insert < tables
// The tables are lines "name count v0 v1 ..." of int32 values (floats as their bits; uint8 arrays widened), scalars as
// arrays of one.  "create" reads the map, the list batch (`list_cap`, `by_keypoint`; kf2, idx2, normal, max_distance,
// min_distance, item_frame / frame_mappoint / kp_cap, recent / n_recent optional) and `alloc`, and prints every updated
// table and output.  "insert" reads a frame batch (`kp_cap`), the keyframe tables (`kf_cap`, `conn_cap`) and the item
// arrays and prints the keyframe tables.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "mk_create.h"

using namespace orbamd;
using Tables = std::map<std::string, std::vector<int32_t>>;

static void print(const char* name, const int32_t* v, size_t n) {
    std::printf("%s %zu", name, n);
    for (size_t i = 0; i < n; i++) std::printf(" %d", v[i]);
    std::printf("\n");
}

static void print(const char* name, const std::vector<int32_t>& v) { print(name, v.data(), v.size()); }

// A uint8 table (narrowed on the way in, widened on the way out); aligned for MkDesc.
struct Bytes {
    std::vector<MkDesc> store;
    size_t n = 0;
    bool given = false;
    Bytes(Tables& t, const char* name) {
        given = t.count(name) > 0;
        const std::vector<int32_t>& v = t[name];
        n = v.size();
        store.resize(n / 32 + 1);
        for (size_t i = 0; i < n; i++) data()[i] = (uint8_t)v[i];
    }
    uint8_t* data() { return reinterpret_cast<uint8_t*>(store.data()); }
    uint8_t* ptr() { return given ? data() : nullptr; }
    MkDesc* desc() { return given ? store.data() : nullptr; }
    void print_as(const char* name) {
        if (!given) return;
        std::vector<int32_t> w(data(), data() + n);
        print(name, w);
    }
};

static float* floats(Tables& t, const char* name) { return t.count(name) ? reinterpret_cast<float*>(t[name].data()) : nullptr; }
static int32_t* ints(Tables& t, const char* name) { return t.count(name) ? t[name].data() : nullptr; }

static int create(Tables& t) {
    for (const char* name : {"kf_n", "kf_id", "mp_bad", "mp_obs_off", "list_cap", "by_keypoint", "alloc", "kf1", "n_list"})
        if (t[name].empty()) return 2;
    Bytes kf_bad(t, "kf_bad"), kf_desc(t, "kf_desc"), mp_bad(t, "mp_bad"), mp_desc(t, "mp_desc");
    MkMap m{};
    m.K = (int)t["kf_n"].size();
    m.M = (int)t["mp_bad"].size();
    m.kf_cap = (int)(t["kf_mappoint"].size() / m.K);
    m.n_obs = (int)t["mp_obs_kf"].size();
    m.kf_id = ints(t, "kf_id"); m.kf_n = ints(t, "kf_n"); m.kf_mappoint = ints(t, "kf_mappoint"); m.kf_uright = floats(t, "kf_uright");
    m.kf_bad = kf_bad.ptr(); m.kf_desc = kf_desc.desc(); m.mp_bad = mp_bad.ptr(); m.mp_xw = floats(t, "mp_xw");
    m.mp_normal = floats(t, "mp_normal"); m.mp_max_min = floats(t, "mp_max_min"); m.mp_nobs = ints(t, "mp_nobs");
    m.mp_found = ints(t, "mp_found"); m.mp_visible = ints(t, "mp_visible"); m.mp_replaced = ints(t, "mp_replaced");
    m.mp_first_kf_id = ints(t, "mp_first_kf_id"); m.mp_ref_kf = ints(t, "mp_ref_kf"); m.mp_desc = mp_desc.desc();
    m.mp_obs_off = ints(t, "mp_obs_off"); m.mp_obs_kf = ints(t, "mp_obs_kf"); m.mp_obs_idx = ints(t, "mp_obs_idx");
    MkLists l{};
    l.n_items = (int)t["kf1"].size();
    l.list_cap = t["list_cap"][0];
    l.by_keypoint = t["by_keypoint"][0];
    l.kf1 = ints(t, "kf1"); l.kf2 = ints(t, "kf2"); l.n_list = ints(t, "n_list"); l.idx1 = ints(t, "idx1"); l.idx2 = ints(t, "idx2");
    l.xw = floats(t, "xw"); l.normal = floats(t, "normal"); l.max_distance = floats(t, "max_distance");
    l.min_distance = floats(t, "min_distance");
    l.item_frame = ints(t, "item_frame");
    l.frame_mappoint = ints(t, "frame_mappoint");
    l.kp_cap = t.count("kp_cap") ? t["kp_cap"][0] : 1;
    l.F = l.frame_mappoint ? (int)(t["frame_mappoint"].size() / l.kp_cap) : 0;
    if (t["idx1"].size() != (size_t)l.n_items * l.list_cap || t["xw"].size() != 3 * t["idx1"].size()) return 2;
    std::vector<int32_t> status(1, -1), needed(2, -9), created((size_t)l.n_items * l.list_cap, -9), n_created(l.n_items, -9);
    MkOut o{};
    o.alloc = ints(t, "alloc"); o.status = status.data(); o.needed = needed.data(); o.created = created.data();
    o.n_created = n_created.data(); o.recent = ints(t, "recent"); o.n_recent = ints(t, "n_recent");
    o.recent_cap = (int)t["recent"].size();
    if (o.recent && !o.n_recent) return 2;

    // count per chunk, scan, the rows, the decision, fill: what orbmk.hip's three kernels do
    const int nc = mk_chunks(l.list_cap);
    std::vector<long long> off((size_t)l.n_items * nc + 1, 0);
    for (int i = 0; i < l.n_items; i++)
        for (int c = 0; c < nc; c++) {
            int n = 0;
            for (int j = c * MK_CHUNK; j < (c + 1) * MK_CHUNK && j < mk_list_n(l, i); j++) n += mk_entry_valid(m, l, i, j) ? 1 : 0;
            off[(size_t)i * nc + c + 1] = off[(size_t)i * nc + c] + n;
        }
    const long long total = off.back();
    const int base = mk_base(m, o), recent_base = mk_recent_base(o);
    int short_slot = -1;
    if (base + total <= m.M)
        for (int i = 0; i < l.n_items && short_slot < 0; i++)
            for (long long r = off[(size_t)i * nc]; r < off[((size_t)i + 1) * nc] && short_slot < 0; r++)
                if (!mk_row_fits(m, (int)(base + r), mk_need(l, i))) short_slot = (int)(base + r);
    const bool ok = mk_decide(m, o, base, recent_base, total, short_slot) == MK_OK;
    for (int i = 0; i < l.n_items; i++) {
        long long r = off[(size_t)i * nc];
        for (int j = 0; j < l.list_cap; j++) {
            if (ok && j < mk_list_n(l, i) && mk_entry_valid(m, l, i, j)) {
                mk_create_point(m, l, o, i, j, (int)(base + r), (int)(recent_base + r));
                r++;
            } else {
                created[(size_t)i * l.list_cap + j] = -1;
            }
        }
        n_created[i] = ok ? (int32_t)(off[((size_t)i + 1) * nc] - off[(size_t)i * nc]) : 0;
    }
    for (const char* name : {"kf_mappoint", "mp_xw", "mp_normal", "mp_max_min", "mp_nobs", "mp_found", "mp_visible", "mp_replaced",
                             "mp_first_kf_id", "mp_ref_kf", "mp_obs_kf", "mp_obs_idx", "frame_mappoint", "alloc", "recent", "n_recent"})
        if (t.count(name)) print(name, t[name]);
    mp_bad.print_as("mp_bad");
    mp_desc.print_as("mp_desc");
    print("status", status);
    print("needed", needed);
    print("created", created);
    print("n_created", n_created);
    return 0;
}

static int insert(Tables& t) {
    for (const char* name : {"frame_n", "kp_cap", "kf_cap", "conn_cap", "n_keyframes", "item_frame", "item_kf"})
        if (t[name].empty()) return 2;
    Bytes kp_desc(t, "kp_desc"), kf_desc(t, "kf_desc"), kf_bad(t, "kf_bad"), kf_not_erase(t, "kf_not_erase"),
        kf_to_be_erased(t, "kf_to_be_erased"), kf_first_connection(t, "kf_first_connection");
    MkFrames f{};
    f.F = (int)t["frame_n"].size();
    f.kp_cap = t["kp_cap"][0];
    f.frame_n = ints(t, "frame_n"); f.frame_mappoint = ints(t, "frame_mappoint");
    f.kp_un = reinterpret_cast<const MkKeypoint*>(ints(t, "kp_un")); f.kp_octave = ints(t, "kp_octave");
    f.kp_uright = floats(t, "kp_uright"); f.kp_depth = floats(t, "kp_depth"); f.kp_desc = kp_desc.desc(); f.pose = floats(t, "pose");
    f.camera = floats(t, "camera");
    MkKeyframes k{};
    k.K = t["n_keyframes"][0];
    k.kf_cap = t["kf_cap"][0];
    k.conn_cap = t["conn_cap"][0];
    k.kf_id = ints(t, "kf_id"); k.kf_n = ints(t, "kf_n"); k.kf_mappoint = ints(t, "kf_mappoint");
    k.kf_keypoint = reinterpret_cast<MkKeypoint*>(ints(t, "kf_keypoint")); k.kf_kp_octave = ints(t, "kf_kp_octave");
    k.kf_uright = floats(t, "kf_uright"); k.kf_depth = floats(t, "kf_depth"); k.kf_desc = kf_desc.desc(); k.kf_pose = floats(t, "kf_pose");
    k.kf_camera = floats(t, "kf_camera"); k.kf_bad = kf_bad.ptr(); k.kf_not_erase = kf_not_erase.ptr();
    k.kf_to_be_erased = kf_to_be_erased.ptr(); k.kf_parent = ints(t, "kf_parent"); k.kf_first_connection = kf_first_connection.ptr();
    k.conn_slot = ints(t, "conn_slot"); k.conn_weight = ints(t, "conn_weight"); k.n_conn = ints(t, "n_conn");
    k.ord_slot = ints(t, "ord_slot"); k.ord_weight = ints(t, "ord_weight"); k.n_ord = ints(t, "n_ord"); k.kf_covis = ints(t, "kf_covis");
    const MkItems a{(int)t["item_frame"].size(), ints(t, "item_frame"), ints(t, "item_kf"), ints(t, "item_id"), floats(t, "item_baseline")};
    if (f.kp_cap > k.kf_cap || t["item_kf"].size() != t["item_frame"].size()) return 2;
    for (int it = 0; it < a.n_items; it++) {
        int fi, ki;
        if (!mk_item(f, k, a, it, fi, ki)) continue;
        for (int i = 0; i < k.kf_cap; i++) mk_insert_keypoint(f, k, fi, ki, i);
        for (int q = 0; q < MK_HEAD_ENTRIES + k.conn_cap; q++) mk_insert_head(f, k, a, it, fi, ki, q);
    }
    for (const char* name : {"kf_id", "kf_n", "kf_mappoint", "kf_keypoint", "kf_kp_octave", "kf_uright", "kf_depth", "kf_pose", "kf_camera",
                             "kf_parent", "conn_slot", "conn_weight", "n_conn", "ord_slot", "ord_weight", "n_ord", "kf_covis"})
        if (t.count(name)) print(name, t[name]);
    kf_desc.print_as("kf_desc");
    kf_bad.print_as("kf_bad");
    kf_not_erase.print_as("kf_not_erase");
    kf_to_be_erased.print_as("kf_to_be_erased");
    kf_first_connection.print_as("kf_first_connection");
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
    if (mode == "create") return create(t);
    if (mode == "insert") return insert(t);
    return 2;
}
