// The projection searches' workspace layouts (csrc/orbp_layout.h) against the hand-written byte counts
// orbp.hip and its headers carried beside their carve sequences until the layouts replaced both
// (pj_workspace_bytes, pi_workspace_bytes, reloc_workspace_bytes / fuse_workspace_bytes, sim3_side_bytes).
// Those sums live here from now on, as the expected values.  Each workspace is also carved from a malloc
// of exactly its dry-run size and the first and last element of every field written, so AddressSanitizer
// sees any field that reaches past the end; the fields' offsets are multiples of 256, strictly increasing
// in the documented order and do not overlap, and the dry-run size is the end of the last field's padding.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbp_layout.h"

using namespace orbamd_host;

static int fails = 0;
static char g_shape[64] = "";
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fails++;                                                          \
            printf("FAILED %s (line %d, shape %s)\n", #c, __LINE__, g_shape); \
        }                                                                     \
    } while (0)

// ---- the library's old formulas
static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
static size_t old_pj_workspace_bytes(int n_frames, int total_kp, int total_mp) {
    return align_up((size_t)std::max(total_kp, 1) * 4, 256) + align_up((size_t)n_frames * (PJ_CELLS + 1) * 4, 256) +
           2 * align_up((size_t)std::max(total_mp, 1) * 4, 256) + align_up((size_t)std::max(total_mp, 1) * PJ_K * 8, 256);
}
static size_t old_pi_workspace_bytes(int n_pairs, int total_kp, int total_q) {
    return old_pj_workspace_bytes(n_pairs, total_kp, total_q) + align_up((size_t)std::max(total_q, 1) * 4, 256) +
           align_up((size_t)std::max(total_q, 1) * PI_CAP * 4, 256);
}
static size_t old_point_workspace_bytes(int n_frames, int total_kp, int total_mp) {   // reloc_ / fuse_workspace_bytes
    const size_t M = (size_t)std::max(total_mp, 1);
    return old_pj_workspace_bytes(n_frames, total_kp, total_mp) + align_up(M * 4, 256) + align_up(M, 256) +
           align_up(M * 12, 256) + align_up(M * 4, 256);
}
static size_t old_motion_workspace_bytes(int n_frames, int total_kp, int total_mp) {
    return old_pj_workspace_bytes(n_frames, total_kp, total_mp) + align_up((size_t)std::max(total_mp, 1) * 4, 256);
}
static size_t old_sim3_side_bytes(int n_pairs, int total) {
    const size_t T = (size_t)std::max(total, 1);
    return 4 * align_up(T * 4, 256) + align_up((size_t)n_pairs * (PJ_CELLS + 1) * 4, 256) + align_up(T, 256) +
           align_up(T * 8, 256);
}

// one field of a carved region: its address and element count / size, in the documented order
struct Field {
    char* p;
    size_t n, elem;
};
#define F(ptr, n) Field{reinterpret_cast<char*>(ptr), (size_t)(n), sizeof(*(ptr))}

// fields 256-aligned from the base, strictly increasing, none overlapping or past `bytes`; touch both ends
static void check_fields(char* base, size_t bytes, const std::vector<Field>& f) {
    size_t prev_end = 0;
    for (size_t i = 0; i < f.size(); i++) {
        const size_t off = (size_t)(f[i].p - base), n = std::max<size_t>(f[i].n, 1);
        CHECK(off % 256 == 0);
        CHECK(i == 0 ? off == 0 : off >= prev_end && off > (size_t)(f[i - 1].p - base));
        CHECK(off + n * f[i].elem <= bytes);
        f[i].p[0] = 1;
        f[i].p[n * f[i].elem - 1] = 1;
        prev_end = off + n * f[i].elem;
    }
    CHECK(bytes - prev_end < 256);   // the dry-run size is the end of the last field's padding
}

static std::vector<Field> grid_fields(const PjGridLayout& g, size_t Fr, size_t K, size_t M) {
    return {F(g.grid_idx, K), F(g.grid_start, Fr * (PJ_CELLS + 1)), F(g.mp_cnt, M), F(g.mp_frame, M), F(g.mp_top, M * PJ_K)};
}

template <class Carve, class Fields>
static void check_workspace(size_t want, Carve carve, Fields fields) {
    Carver dry{nullptr};
    carve(dry);
    CHECK(dry.off == want);
    char* m = (char*)malloc(dry.off);
    Carver c{m};
    carve(c);
    CHECK(c.off == dry.off);
    check_fields(m, dry.off, fields());
    free(m);
}

static void check(int Fr, int K, int M) {
    snprintf(g_shape, sizeof(g_shape), "(%d, %d, %d)", Fr, K, M);
    static_assert(sizeof(*PjGridLayout().mp_top) == 8, "mp_top holds uint2 entries");
    PjGridLayout g;
    PjPointLayout p;
    PiLayout q;
    // the grid / walk workspace alone (SearchByProjection)
    check_workspace(old_pj_workspace_bytes(Fr, K, M), [&](Carver& c) { g.carve(c, Fr, K, M); },
                    [&] { return grid_fields(g, Fr, K, M); });
    {
        Carver dry{nullptr};
        g.carve(dry, Fr, K, M);
        CHECK(g.grid_idx == nullptr && g.mp_top == nullptr);   // a dry run hands out no pointers
    }
    // + choice (the motion-model search)
    int32_t* choice;
    check_workspace(old_motion_workspace_bytes(Fr, K, M), [&](Carver& c) { g.carve(c, Fr, K, M); c.take(choice, M); },
                    [&] { auto f = grid_fields(g, Fr, K, M); f.push_back(F(choice, M)); return f; });
    // + the projected-point block (relocalisation, Fuse, the Sim3 projection search)
    check_workspace(old_point_workspace_bytes(Fr, K, M), [&](Carver& c) { g.carve(c, Fr, K, M); p.carve(c, M); },
                    [&] {
                        auto f = grid_fields(g, Fr, K, M);
                        for (const Field& x : {F(p.choice, M), F(p.out_valid, M), F(p.out_proj, 3 * (size_t)M), F(p.out_level, M)})
                            f.push_back(x);
                        return f;
                    });
    // + SearchForInitialization's candidate lists (M queries)
    check_workspace(old_pi_workspace_bytes(Fr, K, M), [&](Carver& c) { g.carve(c, Fr, K, M); q.carve(c, M); },
                    [&] {
                        auto f = grid_fields(g, Fr, K, M);
                        f.push_back(F(q.cnt, M));
                        f.push_back(F(q.cand, std::max<size_t>(M, 1) * PI_CAP));
                        return f;
                    });
    // SearchBySim3: one block per side (K and M keypoint slots)
    Sim3SideLayout s[2];
    const int tot[2] = {K, M};
    check_workspace(old_sim3_side_bytes(Fr, K) + old_sim3_side_bytes(Fr, M),
                    [&](Carver& c) { for (int d = 0; d < 2; d++) s[d].carve(c, Fr, tot[d]); },
                    [&] {
                        std::vector<Field> f;
                        for (int d = 0; d < 2; d++)
                            for (const Field& x : {F(s[d].grid_idx, tot[d]), F(s[d].grid_start, (size_t)Fr * (PJ_CELLS + 1)),
                                                   F(s[d].pair, tot[d]), F(s[d].out_level, tot[d]), F(s[d].match, tot[d]),
                                                   F(s[d].out_valid, tot[d]), F(s[d].out_uv, 2 * (size_t)tot[d])})
                                f.push_back(x);
                        return f;
                    });
}

int main() {
    // (frames, keypoints, points): empty arrays, one of each, a ragged batch, no points
    const int shapes[][3] = {{1, 0, 0}, {1, 1, 1}, {3, 8192, 700}, {2, 100, 0}};
    for (const auto& s : shapes) check(s[0], s[1], s[2]);
    printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
