// LocalBA's buffer layouts (csrc/ba_layout.h) against the hand-written byte counts the library carried
// until the layouts replaced them: `carve_size` sums kept beside the carve sequences in orbba.hip.  Those
// sums live here from now on, as the expected values.  Each region is also carved from a malloc of
// exactly its dry-run size and the first and last element of every field written, so AddressSanitizer
// sees any field that reaches past the end; the fields' offsets are multiples of 256 and strictly
// increasing in the documented order.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ba_layout.h"

using namespace orbamd_host;

static int fails = 0;
#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fails++;                                                          \
            printf("FAILED %s (line %d, shape %s)\n", #c, __LINE__, g_shape); \
        }                                                                     \
    } while (0)
static const char* g_shape = "";

// ---- the library's old formulas
static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
template <class T>
static size_t carve_size(size_t n) { return align_up(std::max<size_t>(n, 1) * sizeof(T), 256); }
struct old_int2 { int x, y; };
struct alignas(16) old_int4 { int x, y, z, w; };

constexpr int SB = 16, SB_SPLIT = 2;
static int solve_dp(int D) { return (D + SB - 1) / SB * SB; }
static size_t solve_lds_doubles(int D) { return (size_t)solve_dp(D) * (solve_dp(D) + 1) + 3 * (size_t)solve_dp(D); }

struct Shape {
    const char* name;
    int P, N, E;
    bool one_cam;
    int Ea, np, nl, nblk;
    size_t nps, npairs;
};

// one field of a carved region: its address and element count / size, in the documented order
struct Field {
    char* p;
    size_t n, elem;
};
#define F(ptr, n) Field{reinterpret_cast<char*>(ptr), (size_t)(n), sizeof(*(ptr))}

// fields 256-aligned from the base, strictly increasing, none past `bytes`; touch both ends of each
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
    CHECK(bytes - prev_end < 256);   // the region ends with its last field's padding
}

static void check(const Shape& s) {
    g_shape = s.name;
    const size_t P = s.P, N = s.N, E = s.E;
    // ---- upload / state / result
    const size_t ncam = s.one_cam ? 5 : 5 * E;
    const size_t up_bytes = carve_size<uint8_t>(P) + carve_size<int>(E) * 2 + carve_size<uint8_t>(E) +
                            carve_size<double>(3 * E) + carve_size<double>(E) + carve_size<double>(ncam) +
                            carve_size<double>(4 * P) + carve_size<double>(3 * P) + carve_size<double>(3 * N);
    const size_t state_bytes = carve_size<double>(4 * P) + carve_size<double>(3 * P) + carve_size<double>(3 * N) +
                               carve_size<uint8_t>(E) * 2 + carve_size<double>(3 * E);
    const size_t res_bytes = carve_size<double>(4 * P) + carve_size<double>(3 * P) + carve_size<double>(3 * N) +
                             carve_size<uint8_t>(E) + carve_size<double>(E);
    {
        UploadLayout u;
        CHECK(u.carve(nullptr, P, N, E, s.one_cam) == up_bytes);
        CHECK(u.fixed == nullptr && u.X == nullptr);   // a dry run hands out no pointers
        char* m = (char*)malloc(up_bytes);
        CHECK(u.carve(m, P, N, E, s.one_cam) == up_bytes);
        check_fields(m, up_bytes, {F(u.fixed, P), F(u.ep, E), F(u.ek, E), F(u.stereo, E), F(u.obs, 3 * E), F(u.info, E),
                                   F(u.cam, ncam), F(u.q, 4 * P), F(u.t, 3 * P), F(u.X, 3 * N)});
        free(m);
    }
    {
        StateLayout t;
        CHECK(t.carve(nullptr, P, N, E) == state_bytes);
        char* m = (char*)malloc(state_bytes);
        t.carve(m, P, N, E);
        check_fields(m, state_bytes, {F(t.q_sv, 4 * P), F(t.t_sv, 3 * P), F(t.X_sv, 3 * N), F(t.robust, E), F(t.level, E),
                                      F(t.err, 3 * E)});
        free(m);
    }
    {
        ResultLayout r;
        CHECK(r.carve(nullptr, P, N, E) == res_bytes);
        char* m = (char*)malloc(res_bytes);
        r.carve(m, P, N, E);
        check_fields(m, res_bytes, {F(r.q, 4 * P), F(r.t, 3 * P), F(r.X, 3 * N), F(r.outlier, E), F(r.chi2, E)});
        free(m);
    }
    // ---- structure, host build and device build
    const int Ea = s.Ea, np = s.np, nl = s.nl, nblk = s.nblk;
    const size_t nps = s.nps, npairs = s.npairs;
    for (int dev_build = 0; dev_build < 2; dev_build++) {
        const size_t sbytes = carve_size<int>(P) + carve_size<int>(N) + carve_size<int>(nl + 1) + carve_size<int>(nl) +
                              carve_size<int>(np + 1) + carve_size<int>(np) + carve_size<int>(nblk) * 2 +
                              carve_size<int>(nblk + 1) + carve_size<int>(np) + carve_size<int>(Ea) * 2 +
                              carve_size<int>(nps) + carve_size<old_int2>(npairs) + carve_size<old_int4>(Ea) +
                              (dev_build ? carve_size<int>((size_t)np * nl) : 0);
        // (the extents the library took from its carve cursor: after blk_diag, after blk_pair)
        const size_t small_bytes = carve_size<int>(P) + carve_size<int>(N) + carve_size<int>(nl + 1) + carve_size<int>(nl) +
                                   carve_size<int>(np + 1) + carve_size<int>(np) + carve_size<int>(nblk) * 2 +
                                   carve_size<int>(nblk + 1) + carve_size<int>(np);
        const size_t list_bytes = small_bytes + carve_size<int>(Ea) * 2 + carve_size<int>(nps) + carve_size<old_int2>(npairs);
        const StructDims d{P, N, (size_t)Ea, (size_t)np, (size_t)nl, (size_t)nblk, nps, npairs, dev_build != 0};
        StructLayout t;
        CHECK(t.carve(nullptr, d) == sbytes);
        CHECK(t.small_bytes == small_bytes && t.list_bytes == list_bytes);
        char* m = (char*)malloc(sbytes);
        CHECK(t.carve(m, d) == sbytes);
        std::vector<Field> f = {F(t.hp, P), F(t.hl, N), F(t.pt_beg, nl + 1), F(t.pt_id, nl), F(t.ps_beg, np + 1),
                                F(t.ps_id, np), F(t.blk_i1, nblk), F(t.blk_i2, nblk), F(t.blk_beg, nblk + 1),
                                F(t.blk_diag, np), F(t.act, Ea), F(t.pt_slot, Ea), F(t.ps_slot, nps),
                                F(t.blk_pair, npairs), F(t.pt_rec, Ea)};
        CHECK((size_t)((char*)t.act - m) == small_bytes && (size_t)((char*)t.pt_rec - m) == list_bytes);
        CHECK((t.slot != nullptr) == (dev_build != 0));
        if (dev_build) f.push_back(F(t.slot, (size_t)np * nl));
        check_fields(m, sbytes, f);
        free(m);
    }
    static_assert(sizeof(Int2) == sizeof(old_int2) && sizeof(Int4) == sizeof(old_int4), "int2 / int4 sizes");
    // ---- system, LDS solve or global solve as the library decides
    {
        const int D = 6 * np, Dp = solve_dp(D);
        const bool glob = D > 128 || solve_lds_doubles(D) * 8 + 4096 > 160 * 1024;
        const size_t spart_n = (size_t)(SB_SPLIT + 1) * (glob ? 36 * (size_t)nblk : (size_t)D * D);
        const size_t ybytes = carve_size<double>(72 * (size_t)Ea) + carve_size<double>(24 * (size_t)Ea) +
                              carve_size<double>(9 * (size_t)nl) * 2 + carve_size<double>(3 * (size_t)nl) +
                              carve_size<double>(36 * (size_t)np) + carve_size<double>(6 * (size_t)np) +
                              carve_size<double>((size_t)D * D) + carve_size<double>(spart_n) +
                              carve_size<unsigned>((size_t)nblk) + carve_size<double>(D) +
                              carve_size<double>(D + 3 * (size_t)nl) + carve_size<double>(std::max(Ea, nl)) +
                              carve_size<double>(nl + np) + (glob ? carve_size<double>((size_t)Dp * (Dp + 1)) : 0) +
                              carve_size<double>(2 * (size_t)((nl * 8 + 63) / 64)) +
                              64;
        const SystemDims d{(size_t)Ea, (size_t)np, (size_t)nl, (size_t)nblk, spart_n, glob ? (size_t)Dp * (Dp + 1) : 0};
        SystemLayout y;
        // (the old sum ended in 64 spare bytes that no carve ever took; the layout has none)
        const size_t bytes = y.carve(nullptr, d);
        CHECK(bytes == ybytes - 64);
        char* m = (char*)malloc(bytes);
        CHECK(y.carve(m, d) == bytes);
        CHECK((y.Sg != nullptr) == glob);
        std::vector<Field> f = {F(y.J, 72 * (size_t)Ea), F(y.W, 24 * (size_t)Ea), F(y.Hll, 9 * (size_t)nl),
                                F(y.Dinv, 9 * (size_t)nl), F(y.bl, 3 * (size_t)nl), F(y.Hpp, 36 * (size_t)np),
                                F(y.bp, 6 * (size_t)np), F(y.S, (size_t)D * D), F(y.Spart, spart_n), F(y.blk_done, nblk),
                                F(y.bs, D), F(y.x, D + 3 * (size_t)nl), F(y.rchi, std::max(Ea, nl)), F(y.part, nl + np)};
        if (glob) f.push_back(F(y.Sg, (size_t)Dp * (Dp + 1)));
        f.push_back(F(y.wgpart, 2 * (size_t)((nl * 8 + 63) / 64)));
        check_fields(m, bytes, f);
        free(m);
    }
}

int main() {
    // the smallest shapes that reach each branch: empty, one of each, a few poses, C4's window (np = 18: LDS
    // solve), np = 22 (D = 132 > 128: the global solve's Sg), and no pose-pair block
    const Shape shapes[] = {
        {"empty", 0, 0, 0, false, 0, 0, 0, 0, 0, 0},
        {"ones", 1, 1, 1, true, 1, 1, 1, 1, 1, 1},
        {"small", 5, 200, 903, true, 903, 3, 200, 6, 611, 1420},
        {"small, a camera per edge", 5, 200, 903, false, 903, 3, 200, 6, 611, 1420},
        {"C4", 20, 3000, 14711, true, 14711, 18, 3000, 171, 13290, 61007},
        {"np 22", 24, 3000, 16001, false, 16001, 22, 2999, 253, 14873, 70011},
        {"no blocks", 3, 40, 77, true, 77, 0, 40, 0, 0, 0},
    };
    for (const Shape& s : shapes) check(s);
    printf("%d failures\n", fails);
    return fails ? 1 : 0;
}
