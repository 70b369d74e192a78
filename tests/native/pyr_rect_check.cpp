// The pyramid kernels' rectangle model (csrc/orbx_pyr_rect.h) on the CPU, by brute force over every tile of
// every level pair of an 8-level, scale-1.2 pyramid: the rectangles pyr_pair_rect reads from the first and
// last table entries must hold every tap, pyr_pair_plan must accept the kernel's 64 x 64 tile with its
// capacities, and the level-l rectangles the workgroups write must cover level l.  Other tile shapes are
// checked for the same geometric properties under roomy capacities and their issued-slot ratio printed
// (the model of DESIGN §4 "Pyramid").  Also the reciprocal table's divisions.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "orbx_pyr_rect.h"

using namespace orbamd;

struct I2 { int x, y; };
static int fails = 0;
#define CHECK(c, ...)                                   \
    do {                                                \
        if (!(c)) {                                     \
            if (++fails <= 20) { std::printf("FAIL %s: ", #c); std::printf(__VA_ARGS__); std::printf("\n"); } \
        }                                               \
    } while (0)

static int lo(const I2& v) { return v.x & 0xffff; }
static int hi(const I2& v) { return (int)((unsigned)v.x >> 16); }

struct Pyr {
    std::vector<int> w, h, xo, yo;
    std::vector<I2> xt, yt;
};
static Pyr build(int W, int H, int levels = 8, float sf = 1.2f) {
    Pyr P;
    float s = 1.f;
    for (int l = 0; l < levels; l++, s *= sf) {
        const float inv = 1.f / s;
        P.w.push_back(l ? (int)std::lrintf(inv * W) : W);
        P.h.push_back(l ? (int)std::lrintf(inv * H) : H);
        P.xo.push_back((int)P.xt.size());
        P.yo.push_back((int)P.yt.size());
        if (l) pyr_resize_tables(P.w[l - 1], P.h[l - 1], P.w[l], P.h[l], P.xt, P.yt);
    }
    return P;
}

// one pair (l, l+1) under capacities K; kernel: K is the kernel's own form, whose plan must be ok
static void check_pair(const Pyr& P, int W, int H, int l, const PyrCaps& K, bool kernel) {
    const I2 *xt1 = P.xt.data() + P.xo[l], *yt1 = P.yt.data() + P.yo[l];
    const I2 *xt2 = P.xt.data() + P.xo[l + 1], *yt2 = P.yt.data() + P.yo[l + 1];
    const int w0 = P.w[l - 1], h0 = P.h[l - 1], w1 = P.w[l], h1 = P.h[l], w2 = P.w[l + 1], h2 = P.h[l + 1];
    const PyrPairPlan plan = pyr_pair_plan(w0, h0, w1, h1, w2, h2, xt1, yt1, xt2, yt2, K);
    CHECK(plan.ok, "%dx%d pair %d tile %dx%d", W, H, l, K.tw, K.th);
    if (kernel) CHECK(plan.passes <= PP_MAXP && plan.max_ncol <= PP_MAXC && plan.max_nrow <= PP_MAXR, "%dx%d pair %d", W, H, l);
    std::vector<char> wrote((size_t)w1 * h1, 0);
    long long slots = 0;
    int passes = 0;
    for (int ty0 = 0; ty0 < h2; ty0 += K.th)
        for (int tx0 = 0; tx0 < w2; tx0 += K.tw) {
            const int tw = std::min(K.tw, w2 - tx0), th = std::min(K.th, h2 - ty0);
            const PyrPairRect R = pyr_pair_rect(xt1, yt1, xt2, yt2, tx0, ty0, tw, th);
            CHECK(R.c0 >= 0 && R.c0 % 4 == 0 && R.c1 < w1 && R.c0 <= R.c1 && R.ay0 >= 0 && R.ay1 < h1 && R.ay0 <= R.ay1,
                  "%dx%d pair %d tile (%d,%d): level-l rectangle", W, H, l, tx0, ty0);
            CHECK(R.xa >= 0 && R.xa % 16 == 0 && R.bx1 < w0 && R.xa <= R.bx1 && R.by0 >= 0 && R.by1 < h0 && R.by0 <= R.by1,
                  "%dx%d pair %d tile (%d,%d): staged rectangle", W, H, l, tx0, ty0);
            if (fails) return;
            // every tap of every tile pixel inside the level-l rectangle
            for (int x = tx0; x < tx0 + tw; x++)
                CHECK(lo(xt2[x]) >= R.c0 && hi(xt2[x]) <= R.c1, "%dx%d pair %d column %d", W, H, l, x);
            for (int y = ty0; y < ty0 + th; y++)
                CHECK(lo(yt2[y]) >= R.ay0 && hi(yt2[y]) <= R.ay1, "%dx%d pair %d row %d", W, H, l, y);
            // every tap of every rectangle pixel inside the staged level-(l-1) rectangle
            for (int x = R.c0; x <= R.c1; x++)
                CHECK(lo(xt1[x]) >= R.xa && hi(xt1[x]) <= R.bx1, "%dx%d pair %d level-l column %d", W, H, l, x);
            for (int y = R.ay0; y <= R.ay1; y++)
                CHECK(lo(yt1[y]) >= R.by0 && hi(yt1[y]) <= R.by1, "%dx%d pair %d level-l row %d", W, H, l, y);
            // the capacities, spelled out from the kernel's use of them
            const int ncol = R.c1 - R.c0 + 1, nrow = R.ay1 - R.ay0 + 1, ncq = (ncol + 3) / 4, rpp = 256 / ncq;
            const int np = (nrow + rpp - 1) / rpp, nc = (R.bx1 - R.xa) / 16 + 1, bh = R.by1 - R.by0 + 1;
            CHECK(ncol <= K.maxc && nrow <= K.maxr && np <= K.maxp, "%dx%d pair %d tile (%d,%d): %d x %d, %d passes", W, H,
                  l, tx0, ty0, ncol, nrow, np);
            CHECK(4 * ncq + 8 <= K.sw && nrow <= K.sh && 16 * nc <= K.sw && bh <= K.sh && nc * bh <= K.pieces,
                  "%dx%d pair %d tile (%d,%d): LDS %d x %d from %d x %d", W, H, l, tx0, ty0, ncol, nrow, 16 * nc, bh);
            if (kernel) {
                CHECK(ncq < PYR_RECIP_N && nc < PYR_RECIP_N, "%dx%d pair %d: reciprocal table", W, H, l);
                // the staged row of a tap is a row of S, and the level-l rectangle's rows fit the row-tap tables
                CHECK((R.by1 - R.by0) * PYR_SW + 16 * nc <= PYR_SH * PYR_SW, "%dx%d pair %d: S rows", W, H, l);
            }
            passes = std::max(passes, np);
            const int rpp2 = 256 / (K.tw / 4);
            slots += 1024ll * np + 1024ll * ((th + rpp2 - 1) / rpp2);
            for (int y = R.ay0; y <= R.ay1; y++)
                for (int x = R.c0; x <= R.c1; x++) wrote[(size_t)y * w1 + x] = 1;
        }
    size_t missing = 0;
    for (char c : wrote) missing += !c;
    CHECK(missing == 0, "%dx%d pair %d tile %dx%d: %zu level-l pixels unwritten", W, H, l, K.tw, K.th, missing);
    CHECK(plan.passes == passes && plan.slots == slots, "%dx%d pair %d: plan %d passes %lld slots, replay %d / %lld", W, H, l,
          plan.passes, plan.slots, passes, slots);
    std::printf("%4dx%-4d pair (%d,%d) tile %3dx%-3d passes %d slots/pixel %.4f\n", W, H, l, l + 1, K.tw, K.th, passes,
                (double)slots / (double)plan.pixels);
}

// pyramid_level_kernel's tile: the span of the first / last entries holds every tap
static void check_level(const Pyr& P, int W, int H, int l) {
    const I2 *xt = P.xt.data() + P.xo[l], *yt = P.yt.data() + P.yo[l];
    for (int t0 = 0; t0 < P.w[l]; t0 += PYR_TW) {
        const int n = std::min(PYR_TW, P.w[l] - t0);
        const PyrSpan s = pyr_tap_span(xt, t0, t0 + n - 1);
        CHECK(s.lo >= 0 && s.hi < P.w[l - 1] && s.hi - (s.lo & ~15) < PYR_SW, "%dx%d level %d columns", W, H, l);
        for (int x = t0; x < t0 + n; x++) CHECK(lo(xt[x]) >= s.lo && hi(xt[x]) <= s.hi, "%dx%d level %d column %d", W, H, l, x);
    }
    for (int t0 = 0; t0 < P.h[l]; t0 += PYR_TH) {
        const int n = std::min(PYR_TH, P.h[l] - t0);
        const PyrSpan s = pyr_tap_span(yt, t0, t0 + n - 1);
        CHECK(s.lo >= 0 && s.hi < P.h[l - 1] && s.hi - s.lo + 1 <= PYR_SH, "%dx%d level %d rows", W, H, l);
        for (int y = t0; y < t0 + n; y++) CHECK(lo(yt[y]) >= s.lo && hi(yt[y]) <= s.hi, "%dx%d level %d row %d", W, H, l, y);
    }
}

int main() {
    for (int n = 1; n < PYR_RECIP_N; n++) {
        const unsigned m = pyr_recip20(n);
        CHECK((int)(m >> 12) == 256 / n, "256 / %d", n);
        for (unsigned i = 0; i <= 2048; i++) CHECK((int)((i * m) >> 20) == (int)i / n, "%u / %d", i, n);
    }
    const int sizes[][2] = {{640, 480}, {1280, 720}, {1242, 375}, {1920, 1080}, {64, 48}, {97, 75}, {333, 251}, {770, 500}};
    // candidate tiles: the kernel's, then a wider, a flatter, a taller and a smaller one under roomy capacities
    const PyrCaps roomy[] = {{128, 32, 256, 192, 192, 192, 16, 4096}, {64, 32, 256, 192, 192, 192, 16, 4096},
                             {32, 128, 256, 192, 192, 192, 16, 4096}, {80, 48, 256, 192, 192, 192, 16, 4096}};
    for (auto& wh : sizes) {
        const Pyr P = build(wh[0], wh[1]);
        for (int l = 1; l < 8; l++) check_level(P, wh[0], wh[1], l);
        for (int l = 1; l + 1 < 8; l++) {
            check_pair(P, wh[0], wh[1], l, PYR_CAPS, true);
            for (auto& K : roomy) check_pair(P, wh[0], wh[1], l, K, false);
        }
    }
    std::printf("%d failures\n", fails);
    return fails != 0;
}
