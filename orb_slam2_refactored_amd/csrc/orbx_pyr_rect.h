// orbx_pyr_rect.h — the rectangles the pyramid kernels work on, read from the resize tap tables
// (xtab[dx].x = sx0 | sx1 << 16, ytab[dy].x = sy0 | sy1 << 16; orbx_pyramid.h), and the host's replay of
// them for one level pair: capacities, work split, pass count and the issued-slot model (DESIGN §4
// "Pyramid").  One piece of code for the kernels, the host checks and tests/native/pyr_rect_check.cpp;
// no HIP types, so a plain C++ compiler builds it (T2: any struct with int members x, y).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define PYR_HD __host__ __device__ __forceinline__
#else
#define PYR_HD inline
#endif

namespace orbamd {

constexpr int PYR_TW = 64, PYR_TH = 64;     // output tile of a workgroup
constexpr int PYR_SW = 144, PYR_SH = 128;   // LDS source tile capacity (scale factor <= ~1.9)
constexpr int PYR_PF = 5;                   // 16-byte staging pieces per thread: rows x pieces <= 5 x 256
constexpr int PP_MAXP = 8;                  // level-l row passes per thread
constexpr int PP_MAXC = 96, PP_MAXR = 96;   // level-l rectangle columns / rows the tables hold
constexpr int PYR_RECIP_N = PP_MAXC / 4 + 1;   // pyr_recip20's domain: n < PYR_RECIP_N

// cv::resize INTER_LINEAR tables of one level (sw x sh -> dw x dh), appended to xtab / ytab: the same
// arithmetic as OpenCV's (float coordinate, 11-bit coefficients rounded to nearest even, the source
// index clipped to the image).  xtab[dx] = {sx0 | sx1 << 16, a0 | a1 << 16}, ytab[dy] likewise.
template <class T2>
inline void pyr_resize_tables(int sw, int sh, int dw, int dh, std::vector<T2>& xtab, std::vector<T2>& ytab) {
    auto coef = [](float v) { return std::min(std::max((int)std::lrintf(v), -32768), 32767); };
    auto entry = [](int a, int b) {
        T2 v;
        v.x = a, v.y = b;
        return v;
    };
    const double scale_x = 1. / ((double)dw / sw), scale_y = 1. / ((double)dh / sh);
    int xmax = dw;
    std::vector<int> sxs(dw), a0s(dw), a1s(dw);
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = (int)std::floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx + 1 >= sw) {
            xmax = std::min(xmax, dx);
            if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        }
        sxs[dx] = sx;
        a0s[dx] = coef((1.f - fx) * 2048);
        a1s[dx] = coef(fx * 2048);
    }
    for (int dx = 0; dx < dw; dx++) {
        int sx0 = sxs[dx], sx1 = std::min(sxs[dx] + 1, sw - 1), a0 = a0s[dx], a1 = a1s[dx];
        if (dx >= xmax) { sx1 = sx0; a0 = 2048; a1 = 0; }
        xtab.push_back(entry(sx0 | (sx1 << 16), (a0 & 0xffff) | (a1 << 16)));
    }
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = (int)std::floor(fy);
        fy -= sy;
        const int b0 = coef((1.f - fy) * 2048), b1 = coef(fy * 2048);
        auto clip = [&](int y) { return y < 0 ? 0 : (y >= sh ? sh - 1 : y); };
        ytab.push_back(entry(clip(sy) | (clip(sy + 1) << 16), (b0 & 0xffff) | (b1 << 16)));
    }
}

// The source span [lo, hi] that table entries i0..i1 tap.  Both taps are non-decreasing in the entry
// index (sx0 = clamp(floor((dx + 0.5) s - 0.5)), sx1 = sx0 + 1 clipped to the source's last pixel), so the
// span is the first entry's lower tap to the last entry's upper tap; pyr_pair_plan re-checks that over
// every tap.
struct PyrSpan { int lo, hi; };
template <class T2>
PYR_HD PyrSpan pyr_tap_span(const T2* tab, int i0, int i1) {
    return PyrSpan{(int)(tab[i0].x & 0xffff), (int)((unsigned)tab[i1].x >> 16)};
}

// pyramid_pair_kernel's two rectangles for the level-(l+1) tile (tx0, ty0, tw x th): the level-l
// rectangle [c0, c1] x [ay0, ay1] the tile taps (c0 rounded down to a dword: the extra columns are true
// level-l pixels, computed and written like the rest), and the level-(l-1) rectangle [xa, bx1] x
// [by0, by1] that rectangle taps (xa rounded down to a 16-byte staging piece).  xt1 / yt1: level l's
// tables, xt2 / yt2: level l+1's.
struct PyrPairRect { int c0, c1, ay0, ay1, xa, bx1, by0, by1; };
template <class T2>
PYR_HD PyrPairRect pyr_pair_rect(const T2* xt1, const T2* yt1, const T2* xt2, const T2* yt2, int tx0, int ty0,
                                 int tw, int th) {
    const PyrSpan ax = pyr_tap_span(xt2, tx0, tx0 + tw - 1), ay = pyr_tap_span(yt2, ty0, ty0 + th - 1);
    PyrPairRect R;
    R.c0 = ax.lo & ~3, R.c1 = ax.hi, R.ay0 = ay.lo, R.ay1 = ay.hi;
    const PyrSpan bx = pyr_tap_span(xt1, R.c0, R.c1), by = pyr_tap_span(yt1, R.ay0, R.ay1);
    R.xa = bx.lo & ~15, R.bx1 = bx.hi, R.by0 = by.lo, R.by1 = by.hi;
    return R;
}

// ceil(2^20 / n), 1 <= n < 2^12: i / n = (i * m) >> 20 for 0 <= i <= 2048 (the error i (m - 2^20 / n) /
// 2^20 < 2^-9 never reaches the next integer: the fraction of i / n is at most 1 - 1 / n)
constexpr unsigned pyr_recip20(int n) { return (unsigned)(((1 << 20) + n - 1) / n); }

// Host replay of pyramid_pair_kernel over every tile of the pair (levels l-1, l, l+1 of sizes w0 x h0,
// w1 x h1, w2 x h2) for the tile and capacities K: ok when every tap of every tile lies in its rectangle (so the
// first / last reading of pyr_tap_span is the true span), every capacity holds and the written level-l
// rectangles cover level l.  passes: the largest level-l pass count of a tile; slots: pixel slots
// issued (256 threads x 4 pixels per pass, both levels, every tile), pixels: w1 h1 + w2 h2.
struct PyrCaps { int tw, th, sw, sh, maxc, maxr, maxp, pieces; };   // a kernel form's tile and LDS capacities
constexpr PyrCaps PYR_CAPS{PYR_TW, PYR_TH, PYR_SW, PYR_SH, PP_MAXC, PP_MAXR, PP_MAXP, PYR_PF * 256};
struct PyrPairPlan {
    bool ok;
    int passes, max_ncol, max_nrow;
    long long slots, pixels;
};
template <class T2>
inline PyrPairPlan pyr_pair_plan(int w0, int h0, int w1, int h1, int w2, int h2, const T2* xt1, const T2* yt1,
                                 const T2* xt2, const T2* yt2, const PyrCaps& K = PYR_CAPS) {
    PyrPairPlan P{false, 0, 0, 0, 0, (long long)w1 * h1 + (long long)w2 * h2};
    auto lo = [](const T2& v) { return (int)(v.x & 0xffff); };
    auto hi = [](const T2& v) { return (int)((unsigned)v.x >> 16); };
    // every entry's taps inside [s.lo, s.hi], itself inside [0, n)
    auto inside = [&](const T2* tab, int i0, int i1, PyrSpan s, int n) {
        if (s.lo < 0 || s.hi >= n || s.lo > s.hi) return false;
        for (int i = i0; i <= i1; i++)
            if (lo(tab[i]) < s.lo || hi(tab[i]) > s.hi || lo(tab[i]) > hi(tab[i])) return false;
        return true;
    };
    const int tw_max = K.tw, th_max = K.th;
    if (tw_max % 4 || tw_max < 4 || tw_max > 256 || th_max < 1) return P;
    const int rpp2 = 256 / (tw_max / 4);   // level-(l+1) rows per pass
    int covx = 0, covy = 0;                // level-l columns / rows written so far
    for (int ty0 = 0; ty0 < h2; ty0 += th_max) {
        const int th = std::min(th_max, h2 - ty0);
        int covx_row = 0;
        for (int tx0 = 0; tx0 < w2; tx0 += tw_max) {
            const int tw = std::min(tw_max, w2 - tx0);
            const PyrPairRect R = pyr_pair_rect(xt1, yt1, xt2, yt2, tx0, ty0, tw, th);
            if (!inside(xt2, tx0, tx0 + tw - 1, PyrSpan{R.c0, R.c1}, w1) ||
                !inside(yt2, ty0, ty0 + th - 1, PyrSpan{R.ay0, R.ay1}, h1) ||
                !inside(xt1, R.c0, R.c1, PyrSpan{R.xa, R.bx1}, w0) || !inside(yt1, R.ay0, R.ay1, PyrSpan{R.by0, R.by1}, h0))
                return P;
            const int ncol = R.c1 - R.c0 + 1, nrow = R.ay1 - R.ay0 + 1;
            const int ncq = (ncol + 3) / 4, rpp = 256 / ncq, np = (nrow + rpp - 1) / rpp;
            const int nc = ((R.bx1 - R.xa) >> 4) + 1, bh = R.by1 - R.by0 + 1;
            // S holds the level-l rectangle (and the 8-byte windows of the level-(l+1) taps past it), then
            // the tables, the pass count, and the staged level-(l-1) pieces
            if (4 * ncq + 8 > K.sw || nrow > K.sh || ncol > K.maxc || nrow > K.maxr || np > K.maxp || 16 * nc > K.sw ||
                bh > K.sh || bh * nc > K.pieces)
                return P;
            if (R.c0 > covx_row || R.ay0 > covy) return P;   // a gap no workgroup writes
            covx_row = std::max(covx_row, R.c1 + 1);
            if (tx0 + tw == w2) {
                if (covx_row != w1) return P;
                covx = w1;
            }
            if (tx0 + tw == w2 && ty0 + th == h2 && R.ay1 + 1 != h1) return P;
            P.passes = std::max(P.passes, np);
            P.max_ncol = std::max(P.max_ncol, ncol);
            P.max_nrow = std::max(P.max_nrow, nrow);
            P.slots += 1024ll * np + 1024ll * ((th + rpp2 - 1) / rpp2);
            if (tx0 + tw == w2) covy = std::max(covy, R.ay1 + 1);
        }
    }
    P.ok = covx == w1 && covy == h1 && P.passes >= 1;
    return P;
}

}  // namespace orbamd
