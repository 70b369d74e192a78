/*
 * orb_oracle.cpp — CPU restatement of the reference hot path.  TEST INFRASTRUCTURE ONLY.
 *
 * ===========================================================================================
 *  This file is the parity ORACLE.  Only tests/, __graft_entry__.smoke() and bench.py's
 *  cpu_baseline leg may load it.  The product (orb_slam2_refactored_amd/) never links,
 *  imports or calls it; the product fails loudly when its HIP library is missing.
 * ===========================================================================================
 *
 * What it restates (file:line into /root/reference):
 *   ORBextractor   src/ORBextractor.cc:67-828   (Init, ComputePyramid, DetectFAST,
 *                  QuadTreeSuppression + QTreeNode::divide, IC_Angle, ComputeOrbDescriptor,
 *                  Extract) — with std::list / std::sort from the real libstdc++, so the
 *                  quadtree's list order and unstable-sort tie order are the library's own.
 *   OpenCV 4.x generic CPU paths the extractor calls [ext, not vendored, version unpinned]:
 *                  cv::resize INTER_LINEAR 8U (fixed point, SIMD vertical rounding),
 *                  cv::FAST TYPE_9_16 + cornerScore<16> + 3x3 NMS, GaussianBlur 7x7 sigma 2
 *                  bit-exact Q8 (error-diffused taps) REFLECT_101, cv::fastAtan2, cvRound.
 *   ORBmatcher     src/ORBmatcher.cc:60-247 (PatchDistance, ComputeStereoMatches),
 *                  :384-404 (CheckDistEpipolarLine), :477-507 (best /
 *                  second-best loop), :768-866 (SearchForTriangulation), :1449-1457.
 *   LocalBA        src/Optimizer.cc:491-736 and the vendored g2o it drives:
 *                  core/optimization_algorithm_levenberg.cpp:61-189, core/sparse_optimizer.cpp
 *                  (:206-264 active set, :354-435 optimize/update), core/block_solver.hpp
 *                  (:353-486 Schur, :501-604 buildSystem / lambda), core/base_binary_edge.hpp
 *                  :54-120, core/robust_kernel_impl.cpp:65-91, types/types_six_dof_expmap.{h,cpp},
 *                  types/se3quat.h, types/types_sba.h — Eigen replaced by explicit fp64 code,
 *                  SimplicialLDLT by a dense LDLT of the reduced camera system.
 *   DBoW2          Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1130-1263 (transform), :1341-1431
 *                  (loadFromTextFile), BowVector.cpp:34-84, FeatureVector.cpp:31-45, FORB.cpp:80-134.
 *   Grid/Project   src/Frame.cc:32-34,71-145 (FeaturesGrid), src/ORBmatcher.cc:53,315-382
 *                  (SearchByProjection(Frame&, const std::vector<MapPoint*>&, float)).
 *   PoseOpt        src/Optimizer.cc:345-489 (4 x optimize(10) with chi2 classification) over
 *                  the unary edges of types_six_dof_expmap.h:143-202 / .cpp:266-364 and
 *                  solvers/linear_solver_dense.h:65-113 (Eigen LDLT -> unpivoted fp64 LDL^T).
 *
 * Parity status: the reference has NO tests, fixtures or golden vectors for this path and
 * cannot be built here (OpenCV / Eigen absent; a shim build is not allowed).  This oracle is
 * therefore "parity unpinned" against a real OpenCV/g2o build; it is pinned only by the
 * known-answer values derivable from the reference text (umax, quotas, pyramid sizes, Gaussian
 * taps, pattern checksum — tests/test_oracle_kat.py) and by libstdc++ itself for the sort.
 * Documented choices where the reference is ambiguous, each a switch (oracle_set_compat, the same
 * modes as the product's orbx_set_opencv_compat):
 *   - cos/sin in ComputeOrbDescriptor (:107).  trig 0 (default): ::cos(double) (no `using namespace
 *     std` in the refactor) => a = (float)cos((double)angle).  trig 1: the float overloads
 *     std::cos(float) / std::sin(float) = glibc cosf / sinf (visible when a `using namespace std` or
 *     a libstdc++ <math.h> wrapper precedes :107).
 *   - cv::resize vertical pass (VResizeLinear<uchar,int,short,FixedPtCast<int,uchar,22>,
 *     VResizeLinearVec_32s8u>).  The vector op rounds ((b0*(S0>>4))>>16 + (b1*(S1>>4))>>16 + 2) >> 2,
 *     and OpenCV's explicit uchar specialisation of VResizeLinear repeats that formula in its unrolled
 *     and scalar tail loops [ext, recalled], so the result does not depend on the build's SIMD width:
 *     resize_simd V = 0 (default) applies it to every column.  The other modes model a tail with
 *     FixedPtCast rounding (S0*b0 + S1*b1 + 2^21) >> 22 after a V-byte vector loop (x += V while
 *     x <= w - V, then x += V/2 while x < w - V/2): V = 8 / 16 / 32 / 64, or 1 (FixedPtCast
 *     everywhere).  They are sensitivity switches, not claimed to match a real build.
 *   - GaussianBlur taps are OpenCV 4.x's error-diffused Q8 [18,34,48,56,48,34,18].
 *   - Compiled -ffp-contract=off: the reference is ISO C++14 (CMakeLists.txt:10-11), under
 *     which GCC does not contract a*b+c.
 */
#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <fstream>
#include <list>
#include <map>
#include <sstream>
#include <string>
#include <limits>
#include <vector>

#include "orbslam2_amd.h"

namespace oracle {

// ---------------------------------------------------------------------------------------------
// OpenCV scalar primitives [ext]
// ---------------------------------------------------------------------------------------------
static inline int cv_round(double v) { return (int)std::lrint(v); }   // _mm_cvtsd_si32: half-even
static inline int cv_round(float v) { return (int)std::lrintf(v); }   // _mm_cvtss_si32
static inline int cv_floor(float v) { return (int)std::floor(v); }
static inline uint8_t sat_u8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }
static inline short sat_short_f(float v) {
    int iv = cv_round(v);
    return (short)(iv < -32768 ? -32768 : iv > 32767 ? 32767 : iv);
}

// cv::fastAtan2 (core/src/mathfuncs_core.simd.hpp, atan_f32): degrees in [0,360).
static float fast_atan2(float y, float x) {
    const float k = (float)(180 / M_PI);
    const float p1 = 0.9997878412794807f * k, p3 = -0.3258083974640975f * k;
    const float p5 = 0.1555786518463281f * k, p7 = -0.04432655554792128f * k;
    float ax = std::fabs(x), ay = std::fabs(y), a, c, c2;
    if (ax >= ay) {
        c = ay / (ax + (float)DBL_EPSILON);
        c2 = c * c;
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    } else {
        c = ax / (ay + (float)DBL_EPSILON);
        c2 = c * c;
        a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
    }
    if (x < 0) a = 180.f - a;
    if (y < 0) a = 360.f - a;
    return a;
}

// Simple owning 8U image with a row stride.
struct Img {
    int rows = 0, cols = 0;
    size_t step = 0;
    std::vector<uint8_t> buf;
    const uint8_t* data = nullptr;   // may alias external memory
    void alloc(int r, int c) {
        rows = r; cols = c; step = (size_t)c;
        buf.assign((size_t)r * c, 0);
        data = buf.data();
    }
    uint8_t* mut_row(int y) { return buf.data() + (size_t)y * step; }
    const uint8_t* row(int y) const { return data + (size_t)y * step; }
    uint8_t at(int y, int x) const { return data[(size_t)y * step + x]; }
};

// OpenCV-build switches (oracle_set_compat); process-wide, set before any extraction
static int g_trig_float = 0;    // 0: (float)::cos((double)angle); 1: cosf / sinf
static int g_resize_simd = 0;   // tail mode V of the resize's vertical pass (see header; 0 = SIMD rounding everywhere)

// First column VResizeLinear computes with its scalar loop ([ext] imgproc/src/resize.cpp: the vector
// op returns x after `for (; x <= w - V; x += V)` and `for (; x < w - V/2; x += V/2)`).
static int resize_tail_x(int w, int V) {
    if (V <= 0) return w;
    if (V == 1) return 0;
    int x = 0;
    for (; x <= w - V; x += V) {}
    for (; x < w - V / 2; x += V / 2) {}
    return x;
}

// cv::resize(src, dst, Size(dw, dh)) with INTER_LINEAR on CV_8UC1 [ext].
static void resize_linear(const Img& src, Img& dst, int dw, int dh) {
    const int sw = src.cols, sh = src.rows;
    dst.alloc(dh, dw);
    const double inv_sx = (double)dw / sw, inv_sy = (double)dh / sh;
    const double scale_x = 1. / inv_sx, scale_y = 1. / inv_sy;
    std::vector<int> xofs(dw);
    std::vector<short> ialpha(2 * dw);
    int xmax = dw;
    for (int dx = 0; dx < dw; dx++) {
        float fx = (float)((dx + 0.5) * scale_x - 0.5);
        int sx = cv_floor(fx);
        fx -= sx;
        if (sx < 0) { fx = 0; sx = 0; }
        if (sx + 1 >= sw) {
            xmax = std::min(xmax, dx);
            if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
        }
        xofs[dx] = sx;
        ialpha[2 * dx] = sat_short_f((1.f - fx) * 2048);
        ialpha[2 * dx + 1] = sat_short_f(fx * 2048);
    }
    std::vector<int> r0(dw), r1(dw);
    auto hrow = [&](int sy, std::vector<int>& D) {
        const uint8_t* S = src.row(sy);
        int dx = 0;
        for (; dx < xmax; dx++) D[dx] = S[xofs[dx]] * ialpha[2 * dx] + S[xofs[dx] + 1] * ialpha[2 * dx + 1];
        for (; dx < dw; dx++) D[dx] = S[xofs[dx]] * 2048;
    };
    for (int dy = 0; dy < dh; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = cv_floor(fy);
        fy -= sy;
        const int b0 = sat_short_f((1.f - fy) * 2048), b1 = sat_short_f(fy * 2048);
        auto clip = [&](int y) { return y < 0 ? 0 : (y >= sh ? sh - 1 : y); };
        hrow(clip(sy), r0);
        hrow(clip(sy + 1), r1);
        uint8_t* D = dst.mut_row(dy);
        const int xt = resize_tail_x(dw, g_resize_simd);
        for (int x = 0; x < xt; x++) {   // VResizeLinearVec_32s8u: v_mul_hi of the packed S >> 4, v_rshr_pack_u<2>
            const int s0 = std::min(r0[x] >> 4, 32767), s1 = std::min(r1[x] >> 4, 32767);
            const int v = ((s0 * b0) >> 16) + ((s1 * b1) >> 16);
            D[x] = sat_u8((v + 2) >> 2);
        }
        for (int x = xt; x < dw; x++)   // scalar tail: FixedPtCast<int, uchar, 22>
            D[x] = sat_u8((r0[x] * b0 + r1[x] * b1 + (1 << 21)) >> 22);
    }
}

// cv::FAST(img, kps, threshold, nonmax=true), TYPE_9_16 [ext, features2d/src/fast.cpp].
struct RawKp { float x, y, response; };

static const int kCircle[16][2] = {{0, 3}, {1, 3}, {2, 2}, {3, 1}, {3, 0}, {3, -1}, {2, -2}, {1, -3},
                                   {0, -3}, {-1, -3}, {-2, -2}, {-3, -1}, {-3, 0}, {-3, 1}, {-2, 2}, {-1, 3}};

static int corner_score16(const uint8_t* p, const int* off, int threshold) {
    const int N = 25;
    int v = p[0];
    short d[N];
    for (int k = 0; k < N; k++) d[k] = (short)(v - p[off[k]]);
    int a0 = threshold;
    for (int k = 0; k < 16; k += 2) {
        int a = std::min((int)d[k + 1], (int)d[k + 2]);
        a = std::min(a, (int)d[k + 3]);
        if (a <= a0) continue;
        a = std::min(a, (int)d[k + 4]);
        a = std::min(a, (int)d[k + 5]);
        a = std::min(a, (int)d[k + 6]);
        a = std::min(a, (int)d[k + 7]);
        a = std::min(a, (int)d[k + 8]);
        a0 = std::max(a0, std::min(a, (int)d[k]));
        a0 = std::max(a0, std::min(a, (int)d[k + 9]));
    }
    int b0 = -a0;
    for (int k = 0; k < 16; k += 2) {
        int b = std::max((int)d[k + 1], (int)d[k + 2]);
        b = std::max(b, (int)d[k + 3]);
        b = std::max(b, (int)d[k + 4]);
        b = std::max(b, (int)d[k + 5]);
        if (b >= b0) continue;
        b = std::max(b, (int)d[k + 6]);
        b = std::max(b, (int)d[k + 7]);
        b = std::max(b, (int)d[k + 8]);
        b0 = std::min(b0, std::max(b, (int)d[k]));
        b0 = std::min(b0, std::max(b, (int)d[k + 9]));
    }
    return -b0 - 1;
}

// FAST on the view rows [y0,y1) x cols [x0,x1) of `im`; keypoints in view coordinates.
static void fast916(const Img& im, int x0, int y0, int x1, int y1, int threshold, std::vector<RawKp>& out) {
    out.clear();
    const int rows = y1 - y0, cols = x1 - x0;
    const int step = (int)im.step;
    int off[25];
    for (int k = 0; k < 16; k++) off[k] = kCircle[k][0] + kCircle[k][1] * step;
    for (int k = 16; k < 25; k++) off[k] = off[k - 16];
    threshold = std::min(std::max(threshold, 0), 255);
    uint8_t tab[512];
    for (int i = -255; i <= 255; i++) tab[i + 255] = (uint8_t)(i < -threshold ? 1 : i > threshold ? 2 : 0);
    if (rows < 7 || cols < 7) return;
    std::vector<uint8_t> sbuf[3];
    std::vector<int> cpos[3];
    for (int b = 0; b < 3; b++) { sbuf[b].assign(cols, 0); cpos[b].clear(); }
    for (int i = 3; i < rows - 2; i++) {
        std::vector<uint8_t>& curr = sbuf[(i - 3) % 3];
        std::vector<int>& cp = cpos[(i - 3) % 3];
        std::fill(curr.begin(), curr.end(), 0);
        cp.clear();
        if (i < rows - 3) {
            const uint8_t* ptr = im.row(y0 + i) + x0 + 3;
            for (int j = 3; j < cols - 3; j++, ptr++) {
                const int v = ptr[0];
                const uint8_t* t = &tab[0] - v + 255;
                int d = t[ptr[off[0]]] | t[ptr[off[8]]];
                if (d == 0) continue;
                d &= t[ptr[off[2]]] | t[ptr[off[10]]];
                d &= t[ptr[off[4]]] | t[ptr[off[12]]];
                d &= t[ptr[off[6]]] | t[ptr[off[14]]];
                if (d == 0) continue;
                d &= t[ptr[off[1]]] | t[ptr[off[9]]];
                d &= t[ptr[off[3]]] | t[ptr[off[11]]];
                d &= t[ptr[off[5]]] | t[ptr[off[13]]];
                d &= t[ptr[off[7]]] | t[ptr[off[15]]];
                if (d & 1) {
                    int vt = v - threshold, count = 0;
                    for (int k = 0; k < 25; k++) {
                        if (ptr[off[k]] < vt) {
                            if (++count > 8) {
                                cp.push_back(j);
                                curr[j] = (uint8_t)corner_score16(ptr, off, threshold);
                                break;
                            }
                        } else count = 0;
                    }
                }
                if (d & 2) {
                    int vt = v + threshold, count = 0;
                    for (int k = 0; k < 25; k++) {
                        if (ptr[off[k]] > vt) {
                            if (++count > 8) {
                                cp.push_back(j);
                                curr[j] = (uint8_t)corner_score16(ptr, off, threshold);
                                break;
                            }
                        } else count = 0;
                    }
                }
            }
        }
        if (i == 3) continue;
        const std::vector<uint8_t>& prev = sbuf[(i - 4 + 3) % 3];
        const std::vector<uint8_t>& pprev = sbuf[(i - 5 + 3) % 3];
        const std::vector<int>& pc = cpos[(i - 4 + 3) % 3];
        for (int j : pc) {
            const int s = prev[j];
            if (s > prev[j + 1] && s > prev[j - 1] && s > pprev[j - 1] && s > pprev[j] && s > pprev[j + 1] &&
                s > curr[j - 1] && s > curr[j] && s > curr[j + 1])
                out.push_back({(float)j, (float)(i - 1), (float)s});
        }
    }
}

// cv::GaussianBlur(src, dst, Size(7,7), 2, 2, BORDER_REFLECT_101), 8U bit-exact path [ext].
static void gaussian_taps_q8(int taps[7]) {
    // getGaussianKernelBitExact (n=7, sigma=2) then getGaussianKernelFixedPoint_ED(.., 8 bits).
    const double sigma = 2.0, scale2 = -0.125 / (sigma * sigma);
    double vals[3], sum = 0;
    for (int i = 0, x = -6; i < 3; i++, x += 2) { vals[i] = std::exp((double)(x * x) * scale2); sum += vals[i]; }
    sum = sum * 2 + 1.0;
    const double mul = 1.0 / sum;
    double err = 0;
    int64_t s = 0;
    for (int i = 0; i < 3; i++) {
        double adj = vals[i] * mul * 256.0 + err;
        int v = cv_round(adj);
        err = adj - v;
        taps[i] = taps[6 - i] = v;
        s += v;
    }
    taps[3] = (int)(256 - 2 * s);
}

static inline int reflect101(int i, int n) {
    if (n == 1) return 0;
    while (i < 0 || i >= n) {
        if (i < 0) i = -i;
        if (i >= n) i = 2 * n - 2 - i;
    }
    return i;
}

static void gaussian_blur(const Img& src, Img& dst) {
    int k[7];
    gaussian_taps_q8(k);
    const int W = src.cols, H = src.rows;
    dst.alloc(H, W);
    std::vector<uint32_t> h((size_t)W * H);   // Q8 horizontal sums (ufixedpoint16, exact)
    for (int y = 0; y < H; y++) {
        const uint8_t* S = src.row(y);
        for (int x = 0; x < W; x++) {
            uint32_t acc = 0;
            for (int t = 0; t < 7; t++) acc += (uint32_t)k[t] * S[reflect101(x + t - 3, W)];
            h[(size_t)y * W + x] = acc;
        }
    }
    for (int y = 0; y < H; y++) {
        uint8_t* D = dst.mut_row(y);
        for (int x = 0; x < W; x++) {
            uint32_t acc = 0;   // ufixedpoint32, Q16
            for (int t = 0; t < 7; t++) acc += (uint32_t)k[t] * h[(size_t)reflect101(y + t - 3, H) * W + x];
            D[x] = sat_u8((int)((acc + (1u << 15)) >> 16));
        }
    }
}

// ---------------------------------------------------------------------------------------------
// ORBextractor (src/ORBextractor.cc)
// ---------------------------------------------------------------------------------------------
static const int kPattern[1024] = {
#include "orb_pattern31.inc"
};

struct Kp {   // cv::KeyPoint fields used by the extractor
    float x, y, size, angle, response;
    int octave;
};

struct Params {
    int nfeatures;
    float scaleFactor;
    int nlevels, iniThFAST, minThFAST;
};

struct Extractor {
    Params p;
    std::vector<int> quota, umax;
    std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
    std::vector<Img> levels, blurred;

    explicit Extractor(const Params& prm) : p(prm) { init(); }

    // ORBextractor::Init (:697-741) + ComputeNumFeaturesPerScale (:472-487)
    void init() {
        umax.assign(16, 0);
        const int vmax = (int)std::floor(15 * std::sqrt(2.) / 2 + 1);
        const int vmin = (int)std::ceil(15 * std::sqrt(2.) / 2);
        for (int v = 0; v <= vmax; ++v) umax[v] = cv_round(std::sqrt(15.0 * 15 - v * v));
        for (int v = 15, v0 = 0; v >= vmin; --v) {
            while (umax[v0] == umax[v0 + 1]) ++v0;
            umax[v] = v0;
            ++v0;
        }
        const int L = p.nlevels;
        scale.resize(L); inv_scale.resize(L); sigma2.resize(L); inv_sigma2.resize(L);
        float s = 1.f;
        for (int l = 0; l < L; l++) {
            scale[l] = s; inv_scale[l] = 1.f / s; sigma2[l] = s * s; inv_sigma2[l] = 1.f / (s * s);
            s *= p.scaleFactor;
        }
        quota.resize(L);
        const double factor = 1 / p.scaleFactor;   // int / float: float division, widened
        double nf = p.nfeatures * (1 - factor) / (1 - std::pow(factor, L));
        int sum = 0;
        for (int l = 0; l < L - 1; l++) {
            quota[l] = cv_round(nf);
            sum += quota[l];
            nf *= factor;
        }
        quota[L - 1] = std::max(p.nfeatures - sum, 0);
    }

    // ComputePyramid (:455-470)
    void pyramid(const Img& image) {
        levels.assign(p.nlevels, Img());
        levels[0].alloc(image.rows, image.cols);
        for (int y = 0; y < image.rows; y++) std::memcpy(levels[0].mut_row(y), image.row(y), image.cols);
        for (int l = 1; l < p.nlevels; l++) {
            const int h = cv_round(inv_scale[l] * image.rows);
            const int w = cv_round(inv_scale[l] * image.cols);
            resize_linear(levels[l - 1], levels[l], w, h);
        }
    }

    // DetectFAST (:489-540); roi = inset by BORDER 16 (:755-760)
    static void detect_fast(const Img& im, int rx, int ry, int rw, int rh, int thIni, int thMin, std::vector<Kp>& kps) {
        kps.clear();
        const int minx = rx, miny = ry, maxx = rx + rw, maxy = ry + rh;
        const int gridw = rw / 30, gridh = rh / 30;
        if (gridw <= 0 || gridh <= 0) return;   // reference divides by zero here (UB); we emit none
        const int cellw = (int)std::ceil(1. * rw / gridw), cellh = (int)std::ceil(1. * rh / gridh);
        std::vector<RawKp> cell;
        for (int cy = 0, y0 = miny; cy < gridh && y0 + 6 < maxy; cy++, y0 += cellh) {
            for (int cx = 0, x0 = minx; cx < gridw && x0 + 6 < maxx; cx++, x0 += cellw) {
                const int y1 = std::min(y0 + cellh + 6, maxy), x1 = std::min(x0 + cellw + 6, maxx);
                fast916(im, x0, y0, x1, y1, thIni, cell);
                if (cell.empty()) fast916(im, x0, y0, x1, y1, thMin, cell);
                for (const RawKp& r : cell) kps.push_back({r.x + x0, r.y + y0, 7.f, -1.f, r.response, 0});
            }
        }
    }

    // QTreeNode (:402-452)
    struct Node {
        std::vector<Kp> pts;
        int tlx = 0, tly = 0, brx = 0, bry = 0;
        std::list<Node>::iterator self;
        bool divisible = true;
        void split(std::array<Node, 4>& ch) const {
            const int hx = (int)std::ceil(0.5 * (brx - tlx)), hy = (int)std::ceil(0.5 * (bry - tly));
            const int xm = tlx + hx, ym = tly + hy;
            ch[0].tlx = tlx; ch[0].tly = tly; ch[0].brx = xm;  ch[0].bry = ym;
            ch[1].tlx = xm;  ch[1].tly = tly; ch[1].brx = brx; ch[1].bry = ym;
            ch[2].tlx = tlx; ch[2].tly = ym;  ch[2].brx = xm;  ch[2].bry = bry;
            ch[3].tlx = xm;  ch[3].tly = ym;  ch[3].brx = brx; ch[3].bry = bry;
            for (const Kp& k : pts) {
                const int q = k.x < xm ? (k.y < ym ? 0 : 2) : (k.y < ym ? 1 : 3);
                ch[q].pts.push_back(k);
            }
            for (int i = 0; i < 4; i++) if (ch[i].pts.size() == 1) ch[i].divisible = false;
        }
    };

    // QuadTreeSuppression (:542-693)
    static void quadtree(const std::vector<Kp>& src, int rx, int ry, int rw, int rh, size_t nfeat, std::vector<Kp>& dst) {
        std::vector<Kp> out;
        if (src.empty() || rw <= 0 || rh <= 0) { dst.clear(); return; }
        const int nroots = cv_round(1. * rw / rh);
        const double hx = 1. * rw / nroots;
        std::list<Node> nodes;
        std::vector<Node*> roots(nroots);
        for (int i = 0; i < nroots; i++) {
            Node n;
            n.tlx = (int)(rx + hx * i); n.tly = ry;
            n.brx = (int)(rx + hx * (i + 1)); n.bry = ry + rh;
            nodes.push_back(n);
            roots[i] = &nodes.back();
        }
        for (const Kp& k : src) roots[(int)((k.x - rx) / hx)]->pts.push_back(k);
        for (auto it = nodes.begin(); it != nodes.end();) {
            if (it->pts.empty()) it = nodes.erase(it);
            else { if (it->pts.size() == 1) it->divisible = false; ++it; }
        }
        struct Div { size_t size; const Node* node; };
        std::vector<Div> divs;
        auto push_children = [&](const std::array<Node, 4>& ch) {
            for (const Node& c : ch) {
                if (c.pts.empty()) continue;
                nodes.push_front(c);
                if (c.pts.size() > 1) {
                    nodes.front().self = nodes.begin();
                    divs.push_back({c.pts.size(), &nodes.front()});
                }
            }
        };
        bool done = false;
        while (!done) {
            size_t before = nodes.size();
            divs.clear();
            for (auto it = nodes.begin(); it != nodes.end();) {
                if (!it->divisible) { ++it; continue; }
                std::array<Node, 4> ch;
                it->split(ch);
                push_children(ch);
                it = nodes.erase(it);
            }
            if (nodes.size() >= nfeat || nodes.size() == before) break;
            if (nodes.size() + 3 * divs.size() > nfeat) {
                while (!done) {
                    before = nodes.size();
                    std::vector<Div> prev = divs;
                    divs.clear();
                    std::sort(prev.begin(), prev.end(), [](const Div& a, const Div& b) { return a.size > b.size; });
                    for (const Div& d : prev) {
                        std::array<Node, 4> ch;
                        d.node->split(ch);
                        push_children(ch);
                        nodes.erase(d.node->self);
                        if (nodes.size() >= nfeat) break;
                    }
                    if (nodes.size() >= nfeat || nodes.size() == before) done = true;
                }
            }
        }
        for (const Node& n : nodes) {
            const Kp* best = nullptr;
            float maxr = 0.f;
            for (const Kp& k : n.pts)
                if (k.response > maxr) { maxr = k.response; best = &k; }
            out.push_back(*best);
        }
        dst.swap(out);
    }

    // IC_Angle (:74-101)
    float ic_angle(const Img& im, float px, float py) const {
        int m01 = 0, m10 = 0;
        const uint8_t* c = im.row(cv_round(py)) + cv_round(px);
        for (int u = -15; u <= 15; ++u) m10 += u * c[u];
        const int step = (int)im.step;
        for (int v = 1; v <= 15; ++v) {
            int vs = 0;
            const int d = umax[v];
            for (int u = -d; u <= d; ++u) {
                const int vp = c[u + v * step], vm = c[u - v * step];
                vs += vp - vm;
                m10 += u * (vp + vm);
            }
            m01 += v * vs;
        }
        return fast_atan2((float)m01, (float)m10);
    }

    // ComputeOrbDescriptor (:103-140)
    static void describe(const Kp& k, const Img& im, uint8_t* desc) {
        const float factorPI = (float)(M_PI / 180.f);
        const float angle = k.angle * factorPI;
        float a, b;
        if (g_trig_float) {   // std::cos(float) / std::sin(float): glibc cosf / sinf
            a = std::cos(angle);
            b = std::sin(angle);
        } else {              // ::cos(double) / ::sin(double)
            a = (float)std::cos((double)angle);
            b = (float)std::sin((double)angle);
        }
        const uint8_t* c = im.row(cv_round(k.y)) + cv_round(k.x);
        const int step = (int)im.step;
        auto val = [&](int idx) {
            const float x = (float)kPattern[2 * idx], y = (float)kPattern[2 * idx + 1];
            return (int)c[cv_round(x * b + y * a) * step + cv_round(x * a - y * b)];
        };
        for (int i = 0; i < 32; i++) {
            int byte = 0;
            for (int j = 0; j < 8; j++) {
                const int p = i * 16 + 2 * j;
                byte |= (val(p) < val(p + 1)) << j;
            }
            desc[i] = (uint8_t)byte;
        }
    }

    // Extract (:743-820).  Returns total; fills kps/desc (cap checked by caller).
    std::vector<std::vector<Kp>> per_level;
    int extract(const Img& image, std::vector<Kp>& kps, std::vector<uint8_t>& desc) {
        const int L = p.nlevels;
        per_level.assign(L, {});
        pyramid(image);
        int total = 0;
        for (int l = 0; l < L; l++) {
            const Img& im = levels[l];
            const int rx = 16, ry = 16, rw = im.cols - 32, rh = im.rows - 32;
            std::vector<Kp>& lk = per_level[l];
            if (rw > 0 && rh > 0) {
                detect_fast(im, rx, ry, rw, rh, p.iniThFAST, p.minThFAST, lk);
                quadtree(lk, rx, ry, rw, rh, (size_t)quota[l], lk);
            }
            // else: level narrower/shorter than 2*BORDER.  The reference then runs FAST on the
            // whole level (:497-500), skips the quadtree (:544-545) and IC_Angle reads up to 15 px
            // outside the image (or divides by zero when the level is < 30 px): undefined
            // behaviour.  Documented deviation: such a level contributes no keypoints.
            for (Kp& k : lk) {
                k.octave = l;
                k.size = scale[l] * 31;
                k.angle = ic_angle(im, k.x, k.y);
            }
            total += (int)lk.size();
        }
        if (total == 0) return 0;
        desc.assign((size_t)total * 32, 0);
        kps.clear();
        blurred.assign(L, Img());
        int off = 0;
        for (int l = 0; l < L; l++) {
            std::vector<Kp>& lk = per_level[l];
            if (lk.empty()) continue;
            gaussian_blur(levels[l], blurred[l]);
            for (size_t i = 0; i < lk.size(); i++) describe(lk[i], blurred[l], &desc[(size_t)(off + i) * 32]);
            off += (int)lk.size();
            if (l > 0)
                for (Kp& k : lk) { k.x *= scale[l]; k.y *= scale[l]; }
            kps.insert(kps.end(), lk.begin(), lk.end());
        }
        return total;
    }
};

static Params to_params(const orbx_params* p) {
    return Params{p->nfeatures, p->scaleFactor, p->nlevels, p->iniThFAST, p->minThFAST};
}
static Img view(const uint8_t* img, int rows, int cols, size_t step) {
    Img im;
    im.rows = rows; im.cols = cols; im.step = step; im.data = img;
    return im;
}
static void to_abi(const Kp& k, orbx_keypoint* o) {
    o->x = k.x; o->y = k.y; o->size = k.size; o->angle = k.angle; o->response = k.response;
    o->octave = k.octave; o->class_id = -1;
}

// ---------------------------------------------------------------------------------------------
// ORBmatcher
// ---------------------------------------------------------------------------------------------
static int hamming(const uint8_t* a, const uint8_t* b) {   // :1449-1457
    int d = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t x, y;
        std::memcpy(&x, a + 4 * i, 4);
        std::memcpy(&y, b + 4 * i, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

// CheckDistEpipolarLine (:384-404)
static bool epipolar_ok(float x1, float y1, float x2, float y2, const float* F, float sigma2) {
    const float a = x1 * F[0] + y1 * F[3] + F[6];
    const float b = x1 * F[1] + y1 * F[4] + F[7];
    const float c = x1 * F[2] + y1 * F[5] + F[8];
    const float num = a * x2 + b * y2 + c;
    const float den = a * a + b * b;
    if (den == 0) return false;
    const float dsqr = num * num / den;
    return dsqr < 3.84 * sigma2;
}

// ---------------------------------------------------------------------------------------------
// LocalBA: g2o Levenberg-Marquardt with Schur complement (fp64)
// ---------------------------------------------------------------------------------------------
struct Quat { double x, y, z, w; };

// branch (may be null): 0 for t > 0, else 1 + i of the largest diagonal element
static Quat quat_from_R(const double* m, int* branch = nullptr) {   // Eigen::Quaterniond(const Matrix3d&)
    Quat q;
    const double t = m[0] + m[4] + m[8];
    if (branch) *branch = 0;
    if (t > 0) {
        double s = std::sqrt(t + 1.0);
        q.w = 0.5 * s;
        s = 0.5 / s;
        q.x = (m[7] - m[5]) * s;
        q.y = (m[2] - m[6]) * s;
        q.z = (m[3] - m[1]) * s;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[3 * i + i]) i = 2;
        if (branch) *branch = 1 + i;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        double s = std::sqrt(m[3 * i + i] - m[3 * j + j] - m[3 * k + k] + 1.0);
        double qv[3];
        qv[i] = 0.5 * s;
        s = 0.5 / s;
        q.w = (m[3 * k + j] - m[3 * j + k]) * s;
        qv[j] = (m[3 * j + i] + m[3 * i + j]) * s;
        qv[k] = (m[3 * k + i] + m[3 * i + k]) * s;
        q.x = qv[0]; q.y = qv[1]; q.z = qv[2];
    }
    return q;
}
static void quat_normalize_pos(Quat& q) {   // SE3Quat::normalizeRotation
    if (q.w < 0) { q.x = -q.x; q.y = -q.y; q.z = -q.z; q.w = -q.w; }
    const double n = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w);
    if (n > 0) { q.x /= n; q.y /= n; q.z /= n; q.w /= n; }
}
static void quat_to_R(const Quat& q, double* R) {   // Eigen toRotationMatrix
    const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
    const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
    const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}
static Quat quat_mul(const Quat& a, const Quat& b) {
    return Quat{a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
                a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
                a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x,
                a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
static void quat_rotate(const Quat& q, const double* v, double* o) {   // Eigen _transformVector
    double uv[3] = {q.y * v[2] - q.z * v[1], q.z * v[0] - q.x * v[2], q.x * v[1] - q.y * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    const double c[3] = {q.y * uv[2] - q.z * uv[1], q.z * uv[0] - q.x * uv[2], q.x * uv[1] - q.y * uv[0]};
    for (int i = 0; i < 3; i++) o[i] = v[i] + q.w * uv[i] + c[i];
}

struct SE3 { Quat q; double t[3]; };

static void se3_map(const SE3& T, const double* X, double* o) {
    quat_rotate(T.q, X, o);
    o[0] += T.t[0]; o[1] += T.t[1]; o[2] += T.t[2];
}

// SE3Quat::exp (se3quat.h:217-257) followed by operator* (:99-105)
static SE3 se3_exp_mul(const double* upd, const SE3& T) {
    const double w[3] = {upd[0], upd[1], upd[2]}, u[3] = {upd[3], upd[4], upd[5]};
    const double theta = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const double O[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
    double O2[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 3; k++) s += O[3 * i + k] * O[3 * k + j];
            O2[3 * i + j] = s;
        }
    double R[9], V[9];
    if (theta < 0.00001) {
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + O[i] + O2[i];
        for (int i = 0; i < 9; i++) V[i] = R[i];
    } else {
        const double s = std::sin(theta), c = std::cos(theta);
        const double a = s / theta, b = (1 - c) / (theta * theta), d = (theta - s) / std::pow(theta, 3);
        for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0 ? 1.0 : 0.0) + a * O[i] + b * O2[i];
        for (int i = 0; i < 9; i++) V[i] = (i % 4 == 0 ? 1.0 : 0.0) + b * O[i] + d * O2[i];
    }
    SE3 E;
    E.q = quat_from_R(R);
    quat_normalize_pos(E.q);
    for (int i = 0; i < 3; i++) E.t[i] = V[3 * i] * u[0] + V[3 * i + 1] * u[1] + V[3 * i + 2] * u[2];
    SE3 out;
    double rt[3];
    quat_rotate(E.q, T.t, rt);
    for (int i = 0; i < 3; i++) out.t[i] = E.t[i] + rt[i];
    out.q = quat_mul(E.q, T.q);
    quat_normalize_pos(out.q);
    return out;
}

// One LM trial as oracle_local_ba_trace records it (tests/oracle_api.py BA_TRIAL_DTYPE has the same
// layout).  The iteration-end fields are filled on the trial that closes an iteration (iter_end = 1);
// loop_end names why the loop ended on the trial that closes its last iteration.
struct oracle_ba_trial {
    int32_t loop, it, q, accepted;     // loop 0 / 1, iteration, trial within the iteration (from 0)
    double lambda, cur, tmp, scale, rho;   // lambda and cur before the trial; scale with its 1e-3
    int32_t iter_end, nbad_tested;     // nbad_tested: the iteration reached the (ini - cur) * 1e3 < ini test
    double ini, cur_end;
    int32_t nbad, loop_end;            // loop_end: BA_END_*
};
enum { BA_END_NONE = 0, BA_END_BUDGET, BA_END_NBAD, BA_END_RHO0, BA_END_Q10, BA_END_STOP };

struct BATrace {
    oracle_ba_trial* rec = nullptr;
    int cap = 0, n = 0, loop = 0;
    oracle_ba_trial* push() {
        oracle_ba_trial* r = n < cap ? &rec[n] : nullptr;
        n++;   // counts past cap, so the caller sees an overflow
        if (r) { std::memset(r, 0, sizeof *r); r->loop = loop; }
        return r;
    }
};

struct BA {
    // problem
    int P, N, E;
    std::vector<SE3> pose;
    std::vector<uint8_t> fixed;
    std::vector<double> X;   // N x 3
    std::vector<int> ep, ek; // edge point, edge pose
    std::vector<uint8_t> stereo;
    std::vector<double> obs, info, cam;
    // edge state
    std::vector<int> level;
    std::vector<uint8_t> robust;
    std::vector<double> err;   // E x 3 (last computed)
    // active set
    std::vector<int> act_edges;
    std::vector<int> hp, hl;   // Hessian index per pose / point (-1 inactive or fixed)
    int np = 0, nl = 0;
    const volatile int32_t* stop = nullptr;
    int stop_after = -1, trials = 0;   // test hook: the flag "rises" once this many LM trials have run
    BATrace* trace = nullptr;          // test hook: a record per LM trial; read-only for the optimisation
    int end_reason = BA_END_NONE;      // why the last optimize() ended (BA_END_NONE: it had nothing to do)

    bool terminate() const { return (stop && *stop) || (stop_after >= 0 && trials >= stop_after); }

    double chi2(int e) const {
        const int d = stereo[e] ? 3 : 2;
        double s = 0;
        for (int i = 0; i < d; i++) s += err[3 * e + i] * info[e] * err[3 * e + i];
        return s;
    }
    void robustify(int e, double chi, double& r0, double& r1) const {
        if (!robust[e]) { r0 = chi; r1 = 1.0; return; }
        const double delta = stereo[e] ? std::sqrt(7.815) : std::sqrt(5.991);
        const double dsqr = delta * delta;
        if (chi <= dsqr) { r0 = chi; r1 = 1.0; }
        else { const double s = std::sqrt(chi); r0 = 2 * s * delta - dsqr; r1 = delta / s; }
    }
    void compute_error(int e) {
        double Xc[3];
        se3_map(pose[ek[e]], &X[3 * ep[e]], Xc);
        const double* c = &cam[5 * e];
        const double* z = &obs[3 * e];
        if (!stereo[e]) {
            err[3 * e + 0] = z[0] - (Xc[0] / Xc[2] * c[0] + c[2]);
            err[3 * e + 1] = z[1] - (Xc[1] / Xc[2] * c[1] + c[3]);
            err[3 * e + 2] = 0;
        } else {
            const float invz = 1.0f / Xc[2];
            const float bf = (float)c[4];
            const double u = Xc[0] * invz * c[0] + c[2];
            const double v = Xc[1] * invz * c[1] + c[3];
            err[3 * e + 0] = z[0] - u;
            err[3 * e + 1] = z[1] - v;
            err[3 * e + 2] = z[2] - (u - (double)(bf * invz));
        }
    }
    bool depth_positive(int e) const {
        double Xc[3];
        se3_map(pose[ek[e]], &X[3 * ep[e]], Xc);
        return Xc[2] > 0.0;
    }
    double active_robust_chi2() const {
        double s = 0;
        for (int e : act_edges) { double r0, r1; robustify(e, chi2(e), r0, r1); s += r0; }
        return s;
    }
    void compute_active_errors() { for (int e : act_edges) compute_error(e); }

    // initializeOptimization(level) (sparse_optimizer.cpp:206-264, :166-190)
    void init_level(int lvl) {
        act_edges.clear();
        std::vector<uint8_t> pa(P, 0), la(N, 0);
        for (int e = 0; e < E; e++) {
            if (level[e] != lvl) continue;   // points are never fixed: edge never all-fixed
            act_edges.push_back(e);
            pa[ek[e]] = 1; la[ep[e]] = 1;
        }
        hp.assign(P, -1); hl.assign(N, -1);
        np = 0; nl = 0;
        for (int i = 0; i < P; i++) if (pa[i] && !fixed[i]) hp[i] = np++;
        for (int i = 0; i < N; i++) if (la[i]) hl[i] = nl++;
    }

    // system
    std::vector<double> Hpp, Hll, Hpl, bp, bl;   // Hpp dense (6np)^2; Hll nl x 9; Hpl per edge 18; b
    std::vector<double> x;                       // 6np + 3nl

    // linearizeOplus + constructQuadraticForm (types_six_dof_expmap.cpp:103-139,188-234;
    // base_binary_edge.hpp:54-120), then copyB.
    void build_system() {
        const int D = 6 * np;
        Hpp.assign((size_t)D * D, 0); Hll.assign((size_t)nl * 9, 0);
        Hpl.assign((size_t)E * 18, 0);
        bp.assign(D, 0); bl.assign((size_t)nl * 3, 0);
        for (int e : act_edges) {
            const SE3& T = pose[ek[e]];
            double Xc[3];
            se3_map(T, &X[3 * ep[e]], Xc);
            double R[9];
            quat_to_R(T.q, R);
            const double x = Xc[0], y = Xc[1], z = Xc[2], z2 = z * z;
            const double* c = &cam[5 * e];
            const double fx = c[0], fy = c[1], bf = c[4];
            const int d = stereo[e] ? 3 : 2;
            double A[3][3] = {{0}}, B[3][6] = {{0}};
            if (!stereo[e]) {
                const double tmp[2][3] = {{fx, 0, -x / z * fx}, {0, fy, -y / z * fy}};
                for (int r = 0; r < 2; r++)
                    for (int j = 0; j < 3; j++) {
                        double s = 0;
                        for (int k = 0; k < 3; k++) s += tmp[r][k] * R[3 * k + j];
                        A[r][j] = -1. / z * s;
                    }
            } else {
                for (int j = 0; j < 3; j++) {
                    A[0][j] = -fx * R[j] / z + fx * x * R[6 + j] / z2;
                    A[1][j] = -fy * R[3 + j] / z + fy * y * R[6 + j] / z2;
                    A[2][j] = A[0][j] - bf * R[6 + j] / z2;
                }
            }
            B[0][0] = x * y / z2 * fx; B[0][1] = -(1 + (x * x / z2)) * fx; B[0][2] = y / z * fx;
            B[0][3] = -1. / z * fx;    B[0][4] = 0;                        B[0][5] = x / z2 * fx;
            B[1][0] = (1 + y * y / z2) * fy; B[1][1] = -x * y / z2 * fy; B[1][2] = -x / z * fy;
            B[1][3] = 0;                     B[1][4] = -1. / z * fy;     B[1][5] = y / z2 * fy;
            if (stereo[e]) {
                B[2][0] = B[0][0] - bf * y / z2; B[2][1] = B[0][1] + bf * x / z2; B[2][2] = B[0][2];
                B[2][3] = B[0][3];               B[2][4] = 0;                     B[2][5] = B[0][5] - bf / z2;
            }
            double r0, r1;
            robustify(e, chi2(e), r0, r1);
            const double w = r1 * info[e];   // weighted information (diagonal)
            double om_r[3];
            for (int r = 0; r < d; r++) om_r[r] = -info[e] * err[3 * e + r] * r1;
            const int il = hl[ep[e]], ip = hp[ek[e]];
            // point block (vertex 0 = point, never fixed)
            for (int i = 0; i < 3; i++) {
                double s = 0;
                for (int r = 0; r < d; r++) s += A[r][i] * om_r[r];
                bl[3 * il + i] += s;
                for (int j = 0; j < 3; j++) {
                    double h = 0;
                    for (int r = 0; r < d; r++) h += A[r][i] * w * A[r][j];
                    Hll[9 * il + 3 * i + j] += h;
                }
            }
            if (ip >= 0) {
                for (int i = 0; i < 6; i++) {
                    double s = 0;
                    for (int r = 0; r < d; r++) s += B[r][i] * om_r[r];
                    bp[6 * ip + i] += s;
                    for (int j = 0; j < 6; j++) {
                        double h = 0;
                        for (int r = 0; r < d; r++) h += B[r][i] * w * B[r][j];
                        Hpp[(size_t)(6 * ip + i) * D + 6 * ip + j] += h;
                    }
                    for (int j = 0; j < 3; j++) {   // Hpl (pose i, point j) = B^T W A
                        double h = 0;
                        for (int r = 0; r < d; r++) h += B[r][i] * w * A[r][j];
                        Hpl[18 * e + 3 * i + j] = h;
                    }
                }
            }
        }
    }

    double lambda_init() const {   // computeLambdaInit (levenberg.cpp:166-180), tau = 1e-5
        const int D = 6 * np;
        double m = 0;
        for (int i = 0; i < D; i++) m = std::max(m, std::fabs(Hpp[(size_t)i * D + i]));
        for (int l = 0; l < nl; l++)
            for (int j = 0; j < 3; j++) m = std::max(m, std::fabs(Hll[9 * l + 4 * j]));
        return 1e-5 * m;
    }

    static bool inv3(const double* m, double* o) {
        const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
        const double det = m[0] * c00 + m[1] * c01 + m[2] * c02;
        if (det == 0) return false;
        const double id = 1.0 / det;
        o[0] = c00 * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
        o[3] = c01 * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
        o[6] = c02 * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
        return true;
    }

    // BlockSolver::solve with lambda on the diagonals (block_solver.hpp:353-486, :563-604)
    bool solve(double lambda) {
        const int D = 6 * np;
        x.assign((size_t)D + 3 * nl, 0);
        std::vector<double> S = Hpp, bs = bp;
        for (int i = 0; i < D; i++) S[(size_t)i * D + i] += lambda;
        std::vector<double> Dinv((size_t)nl * 9), db((size_t)nl * 3);
        // per point: its active edges with a free pose
        std::vector<std::vector<int>> pe(nl);
        for (int e : act_edges) if (hp[ek[e]] >= 0) pe[hl[ep[e]]].push_back(e);
        for (int l = 0; l < nl; l++) {
            double Dm[9];
            for (int i = 0; i < 9; i++) Dm[i] = Hll[9 * l + i];
            Dm[0] += lambda; Dm[4] += lambda; Dm[8] += lambda;
            inv3(Dm, &Dinv[9 * l]);
            for (int i = 0; i < 3; i++) {
                double s = 0;
                for (int j = 0; j < 3; j++) s += Dinv[9 * l + 3 * i + j] * bl[3 * l + j];
                db[3 * l + i] = s;
            }
            for (int e1 : pe[l]) {
                const int i1 = hp[ek[e1]];
                double W[18];   // Hpl * Dinv (6x3)
                for (int r = 0; r < 6; r++)
                    for (int c = 0; c < 3; c++) {
                        double s = 0;
                        for (int k = 0; k < 3; k++) s += Hpl[18 * e1 + 3 * r + k] * Dinv[9 * l + 3 * k + c];
                        W[3 * r + c] = s;
                    }
                for (int r = 0; r < 6; r++) {
                    double s = 0;
                    for (int k = 0; k < 3; k++) s += Hpl[18 * e1 + 3 * r + k] * db[3 * l + k];
                    bs[6 * i1 + r] -= s;
                }
                for (int e2 : pe[l]) {
                    const int i2 = hp[ek[e2]];
                    for (int r = 0; r < 6; r++)
                        for (int c = 0; c < 6; c++) {
                            double s = 0;
                            for (int k = 0; k < 3; k++) s += W[3 * r + k] * Hpl[18 * e2 + 3 * c + k];
                            S[(size_t)(6 * i1 + r) * D + 6 * i2 + c] -= s;
                        }
                }
            }
        }
        // dense LDL^T of the reduced camera system (stands in for SimplicialLDLT)
        std::vector<double> L((size_t)D * D, 0), dd(D, 0);
        for (int j = 0; j < D; j++) {
            double v = S[(size_t)j * D + j];
            for (int k = 0; k < j; k++) v -= L[(size_t)j * D + k] * L[(size_t)j * D + k] * dd[k];
            if (v == 0 || !std::isfinite(v)) return false;
            dd[j] = v;
            L[(size_t)j * D + j] = 1;
            for (int i = j + 1; i < D; i++) {
                double s = S[(size_t)i * D + j];
                for (int k = 0; k < j; k++) s -= L[(size_t)i * D + k] * L[(size_t)j * D + k] * dd[k];
                L[(size_t)i * D + j] = s / v;
            }
        }
        std::vector<double> yv(D);
        for (int i = 0; i < D; i++) {
            double s = bs[i];
            for (int k = 0; k < i; k++) s -= L[(size_t)i * D + k] * yv[k];
            yv[i] = s;
        }
        for (int i = 0; i < D; i++) yv[i] /= dd[i];
        for (int i = D - 1; i >= 0; i--) {
            double s = yv[i];
            for (int k = i + 1; k < D; k++) s -= L[(size_t)k * D + i] * x[k];
            x[i] = s;
        }
        // back-substitution for points: xl = Dinv (bl - Hpl^T xp)
        for (int l = 0; l < nl; l++) {
            double cl[3] = {bl[3 * l], bl[3 * l + 1], bl[3 * l + 2]};
            for (int e : pe[l]) {
                const int ip = hp[ek[e]];
                for (int k = 0; k < 3; k++) {
                    double s = 0;
                    for (int r = 0; r < 6; r++) s += Hpl[18 * e + 3 * r + k] * x[6 * ip + r];
                    cl[k] -= s;
                }
            }
            for (int i = 0; i < 3; i++) {
                double s = 0;
                for (int j = 0; j < 3; j++) s += Dinv[9 * l + 3 * i + j] * cl[j];
                x[(size_t)D + 3 * l + i] = s;
            }
        }
        return true;
    }

    std::vector<SE3> saved_pose;
    std::vector<double> saved_X;
    void push() { saved_pose = pose; saved_X = X; }
    void pop() { pose = saved_pose; X = saved_X; }
    void update() {
        const int D = 6 * np;
        for (int i = 0; i < P; i++) if (hp[i] >= 0) pose[i] = se3_exp_mul(&x[6 * hp[i]], pose[i]);
        for (int l = 0; l < N; l++)
            if (hl[l] >= 0) for (int k = 0; k < 3; k++) X[3 * l + k] += x[(size_t)D + 3 * hl[l] + k];
    }

    // SparseOptimizer::optimize + OptimizationAlgorithmLevenberg::solve
    int optimize(int iters, double& final_chi) {
        double lambda = 0, ni = 2;
        int nbad = 0, done_iters = 0;
        final_chi = 0;
        end_reason = BA_END_NONE;
        oracle_ba_trial* tr = nullptr;
        if (np + nl == 0 || act_edges.empty()) return 0;
        for (int it = 0; it < iters && !terminate(); it++) {
            compute_active_errors();
            double cur = active_robust_chi2();
            const double ini = cur;
            build_system();
            if (it == 0) { lambda = lambda_init(); ni = 2; nbad = 0; }
            double rho = 0;
            int q = 0;
            do {
                tr = trace ? trace->push() : nullptr;
                if (tr) { tr->it = it; tr->q = q; tr->lambda = lambda; tr->cur = cur; }
                push();
                const bool ok = solve(lambda);
                update();
                compute_active_errors();
                double tmp = active_robust_chi2();
                if (!ok) tmp = DBL_MAX;
                rho = cur - tmp;
                double scale = 0;
                const int D = 6 * np;
                for (int j = 0; j < D; j++) scale += x[j] * (lambda * x[j] + bp[j]);
                for (int j = 0; j < 3 * nl; j++) scale += x[(size_t)D + j] * (lambda * x[(size_t)D + j] + bl[j]);
                scale += 1e-3;
                rho /= scale;
                if (tr) { tr->tmp = tmp; tr->scale = scale; tr->rho = rho; tr->accepted = rho > 0 && std::isfinite(tmp); }
                if (rho > 0 && std::isfinite(tmp)) {
                    double alpha = 1. - std::pow((2 * rho - 1), 3);
                    alpha = std::min(alpha, 2. / 3.);
                    lambda *= std::max(1. / 3., alpha);
                    ni = 2;
                    cur = tmp;
                } else {
                    lambda *= ni;
                    ni *= 2;
                    pop();
                }
                q++;
                trials++;
            } while (rho < 0 && q < 10 && !terminate());
            done_iters++;
            final_chi = cur;
            if (tr) { tr->iter_end = 1; tr->ini = ini; tr->cur_end = cur; tr->nbad = nbad; }
            end_reason = BA_END_BUDGET;   // (until something below says otherwise)
            if (q == 10 || rho == 0) { end_reason = q == 10 ? BA_END_Q10 : BA_END_RHO0; break; }
            if ((ini - cur) * 1e3 < ini) nbad++; else nbad = 0;
            if (tr) { tr->nbad_tested = 1; tr->nbad = nbad; }
            if (nbad >= 3) { end_reason = BA_END_NBAD; break; }
        }
        if (end_reason == BA_END_BUDGET && done_iters < iters) end_reason = BA_END_STOP;   // terminate() ended it
        if (end_reason == BA_END_NONE && terminate()) end_reason = BA_END_STOP;
        if (tr) tr->loop_end = end_reason;
        return done_iters;
    }
};

// ---------------------------------------------------------------------------------------------
// FeaturesGrid (src/Frame.cc:32-34 rounding, :71-145) and SearchByProjection (ORBmatcher.cc:315-382)
// ---------------------------------------------------------------------------------------------
struct FeaturesGrid {
    static const int ROWS = 48, COLS = 64;
    float invW = 0, invH = 0, minx = 0, miny = 0;
    int nlevels = 0, n = 0;
    const float* xy = nullptr;
    const int32_t* oct = nullptr;
    std::vector<size_t> grid[COLS][ROWS];

    static int Round(float v) { return static_cast<int>(std::round(v)); }
    static int RoundUp(float v) { return static_cast<int>(std::ceil(v)); }
    static int RoundDn(float v) { return static_cast<int>(std::floor(v)); }

    void assign(const float* kxy, const int32_t* koct, int nk, const float* bounds, int nl) {   // :71-100
        invW = COLS / (bounds[1] - bounds[0]);   // ImageBounds::Width() = maxx - minx (:41-44)
        invH = ROWS / (bounds[3] - bounds[2]);
        minx = bounds[0]; miny = bounds[2];
        xy = kxy; oct = koct; n = nk; nlevels = nl;
        for (int i = 0; i < n; i++) {
            const int cx = Round(invW * (xy[2 * i] - minx));
            const int cy = Round(invH * (xy[2 * i + 1] - miny));
            if (cx < 0 || cx >= COLS || cy < 0 || cy >= ROWS) continue;
            grid[cx][cy].push_back(i);
        }
    }
    std::vector<size_t> in_area(float x, float y, float r, int minLevel, int maxLevel) const {   // :102-145
        std::vector<size_t> indices;
        const int mincx = std::max(RoundDn(invW * (x - r - minx)), 0);
        const int maxcx = std::min(RoundUp(invW * (x + r - minx)), COLS - 1);
        const int mincy = std::max(RoundDn(invH * (y - r - miny)), 0);
        const int maxcy = std::min(RoundUp(invH * (y + r - miny)), ROWS - 1);
        if (mincx >= COLS || maxcx < 0 || mincy >= ROWS || maxcy < 0) return indices;
        const bool checkLevels = (minLevel > 0) || (maxLevel >= 0);
        if (maxLevel < 0) maxLevel = nlevels;
        for (int cx = mincx; cx <= maxcx; cx++)
            for (int cy = mincy; cy <= maxcy; cy++)
                for (size_t idx : grid[cx][cy]) {
                    const int level = oct[idx];
                    if (checkLevels && (level < minLevel || level > maxLevel)) continue;
                    const float distx = xy[2 * idx] - x;
                    const float disty = xy[2 * idx + 1] - y;
                    if (std::fabs(distx) < r && std::fabs(disty) < r) indices.push_back(idx);
                }
        return indices;
    }
};

// ---------------------------------------------------------------------------------------------
// DBoW2 TemplatedVocabulary<FORB> (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h, BowVector.cpp,
// FeatureVector.cpp, FORB.cpp, ScoringObject.h)
// ---------------------------------------------------------------------------------------------
struct Vocabulary {
    struct Node {   // :300-331
        uint32_t id = 0;
        double weight = 0;
        std::vector<uint32_t> children;
        uint32_t parent = 0;
        uint8_t desc[32] = {0};
        uint32_t word_id = 0;
        bool isLeaf() const { return children.empty(); }
    };
    int k = 0, L = 0, scoring = 0, weighting = 0;
    std::vector<Node> nodes;
    std::vector<uint32_t> words;

    // loadFromTextFile (:1341-1431); a blank line (the reference's trailing-newline artefact) is skipped
    bool load_text(const char* path) {
        std::ifstream f(path);
        if (!f.is_open() || f.eof()) return false;
        words.clear();
        nodes.clear();
        std::string s;
        std::getline(f, s);
        std::stringstream ss;
        ss << s;
        int n1 = -1, n2 = -1;
        ss >> k >> L >> n1 >> n2;
        if (k < 0 || k > 20 || L < 1 || L > 10 || n1 < 0 || n1 > 5 || n2 < 0 || n2 > 3) return false;
        scoring = n1;
        weighting = n2;
        nodes.resize(1);
        nodes[0].id = 0;
        while (!f.eof()) {
            std::string snode;
            std::getline(f, snode);
            if (snode.find_first_not_of(" \t\r") == std::string::npos) continue;
            std::stringstream ssnode;
            ssnode << snode;
            const uint32_t nid = (uint32_t)nodes.size();
            nodes.resize(nodes.size() + 1);
            nodes[nid].id = nid;
            int pid = 0;
            ssnode >> pid;
            nodes[nid].parent = (uint32_t)pid;
            nodes[pid].children.push_back(nid);
            int nIsLeaf = 0;
            ssnode >> nIsLeaf;
            for (int i = 0; i < 32; i++) {   // FORB::fromString (FORB.cpp:119-134)
                int n = 0;
                ssnode >> n;
                nodes[nid].desc[i] = (unsigned char)n;
            }
            ssnode >> nodes[nid].weight;
            if (nIsLeaf > 0) {
                nodes[nid].word_id = (uint32_t)words.size();
                words.push_back(nid);
            }
        }
        return true;
    }
    void from_arrays(int k_, int L_, int sc, int wt, int n, const int32_t* parent, const uint8_t* is_leaf,
                     const uint8_t* desc, const double* weight) {
        k = k_; L = L_; scoring = sc; weighting = wt;
        nodes.assign(1, Node());
        words.clear();
        for (int i = 1; i < n; i++) {
            Node nd;
            nd.id = (uint32_t)i;
            nd.parent = (uint32_t)parent[i];
            std::memcpy(nd.desc, desc + 32 * (size_t)i, 32);
            nd.weight = weight[i];
            nodes.push_back(nd);
            nodes[parent[i]].children.push_back((uint32_t)i);
            if (is_leaf[i]) {
                nodes[i].word_id = (uint32_t)words.size();
                words.push_back((uint32_t)i);
            }
        }
    }
    // transform(feature, word_id, weight, nid, levelsup) (:1221-1263); FORB::distance = Hamming
    void transform1(const uint8_t* feature, uint32_t& word_id, double& weight, uint32_t* nid, int levelsup) const {
        const int nid_level = L - levelsup;
        bool nid_set = false;
        if (nid_level <= 0 && nid != nullptr) { *nid = 0; nid_set = true; }
        uint32_t final_id = 0;
        int current_level = 0;
        do {
            ++current_level;
            const std::vector<uint32_t>& ch = nodes[final_id].children;
            final_id = ch[0];
            double best_d = hamming(feature, nodes[final_id].desc);
            for (size_t c = 1; c < ch.size(); c++) {
                const double d = hamming(feature, nodes[ch[c]].desc);
                if (d < best_d) { best_d = d; final_id = ch[c]; }
            }
            if (nid != nullptr && current_level == nid_level) { *nid = final_id; nid_set = true; }
        } while (!nodes[final_id].isLeaf());
        if (nid != nullptr && !nid_set) *nid = final_id;   // undefined in the reference
        word_id = nodes[final_id].word_id;
        weight = nodes[final_id].weight;
    }
    // transform(features, BowVector&, FeatureVector&, levelsup) (:1130-1196)
    void transform(const uint8_t* desc, int n, int levelsup, std::map<uint32_t, double>& v,
                   std::map<uint32_t, std::vector<uint32_t>>& fv) const {
        v.clear();
        fv.clear();
        if (words.empty()) return;
        const bool must = scoring != 5;          // DotProductScoring: false (ScoringObject.h:74-89)
        const bool l2 = scoring == 1;            // L2Scoring: L2, the others L1
        for (int i = 0; i < n; i++) {
            uint32_t id, nid;
            double w;
            transform1(desc + 32 * (size_t)i, id, w, &nid, levelsup);
            if (w > 0) {
                if (weighting == 0 || weighting == 1) {   // TF_IDF, TF: addWeight (BowVector.cpp:34-46)
                    auto it = v.lower_bound(id);
                    if (it != v.end() && !(id < it->first)) it->second += w;
                    else v.insert(it, std::make_pair(id, w));
                } else {                                    // IDF, BINARY: addIfNotExist (:50-58)
                    auto it = v.lower_bound(id);
                    if (it == v.end() || id < it->first) v.insert(it, std::make_pair(id, w));
                }
                fv[nid].push_back((uint32_t)i);             // FeatureVector::addFeature (:31-45)
            }
        }
        if ((weighting == 0 || weighting == 1) && !v.empty() && !must) {
            const double nd = (double)v.size();
            for (auto& e : v) e.second /= nd;
        }
        if (must) {   // BowVector::normalize (:62-84)
            double norm = 0.0;
            if (!l2) for (auto& e : v) norm += std::fabs(e.second);
            else {
                for (auto& e : v) norm += e.second * e.second;
                norm = std::sqrt(norm);
            }
            if (norm > 0.0) for (auto& e : v) e.second /= norm;
        }
    }
};

// ---------------------------------------------------------------------------------------------
// PoseOptimization: one SE3 vertex, unary edges (types_six_dof_expmap.h:143-202,
// types_six_dof_expmap.cpp:266-364), LinearSolverDense under OptimizationAlgorithmLevenberg.
// ---------------------------------------------------------------------------------------------
// oracle_pose_optimization_trace's records (tests/oracle_api.py PO_*_DTYPE have the same layouts).  One per
// LM trial: lambda and cur before the trial, scale with its 1e-3; the iteration-end fields are filled on the
// trial that closes an iteration (iter_end = 1), nbad after the relative-improvement test where the iteration
// reached it (nbad_tested).
struct oracle_po_trial {
    int32_t frame, round, it, q, ok, accepted;
    double cur, tmp, scale, rho, lambda;
    int32_t iter_end, nbad_tested;
    double ini, cur_end;
    int32_t nbad, pad;
};
enum { PO_END_NONE = 0, PO_END_BUDGET, PO_END_Q10, PO_END_RHO0, PO_END_NBAD };
// One per round: the optimize() call, then the classification that follows it.  min_margin is the smallest
// |chi2 - th| / th over the frame's edges (NaN chi2 skipped).
struct oracle_po_round {
    int32_t frame, round, n_active, iterations, reason, n_outliers, n_readmitted, pad;
    double min_margin;
};
// One per frame that ran: the branch ToSE3Quat's Quaterniond(R) took (0: trace > 0, 1 + i: largest diagonal
// i) and whether normalizeRotation flipped the sign (w < 0).
struct oracle_po_frame { int32_t frame, branch, flipped; };

struct POTrace {
    oracle_po_trial* trial = nullptr;
    oracle_po_round* round = nullptr;
    oracle_po_frame* frame = nullptr;
    int trial_cap = 0, round_cap = 0, frame_cap = 0;
    int n_trials = 0, n_rounds = 0, n_frames = 0;   // count past the caps, so the caller sees an overflow
    int f = 0, k = 0;
    oracle_po_trial* push_trial() {
        oracle_po_trial* r = n_trials < trial_cap ? &trial[n_trials] : nullptr;
        n_trials++;
        if (r) { std::memset(r, 0, sizeof *r); r->frame = f; r->round = k; }
        return r;
    }
    oracle_po_round* push_round() {
        oracle_po_round* r = n_rounds < round_cap ? &round[n_rounds] : nullptr;
        n_rounds++;
        if (r) { std::memset(r, 0, sizeof *r); r->frame = f; r->round = k; }
        return r;
    }
    oracle_po_frame* push_frame() {
        oracle_po_frame* r = n_frames < frame_cap ? &frame[n_frames] : nullptr;
        n_frames++;
        if (r) { std::memset(r, 0, sizeof *r); r->frame = f; }
        return r;
    }
};

struct PoseOpt {
    POTrace* trace = nullptr;      // test hook: read-only for the optimisation
    int end_reason = PO_END_NONE;   // why the last optimize() ended
    int E = 0;
    const double *xw = nullptr, *obs = nullptr, *info = nullptr;
    double fx = 0, fy = 0, cx = 0, cy = 0, bf = 0;
    std::vector<uint8_t> stereo, level;
    bool robust = true;
    std::vector<double> err;   // E x 3, the edge's _error as last computed
    SE3 pose;
    std::vector<int> act;

    void compute_error(int e) {   // computeError (types_six_dof_expmap.h:153-158, :184-189)
        double Xc[3];
        se3_map(pose, &xw[3 * e], Xc);
        const double* z = &obs[3 * e];
        if (!stereo[e]) {         // cam_project (.cpp:290-296)
            err[3 * e + 0] = z[0] - (Xc[0] / Xc[2] * fx + cx);
            err[3 * e + 1] = z[1] - (Xc[1] / Xc[2] * fy + cy);
            err[3 * e + 2] = 0;
        } else {                  // (.cpp:299-306): invz narrowed to float, bf stays double
            const float invz = 1.0f / Xc[2];
            const double u = Xc[0] * invz * fx + cx;
            const double v = Xc[1] * invz * fy + cy;
            err[3 * e + 0] = z[0] - u;
            err[3 * e + 1] = z[1] - v;
            err[3 * e + 2] = z[2] - (u - bf * invz);
        }
    }
    double chi2(int e) const {   // BaseEdge::chi2: e . (Omega e), Omega = invSigma2 * I
        double s = 0;
        for (int i = 0; i < (stereo[e] ? 3 : 2); i++) s += err[3 * e + i] * (info[e] * err[3 * e + i]);
        return s;
    }
    void robustify(int e, double c, double& r0, double& r1) const {   // RobustKernelHuber
        if (!robust) { r0 = c; r1 = 1.0; return; }
        const double delta = stereo[e] ? std::sqrt(7.815) : std::sqrt(5.991), dsqr = delta * delta;
        if (c <= dsqr) { r0 = c; r1 = 1.0; }
        else { const double s = std::sqrt(c); r0 = 2 * s * delta - dsqr; r1 = delta / s; }
    }
    double active_robust_chi2() const {
        double s = 0;
        for (int e : act) { double r0, r1; robustify(e, chi2(e), r0, r1); s += r0; }
        return s;
    }
    void compute_active_errors() { for (int e : act) compute_error(e); }

    double H[36], b[6], x[6];
    // linearizeOplus (.cpp:266-288, :335-364) + BaseUnaryEdge::constructQuadraticForm
    void build_system() {
        std::memset(H, 0, sizeof(H));
        std::memset(b, 0, sizeof(b));
        for (int e : act) {
            double Xc[3];
            se3_map(pose, &xw[3 * e], Xc);
            const double X = Xc[0], Y = Xc[1], invz = 1.0 / Xc[2], invz2 = invz * invz;
            double J[3][6] = {{0}};
            J[0][0] = X * Y * invz2 * fx; J[0][1] = -(1 + (X * X * invz2)) * fx; J[0][2] = Y * invz * fx;
            J[0][3] = -invz * fx;         J[0][4] = 0;                            J[0][5] = X * invz2 * fx;
            J[1][0] = (1 + Y * Y * invz2) * fy; J[1][1] = -X * Y * invz2 * fy; J[1][2] = -X * invz * fy;
            J[1][3] = 0;                        J[1][4] = -invz * fy;          J[1][5] = Y * invz2 * fy;
            const int d = stereo[e] ? 3 : 2;
            if (d == 3) {
                J[2][0] = J[0][0] - bf * Y * invz2; J[2][1] = J[0][1] + bf * X * invz2; J[2][2] = J[0][2];
                J[2][3] = J[0][3];                  J[2][4] = 0;                         J[2][5] = J[0][5] - bf * invz2;
            }
            double r0, r1;
            robustify(e, chi2(e), r0, r1);
            const double w = r1 * info[e];
            for (int i = 0; i < 6; i++) {
                double s = 0;
                for (int r = 0; r < d; r++) s += J[r][i] * (info[e] * err[3 * e + r]);
                b[i] -= r1 * s;
                for (int j = 0; j < 6; j++) {
                    double h = 0;
                    for (int r = 0; r < d; r++) h += J[r][i] * w * J[r][j];
                    H[6 * i + j] += h;
                }
            }
        }
    }
    // LinearSolverDense::solve (linear_solver_dense.h:65-113): Eigen LDLT, rejected unless
    // positive (semi)definite.  Unpivoted here; H + lambda*I is SPD whenever it is accepted.
    bool solve(double lambda) {
        double A[36], L[36] = {0}, dd[6];
        std::memcpy(A, H, sizeof(A));
        for (int i = 0; i < 6; i++) A[7 * i] += lambda;
        for (int j = 0; j < 6; j++) {
            double v = A[7 * j];
            for (int k = 0; k < j; k++) v -= L[6 * j + k] * L[6 * j + k] * dd[k];
            if (!(v >= 0) || !std::isfinite(v)) return false;
            dd[j] = v;
            L[7 * j] = 1;
            for (int i = j + 1; i < 6; i++) {
                double s = A[6 * i + j];
                for (int k = 0; k < j; k++) s -= L[6 * i + k] * L[6 * j + k] * dd[k];
                L[6 * i + j] = v != 0 ? s / v : 0;
            }
        }
        double y[6];
        for (int i = 0; i < 6; i++) {
            double s = b[i];
            for (int k = 0; k < i; k++) s -= L[6 * i + k] * y[k];
            y[i] = s;
        }
        for (int i = 0; i < 6; i++) y[i] = dd[i] != 0 ? y[i] / dd[i] : 0;
        for (int i = 5; i >= 0; i--) {
            double s = y[i];
            for (int k = i + 1; k < 6; k++) s -= L[6 * k + i] * x[k];
            x[i] = s;
        }
        return true;
    }
    // SparseOptimizer::optimize (sparse_optimizer.cpp:354-419) around
    // OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:60-163).
    // max_trials is g2o's _maxTrialsAfterFailure (10).
    int optimize(int iters, int max_trials = 10) {
        end_reason = PO_END_NONE;
        if (act.empty()) return -1;   // "0 vertices to optimize"
        double lambda = 0, ni = 2;
        int nbad = 0, done = 0;
        oracle_po_trial* tr = nullptr;
        for (int it = 0; it < iters; it++) {
            compute_active_errors();
            double cur = active_robust_chi2();
            const double ini = cur;
            build_system();
            if (it == 0) {   // computeLambdaInit (:166-180), tau 1e-5
                double m = 0;
                for (int j = 0; j < 6; j++) m = std::max(std::fabs(H[7 * j]), m);   // g2o's argument order: NaN wins
                lambda = 1e-5 * m; ni = 2; nbad = 0;
            }
            double rho = 0;
            int q = 0;
            do {
                tr = trace ? trace->push_trial() : nullptr;
                if (tr) { tr->it = it; tr->q = q; tr->lambda = lambda; tr->cur = cur; }
                const SE3 saved = pose;
                const bool ok = solve(lambda);
                if (!ok) std::memset(x, 0, sizeof(x));   // x left unspecified by a failed solve
                pose = se3_exp_mul(x, pose);             // VertexSE3Expmap::oplusImpl
                compute_active_errors();
                double tmp = active_robust_chi2();
                if (!ok) tmp = DBL_MAX;
                rho = cur - tmp;
                double scale = 1e-3;   // computeScale (:182-190) + 1e-3
                {
                    double s = 0;
                    for (int j = 0; j < 6; j++) s += x[j] * (lambda * x[j] + b[j]);
                    scale += s;
                }
                rho /= scale;
                if (tr) {
                    tr->ok = ok; tr->tmp = tmp; tr->scale = scale; tr->rho = rho;
                    tr->accepted = rho > 0 && std::isfinite(tmp);
                }
                if (rho > 0 && std::isfinite(tmp)) {
                    double alpha = 1. - std::pow((2 * rho - 1), 3);
                    alpha = std::min(alpha, 2. / 3.);
                    lambda *= std::max(1. / 3., alpha);
                    ni = 2;
                    cur = tmp;
                } else {
                    lambda *= ni;
                    ni *= 2;
                    pose = saved;
                }
                q++;
            } while (rho < 0 && q < max_trials);
            done++;
            if (tr) { tr->iter_end = 1; tr->ini = ini; tr->cur_end = cur; tr->nbad = nbad; }
            end_reason = PO_END_BUDGET;   // (until something below says otherwise)
            if (q == max_trials || rho == 0) { end_reason = q == max_trials ? PO_END_Q10 : PO_END_RHO0; break; }
            if ((ini - cur) * 1e3 < ini) nbad++; else nbad = 0;
            if (tr) { tr->nbad_tested = 1; tr->nbad = nbad; }
            if (nbad >= 3) { end_reason = PO_END_NBAD; break; }
        }
        return done;
    }
};

}  // namespace oracle

using namespace oracle;

// =============================================================================================
// C ABI for the tests (ctypes).  Prefix oracle_.
// =============================================================================================
extern "C" {

int oracle_scale_tables(const orbx_params* prm, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                        int32_t* quota, int32_t* umax16) {
    Extractor ex(to_params(prm));
    for (int l = 0; l < prm->nlevels; l++) {
        if (scale) scale[l] = ex.scale[l];
        if (inv_scale) inv_scale[l] = ex.inv_scale[l];
        if (sigma2) sigma2[l] = ex.sigma2[l];
        if (inv_sigma2) inv_sigma2[l] = ex.inv_sigma2[l];
        if (quota) quota[l] = ex.quota[l];
    }
    if (umax16) for (int v = 0; v < 16; v++) umax16[v] = ex.umax[v];
    return 0;
}

void oracle_gaussian_taps(int32_t* taps7) {
    int t[7];
    gaussian_taps_q8(t);
    for (int i = 0; i < 7; i++) taps7[i] = t[i];
}

float oracle_fast_atan2(float y, float x) { return fast_atan2(y, x); }

// OpenCV-build switches (see the header): trig 0 double / 1 float; resize_simd V in {0, 1, 16, 32, 64}.
// Negative values leave a switch unchanged.  Returns the previous values as trig | V << 8.
int oracle_set_compat(int trig, int resize_simd) {
    const int prev = g_trig_float | (g_resize_simd << 8);
    if (trig >= 0) g_trig_float = trig ? 1 : 0;
    if (resize_simd >= 0) g_resize_simd = resize_simd;
    return prev;
}
int oracle_resize_tail_x(int w, int resize_simd) { return resize_tail_x(w, resize_simd); }

// Pyramid: level l written at out + offs[l] (tight rows); dims in w[l], h[l].
int oracle_pyramid(const orbx_params* prm, const uint8_t* img, int rows, int cols, size_t step, uint8_t* out,
                   int64_t* offs, int32_t* w, int32_t* h) {
    Extractor ex(to_params(prm));
    ex.pyramid(view(img, rows, cols, step));
    int64_t o = 0;
    for (int l = 0; l < prm->nlevels; l++) {
        const Img& im = ex.levels[l];
        w[l] = im.cols; h[l] = im.rows; offs[l] = o;
        if (out) for (int y = 0; y < im.rows; y++) std::memcpy(out + o + (int64_t)y * im.cols, im.row(y), im.cols);
        o += (int64_t)im.rows * im.cols;
    }
    return 0;
}

// DetectFAST on one level image (full-image ROI inset 16): xs/ys/resp up to cap, returns count.
int oracle_detect_fast(const uint8_t* img, int rows, int cols, size_t step, int thIni, int thMin, float* xs, float* ys,
                       float* resp, int cap) {
    std::vector<Kp> k;
    Img im = view(img, rows, cols, step);
    if (cols - 32 > 0 && rows - 32 > 0) Extractor::detect_fast(im, 16, 16, cols - 32, rows - 32, thIni, thMin, k);
    const int n = (int)k.size();
    for (int i = 0; i < n && i < cap; i++) { xs[i] = k[i].x; ys[i] = k[i].y; resp[i] = k[i].response; }
    return n;
}

// Literal cv::FAST on a whole image (for score-map unit tests).
int oracle_fast_raw(const uint8_t* img, int rows, int cols, size_t step, int th, float* xs, float* ys, float* resp,
                    int cap) {
    std::vector<RawKp> k;
    fast916(view(img, rows, cols, step), 0, 0, cols, rows, th, k);
    const int n = (int)k.size();
    for (int i = 0; i < n && i < cap; i++) { xs[i] = k[i].x; ys[i] = k[i].y; resp[i] = k[i].response; }
    return n;
}

// QuadTreeSuppression over given keypoints (roi inset 16 of a rows x cols level).
int oracle_quadtree(const float* xs, const float* ys, const float* resp, int n, int rows, int cols, int nfeat,
                    float* oxs, float* oys, float* oresp, int cap) {
    std::vector<Kp> src(n), dst;
    for (int i = 0; i < n; i++) src[i] = {xs[i], ys[i], 7.f, -1.f, resp[i], 0};
    Extractor::quadtree(src, 16, 16, cols - 32, rows - 32, (size_t)nfeat, dst);
    const int m = (int)dst.size();
    for (int i = 0; i < m && i < cap; i++) { oxs[i] = dst[i].x; oys[i] = dst[i].y; oresp[i] = dst[i].response; }
    return m;
}

int oracle_gaussian_blur(const uint8_t* img, int rows, int cols, size_t step, uint8_t* out) {
    Img d;
    gaussian_blur(view(img, rows, cols, step), d);
    std::memcpy(out, d.buf.data(), (size_t)rows * cols);
    return 0;
}

int oracle_extract(const orbx_params* prm, const uint8_t* img, int rows, int cols, size_t step, orbx_keypoint* kps,
                   uint8_t* desc, int cap, int32_t* n, int32_t* per_level) {
    Extractor ex(to_params(prm));
    std::vector<Kp> k;
    std::vector<uint8_t> d;
    const int total = ex.extract(view(img, rows, cols, step), k, d);
    *n = total;
    if (per_level)
        for (int l = 0; l < prm->nlevels; l++) per_level[l] = (int32_t)ex.per_level[l].size();
    if (total > cap) return ORB_ECAP;
    for (int i = 0; i < total; i++) to_abi(k[i], &kps[i]);
    if (total) std::memcpy(desc, d.data(), (size_t)total * 32);
    return 0;
}

// describe alone on planted keypoints: points = n x (level, x, y, score) in level coordinates.  The pyramid,
// IC_Angle on the raw level, one blur per level that has points, the descriptor, and the record as extract()
// writes it (response = the planted score); output level-major, then plant order.  ORB_EINVAL for a point
// outside what DetectFAST can return ([19, w - 19) x [19, h - 19) of its level).
int oracle_describe(const orbx_params* prm, const uint8_t* img, int rows, int cols, size_t step, const int32_t* points,
                    int n, orbx_keypoint* kps, uint8_t* desc) {
    Extractor ex(to_params(prm));
    ex.pyramid(view(img, rows, cols, step));
    for (int i = 0; i < n; i++) {
        const int l = points[4 * i], x = points[4 * i + 1], y = points[4 * i + 2], s = points[4 * i + 3];
        if (l < 0 || l >= prm->nlevels || s < 0 || s > 255) return ORB_EINVAL;
        const Img& im = ex.levels[l];
        if (x < 19 || x >= im.cols - 19 || y < 19 || y >= im.rows - 19) return ORB_EINVAL;
    }
    int o = 0;
    for (int l = 0; l < prm->nlevels; l++) {
        Img blurred;
        for (int i = 0; i < n; i++) {
            if (points[4 * i] != l) continue;
            if (!blurred.rows) gaussian_blur(ex.levels[l], blurred);
            Kp k{(float)points[4 * i + 1], (float)points[4 * i + 2], ex.scale[l] * 31, -1.f, (float)points[4 * i + 3], l};
            k.angle = ex.ic_angle(ex.levels[l], k.x, k.y);
            Extractor::describe(k, blurred, desc + (size_t)o * 32);
            if (l > 0) { k.x *= ex.scale[l]; k.y *= ex.scale[l]; }
            to_abi(k, &kps[o++]);
        }
    }
    return 0;
}

int oracle_descriptor_distance(const uint8_t* a, const uint8_t* b) { return hamming(a, b); }

// Best / second-best scan (ORBmatcher.cc:477-498) + acceptance (:500).
void oracle_bf_match(const uint8_t* A, int nA, const uint8_t* B, int nB, float nnratio, int th_low, int32_t* bidx,
                     int32_t* best, int32_t* second, int32_t* match) {
    for (int i = 0; i < nA; i++) {
        int bd = 256, sd = 256, bi = -1;
        for (int j = 0; j < nB; j++) {
            const int d = hamming(A + 32 * (size_t)i, B + 32 * (size_t)j);
            if (d < bd) { sd = bd; bd = d; bi = j; }
            else if (d < sd) sd = d;
        }
        bidx[i] = bi; best[i] = bd; second[i] = sd;
        if (match) match[i] = (bd <= th_low && bd < nnratio * sd) ? bi : -1;
    }
}

// CheckOrientation (ORBmatcher.cc:249-309), literally: vector<int> bins and std::sort (libstdc++'s
// unstable order decides which of several equal-size bins are kept), on a query-indexed result as
// SearchForInitialization builds it (:670-686): matchIds = (bestIdx2, idx1) in ascending idx1,
// keypoints1 = B, keypoints2 = A, status = matches12 (indexed by idx1).
int oracle_check_orientation(const float* angA, int nA, const float* angB, int32_t* match) {
    const int HISTO_LENGTH = 30;
    std::vector<std::pair<int, int>> matchIds;
    for (int i = 0; i < nA; i++)
        if (match[i] >= 0) matchIds.push_back(std::make_pair(match[i], i));
    const float factor = 1.f / HISTO_LENGTH;
    std::vector<int> hist[HISTO_LENGTH];
    auto diffToBin = [=](float diff) {
        if (diff < 0) diff += 360;
        int bin = cv_round(factor * diff);
        if (bin == HISTO_LENGTH) bin = 0;
        return bin;
    };
    for (const auto& m : matchIds) {
        const int bin = diffToBin(angB[m.first] - angA[m.second]);
        if (bin < 0 || bin >= HISTO_LENGTH) return -1;   // CV_Assert
        hist[bin].push_back(m.second);
    }
    std::sort(std::begin(hist), std::end(hist),
              [](const std::vector<int>& l, const std::vector<int>& r) { return l.size() > r.size(); });
    const size_t max1 = hist[0].size(), max2 = hist[1].size(), max3 = hist[2].size();
    int eraseBin = 3;
    if (max2 < 0.1 * max1) eraseBin = 1;
    else if (max3 < 0.1 * max1) eraseBin = 2;
    int reduction = 0;
    for (int bin = eraseBin; bin < HISTO_LENGTH; bin++)
        for (int i2 : hist[bin]) {
            match[i2] = -1;
            reduction++;
        }
    return (int)matchIds.size() - reduction;
}

// SearchByBoW(KeyFrame*, Frame&, matches) (ORBmatcher.cc:452-516), literally: FeatureVectorIterator
// (:406-450), the greedy `matches[idx2]` skip, best / second-best (:477-498), acceptance (:500) and,
// with check_ori, CheckOrientation(keyframe->keypointsUn, frame.keypointsUn, matchIds, matches)
// (:249-309) with matchIds in push order.  kf->has_mappoint = mappoint valid (non-null, !isBad).
// match[idx2] = idx1 or -1; returns nmatches.
int oracle_search_by_bow(const orbm_tri_frame* kf, const orbm_tri_frame* fr, float nnratio, int check_ori,
                         const float* ang_kf, const float* ang_fr, int32_t* match) {
    const int TH_LOW = 50, HISTO_LENGTH = 30;
    for (int i = 0; i < fr->n; i++) match[i] = -1;
    int nmatches = 0;
    std::vector<std::pair<int, int>> matchIds;
    int a = 0, b = 0;
    while (a < kf->n_nodes && b < fr->n_nodes) {
        if (kf->node_id[a] == fr->node_id[b]) {
            for (int u = kf->node_off[a]; u < kf->node_off[a + 1]; u++) {
                const int idx1 = kf->indices[u];
                if (!kf->has_mappoint[idx1]) continue;
                int bestDist = 256, bestIdx2 = -1, secondBestDist = 256;
                for (int v = fr->node_off[b]; v < fr->node_off[b + 1]; v++) {
                    const int idx2 = fr->indices[v];
                    if (match[idx2] >= 0) continue;
                    const int dist = hamming(kf->desc + 32 * (size_t)idx1, fr->desc + 32 * (size_t)idx2);
                    if (dist < bestDist) {
                        secondBestDist = bestDist;
                        bestDist = dist;
                        bestIdx2 = idx2;
                    } else if (dist < secondBestDist) {
                        secondBestDist = dist;
                    }
                }
                if (bestDist <= TH_LOW && bestDist < nnratio * secondBestDist) {
                    match[bestIdx2] = idx1;
                    nmatches++;
                    if (check_ori) matchIds.push_back(std::make_pair(idx1, bestIdx2));
                }
            }
            a++; b++;
        } else if (kf->node_id[a] < fr->node_id[b]) a++;
        else b++;
    }
    if (!check_ori) return nmatches;
    const float factor = 1.f / HISTO_LENGTH;
    std::vector<int> hist[HISTO_LENGTH];
    for (const auto& m : matchIds) {
        float diff = ang_kf[m.first] - ang_fr[m.second];
        if (diff < 0) diff += 360;
        int bin = cv_round(factor * diff);
        if (bin == HISTO_LENGTH) bin = 0;
        if (bin < 0 || bin >= HISTO_LENGTH) return -1;   // CV_Assert
        hist[bin].push_back(m.second);
    }
    std::sort(std::begin(hist), std::end(hist),
              [](const std::vector<int>& l, const std::vector<int>& r) { return l.size() > r.size(); });
    const size_t max1 = hist[0].size(), max2 = hist[1].size(), max3 = hist[2].size();
    int eraseBin = 3;
    if (max2 < 0.1 * max1) eraseBin = 1;
    else if (max3 < 0.1 * max1) eraseBin = 2;
    int reduction = 0;
    for (int bin = eraseBin; bin < HISTO_LENGTH; bin++)
        for (int i2 : hist[bin]) {
            match[i2] = -1;
            reduction++;
        }
    return (int)matchIds.size() - reduction;
}

// SearchByBoW(KeyFrame* keyframe1, KeyFrame* keyframe2, matches12) (ORBmatcher.cc:696-766), literally:
// candidates need an unclaimed idx2 with a valid MapPoint (:733), bestDist < TH_LOW (:750), matches12 by
// idx1, CheckOrientation(keypoints2, keypoints1, matchIds = (bestIdx2, idx1), matches12) (:762-763).
// kf1/kf2->has_mappoint = MapPoint valid.  match12[idx1] = idx2 or -1; returns nmatches.
int oracle_search_by_bow_kf(const orbm_tri_frame* kf1, const orbm_tri_frame* kf2, float nnratio, int check_ori,
                            const float* ang1, const float* ang2, int32_t* match12) {
    const int TH_LOW = 50, HISTO_LENGTH = 30;
    for (int i = 0; i < kf1->n; i++) match12[i] = -1;
    std::vector<char> matched2(kf2->n, 0);
    int nmatches = 0;
    std::vector<std::pair<int, int>> matchIds;
    int a = 0, b = 0;
    while (a < kf1->n_nodes && b < kf2->n_nodes) {
        if (kf1->node_id[a] == kf2->node_id[b]) {
            for (int u = kf1->node_off[a]; u < kf1->node_off[a + 1]; u++) {
                const int idx1 = kf1->indices[u];
                if (!kf1->has_mappoint[idx1]) continue;
                int bestDist = 256, bestIdx2 = -1, secondBestDist = 256;
                for (int v = kf2->node_off[b]; v < kf2->node_off[b + 1]; v++) {
                    const int idx2 = kf2->indices[v];
                    if (matched2[idx2] || !kf2->has_mappoint[idx2]) continue;
                    const int dist = hamming(kf1->desc + 32 * (size_t)idx1, kf2->desc + 32 * (size_t)idx2);
                    if (dist < bestDist) {
                        secondBestDist = bestDist;
                        bestDist = dist;
                        bestIdx2 = idx2;
                    } else if (dist < secondBestDist) {
                        secondBestDist = dist;
                    }
                }
                if (bestDist < TH_LOW && bestDist < nnratio * secondBestDist) {
                    match12[idx1] = bestIdx2;
                    matched2[bestIdx2] = 1;
                    nmatches++;
                    if (check_ori) matchIds.push_back(std::make_pair(bestIdx2, idx1));
                }
            }
            a++; b++;
        } else if (kf1->node_id[a] < kf2->node_id[b]) a++;
        else b++;
    }
    if (!check_ori) return nmatches;
    const float factor = 1.f / HISTO_LENGTH;
    std::vector<int> hist[HISTO_LENGTH];
    for (const auto& m : matchIds) {   // keypoint1 = keypoints2[bestIdx2], keypoint2 = keypoints1[idx1]
        float diff = ang2[m.first] - ang1[m.second];
        if (diff < 0) diff += 360;
        int bin = cv_round(factor * diff);
        if (bin == HISTO_LENGTH) bin = 0;
        if (bin < 0 || bin >= HISTO_LENGTH) return -1;
        hist[bin].push_back(m.second);
    }
    std::sort(std::begin(hist), std::end(hist),
              [](const std::vector<int>& l, const std::vector<int>& r) { return l.size() > r.size(); });
    const size_t max1 = hist[0].size(), max2 = hist[1].size(), max3 = hist[2].size();
    int eraseBin = 3;
    if (max2 < 0.1 * max1) eraseBin = 1;
    else if (max3 < 0.1 * max1) eraseBin = 2;
    int reduction = 0;
    for (int bin = eraseBin; bin < HISTO_LENGTH; bin++)
        for (int i1 : hist[bin]) {
            match12[i1] = -1;
            reduction++;
        }
    return (int)matchIds.size() - reduction;
}

// SearchForTriangulation (ORBmatcher.cc:768-866), checkOrientation = false.
int oracle_search_for_triangulation(const orbm_tri_frame* f1, const orbm_tri_frame* f2, const float* F12,
                                    const float* ep2, const float* scale2, const float* sigma2, int only_stereo,
                                    int32_t* match12) {
    const int TH_LOW = 50;
    for (int i = 0; i < f1->n; i++) match12[i] = -1;
    int nm = 0;
    int a = 0, b = 0;
    while (a < f1->n_nodes && b < f2->n_nodes) {   // FeatureVectorIterator (:406-450)
        if (f1->node_id[a] == f2->node_id[b]) {
            for (int u = f1->node_off[a]; u < f1->node_off[a + 1]; u++) {
                const int i1 = f1->indices[u];
                if (f1->has_mappoint[i1]) continue;
                const bool st1 = f1->uright[i1] >= 0;
                if (only_stereo && !st1) continue;
                int bd = TH_LOW, bi = -1;
                for (int v = f2->node_off[b]; v < f2->node_off[b + 1]; v++) {
                    const int i2 = f2->indices[v];
                    if (f2->has_mappoint[i2]) continue;
                    const bool st2 = f2->uright[i2] >= 0;
                    if (only_stereo && !st2) continue;
                    const int d = hamming(f1->desc + 32 * (size_t)i1, f2->desc + 32 * (size_t)i2);
                    if (d > TH_LOW || d > bd) continue;
                    const float x2 = f2->kp_xy[2 * i2], y2 = f2->kp_xy[2 * i2 + 1];
                    const int o2 = f2->octave[i2];
                    if (!st1 && !st2) {
                        const float dx = ep2[0] - x2, dy = ep2[1] - y2;
                        if (dx * dx + dy * dy < 100 * scale2[o2]) continue;
                    }
                    if (epipolar_ok(f1->kp_xy[2 * i1], f1->kp_xy[2 * i1 + 1], x2, y2, F12, sigma2[o2])) {
                        bi = i2; bd = d;
                    }
                }
                if (bi >= 0) { match12[i1] = bi; nm++; }
            }
            a++; b++;
        } else if (f1->node_id[a] < f2->node_id[b]) a++;
        else b++;
    }
    return nm;
}

// Optimizer::LocalBundleAdjustment from the vertex/edge setup on (Optimizer.cc:540-735).
// ComputeStereoMatches (src/ORBmatcher.cc:72-247) with PatchDistance (:60-68).  Rounding helpers as
// the reference's Round / RoundUp / RoundDn (:50-52): std::round (half away from zero), ceil, floor.
// The empty-match case reads distIndices[0] in the reference (undefined); here it leaves all
// results as computed.
int oracle_compute_stereo_matches(const orbm_stereo_view* L, const orbm_stereo_view* R, const float* scaleFactors,
                                  const float* invScaleFactors, float bf, float baseline, float* uright,
                                  float* depth) {
    const int TH_HIGH = 100, TH_LOW = 50, PR = 5, PS = 11, SR = 5;
    const int nL = L->n, nR = R->n;
    for (int i = 0; i < nL; i++) { uright[i] = -1.f; depth[i] = -1.f; }
    auto px = [](const orbm_stereo_view* v, int lvl, int y, int x) -> int {
        return v->level[lvl][(size_t)y * v->level_step[lvl] + x];
    };
    // row table (:86-100): right keypoint indices per image row, ascending
    const int nrows = L->level_rows[0];
    std::vector<std::vector<int>> rowIndices(nrows);
    for (int iR = 0; iR < nR; iR++) {
        const orbx_keypoint& k = R->kps[iR];
        const float r = 2.f * scaleFactors[k.octave];
        const int miny = (int)std::floor(k.y - r), maxy = (int)std::ceil(k.y + r);
        for (int y = miny; y <= maxy; y++)
            if (y >= 0 && y < nrows) rowIndices[y].push_back(iR);
    }
    const float minZ = baseline, mind = 0, maxd = bf / minZ;
    const int TH_ORB_DIST = (TH_HIGH + TH_LOW) / 2;
    const float eps = 0.01f;
    std::vector<std::pair<int, int>> distIndices;
    int distances[2 * SR + 1];
    for (int iL = 0; iL < nL; iL++) {
        const orbx_keypoint& kL = L->kps[iL];
        const int octaveL = kL.octave;
        const float vL = kL.y, uL = kL.x;
        const int row = (int)vL;
        if (row < 0 || row >= nrows) continue;
        const std::vector<int>& cand = rowIndices[row];
        if (cand.empty()) continue;
        const float minu = uL - maxd, maxu = uL - mind;
        if (maxu < 0) continue;
        int bestHam = TH_HIGH, bestIdxR = 0;
        for (int iR : cand) {
            const orbx_keypoint& kR = R->kps[iR];
            if (kR.octave < octaveL - 1 || kR.octave > octaveL + 1) continue;
            const float uR = kR.x;
            if (uR >= minu && uR <= maxu) {
                const int d = hamming(L->desc + 32 * (size_t)iL, R->desc + 32 * (size_t)iR);
                if (d < bestHam) { bestHam = d; bestIdxR = iR; }
            }
        }
        if (!(bestHam < TH_ORB_DIST)) continue;
        // sub-pixel correlation on the left octave's level (:170-236)
        const float sf = invScaleFactors[octaveL];
        const int suL = (int)std::round(sf * kL.x);
        const int svL = (int)std::round(sf * kL.y);
        const int suR = (int)std::round(sf * R->kps[bestIdxR].x);
        const int colsR = R->level_cols[octaveL];
        if (suR + SR - PR < 0 || suR + SR + PR + 1 >= colsR) continue;
        int bestSad = INT32_MAX, bestdx = 0;
        for (int dx = -SR; dx <= SR; dx++) {
            const int sub = px(L, octaveL, svL, suL) - px(R, octaveL, svL, suR + dx);
            int sum = 0;
            for (int y = 0; y < PS; y++)
                for (int x = 0; x < PS; x++)
                    sum += std::abs(px(L, octaveL, svL - PR + y, suL - PR + x) -
                                    px(R, octaveL, svL - PR + y, suR + dx - PR + x) - sub);
            if (sum < bestSad) { bestSad = sum; bestdx = dx; }
            distances[SR + dx] = sum;
        }
        if (bestdx == -SR || bestdx == SR) continue;
        const int d1 = distances[SR + bestdx - 1], d2 = distances[SR + bestdx], d3 = distances[SR + bestdx + 1];
        const float deltaR = (d1 - d3) / (2.f * (d1 + d3 - 2.f * d2));
        if (deltaR < -1 || deltaR > 1) continue;
        float bestuR = scaleFactors[octaveL] * (suR + bestdx + deltaR);
        float disparity = uL - bestuR;
        if (disparity >= mind && disparity < maxd) {
            if (disparity <= 0) { disparity = eps; bestuR = uL - eps; }
            depth[iL] = bf / disparity;
            uright[iL] = bestuR;
            distIndices.push_back(std::make_pair(bestSad, iL));
        }
    }
    if (distIndices.empty()) return 0;
    std::sort(distIndices.begin(), distIndices.end(), std::greater<std::pair<int, int>>());
    const int m = std::max((int)distIndices.size() / 2 - 1, 0);
    const int median = distIndices[m].first;
    const float thDist = 1.5f * 1.4f * median;
    int n = 0;
    for (const auto& v : distIndices) {
        if (v.first < thDist) break;
        uright[v.second] = -1;
        depth[v.second] = -1;
    }
    for (int i = 0; i < nL; i++) n += uright[i] >= 0;
    return n;
}

// stop_after >= 0: the stop flag is raised right after that many LM trials (between trials, where
// g2o polls terminate(): optimization_algorithm_levenberg.cpp:149, sparse_optimizer.cpp:376).
// trace / end_reason (either may be null): the per-trial records and why each optimize() ended.
static int local_ba_run(const orbba_problem* pr, orbba_result* res, const volatile int32_t* stop, int stop_after,
                        BATrace* trace, int32_t* end_reason) {
    BA ba;
    ba.stop_after = stop_after;
    ba.trace = trace;
    if (end_reason) end_reason[0] = end_reason[1] = BA_END_NONE;
    ba.P = pr->n_poses; ba.N = pr->n_points; ba.E = pr->n_edges;
    ba.stop = stop;
    ba.pose.resize(ba.P);
    ba.fixed.assign(pr->pose_fixed, pr->pose_fixed + ba.P);
    for (int i = 0; i < ba.P; i++) {   // ToSE3Quat: SE3Quat(R, t) -> Quaterniond(R), normalize
        ba.pose[i].q = quat_from_R(pr->pose_R + 9 * i);
        quat_normalize_pos(ba.pose[i].q);
        for (int k = 0; k < 3; k++) ba.pose[i].t[k] = pr->pose_t[3 * i + k];
    }
    ba.X.assign(pr->points, pr->points + 3 * (size_t)ba.N);
    ba.ep.assign(pr->edge_point, pr->edge_point + ba.E);
    ba.ek.assign(pr->edge_pose, pr->edge_pose + ba.E);
    ba.obs.assign(pr->edge_obs, pr->edge_obs + 3 * (size_t)ba.E);
    ba.info.assign(pr->edge_inv_sigma2, pr->edge_inv_sigma2 + ba.E);
    ba.cam.assign(pr->edge_cam, pr->edge_cam + 5 * (size_t)ba.E);
    ba.stereo.resize(ba.E);
    for (int e = 0; e < ba.E; e++) ba.stereo[e] = ba.obs[3 * e + 2] < 0 ? 0 : 1;
    ba.level.assign(ba.E, 0);
    ba.robust.assign(ba.E, 1);
    ba.err.assign(3 * (size_t)ba.E, 0);
    res->iterations[0] = res->iterations[1] = 0;
    res->chi2[0] = res->chi2[1] = 0;
    bool run = !ba.terminate();
    if (run) {
        ba.init_level(0);
        res->iterations[0] = ba.optimize(5, res->chi2[0]);
        if (end_reason) end_reason[0] = ba.end_reason;
        bool more = !ba.terminate();
        if (more) {
            for (int e = 0; e < ba.E; e++) {
                const double maxc = ba.stereo[e] ? 7.815 : 5.991;
                if (ba.chi2(e) > maxc || !ba.depth_positive(e)) ba.level[e] = 1;
                ba.robust[e] = 0;
            }
            ba.init_level(0);
            if (trace) trace->loop = 1;
            res->iterations[1] = ba.optimize(10, res->chi2[1]);
            if (end_reason) end_reason[1] = ba.end_reason;
        }
    }
    for (int e = 0; e < ba.E; e++) {
        const double maxc = ba.stereo[e] ? 7.815 : 5.991;
        const double c = ba.chi2(e);
        res->edge_outlier[e] = run ? (uint8_t)(c > maxc || !ba.depth_positive(e)) : 0;
        if (res->edge_chi2) res->edge_chi2[e] = c;
    }
    for (int i = 0; i < ba.P; i++) {
        quat_to_R(ba.pose[i].q, res->pose_R + 9 * i);
        for (int k = 0; k < 3; k++) res->pose_t[3 * i + k] = ba.pose[i].t[k];
        if (res->pose_q) {
            res->pose_q[4 * i] = ba.pose[i].q.x; res->pose_q[4 * i + 1] = ba.pose[i].q.y;
            res->pose_q[4 * i + 2] = ba.pose[i].q.z; res->pose_q[4 * i + 3] = ba.pose[i].q.w;
        }
    }
    std::memcpy(res->points, ba.X.data(), sizeof(double) * 3 * ba.N);
    return 0;
}

int oracle_local_ba_stop_after(const orbba_problem* pr, orbba_result* res, const volatile int32_t* stop,
                               int stop_after) {
    return local_ba_run(pr, res, stop, stop_after, nullptr, nullptr);
}

// The same run with a record per LM trial written to trace[0 .. cap) and why each optimize() ended in
// end_reason[2] (BA_END_*).  Returns the number of trials (more than cap: the array was too short).
int oracle_local_ba_trace(const orbba_problem* pr, orbba_result* res, const volatile int32_t* stop, int stop_after,
                          oracle_ba_trial* trace, int cap, int32_t* end_reason) {
    BATrace t;
    t.rec = trace;
    t.cap = cap;
    local_ba_run(pr, res, stop, stop_after, &t, end_reason);
    return t.n;
}

int oracle_local_ba(const orbba_problem* pr, orbba_result* res, const volatile int32_t* stop) {
    return oracle_local_ba_stop_after(pr, res, stop, -1);
}

void* oracle_voc_load_text(const char* path) {
    std::unique_ptr<Vocabulary> v(new Vocabulary);
    if (!v->load_text(path)) return nullptr;
    return v.release();
}
void* oracle_voc_create(int k, int L, int scoring, int weighting, int n, const int32_t* parent, const uint8_t* is_leaf,
                        const uint8_t* desc, const double* weight) {
    Vocabulary* v = new Vocabulary;
    v->from_arrays(k, L, scoring, weighting, n, parent, is_leaf, desc, weight);
    return v;
}
void oracle_voc_destroy(void* h) { delete static_cast<Vocabulary*>(h); }
int oracle_voc_info(void* h, int32_t* out6) {
    const Vocabulary* v = static_cast<Vocabulary*>(h);
    out6[0] = v->k; out6[1] = v->L; out6[2] = (int32_t)v->nodes.size(); out6[3] = (int32_t)v->words.size();
    out6[4] = v->scoring; out6[5] = v->weighting;
    return 0;
}
// Per-feature word id / weight / node id (transform(feature, id, w, &nid, levelsup)).
void oracle_voc_words(void* h, const uint8_t* desc, int n, int levelsup, uint32_t* word, double* weight, uint32_t* nid) {
    const Vocabulary* v = static_cast<Vocabulary*>(h);
    for (int i = 0; i < n; i++) v->transform1(desc + 32 * (size_t)i, word[i], weight[i], &nid[i], levelsup);
}
int oracle_voc_transform(void* h, const uint8_t* desc, int n, int levelsup, uint32_t* bow_word, double* bow_weight,
                         int32_t* n_words, uint32_t* fv_node, int32_t* fv_off, int32_t* fv_idx, int32_t* n_nodes) {
    const Vocabulary* v = static_cast<Vocabulary*>(h);
    std::map<uint32_t, double> bv;
    std::map<uint32_t, std::vector<uint32_t>> fv;
    v->transform(desc, n, levelsup, bv, fv);
    int t = 0;
    for (auto& e : bv) { bow_word[t] = e.first; bow_weight[t] = e.second; t++; }
    *n_words = t;
    t = 0;
    int o = 0;
    for (auto& e : fv) {
        fv_node[t] = e.first;
        fv_off[t] = o;
        for (uint32_t i : e.second) fv_idx[o++] = (int32_t)i;
        t++;
    }
    fv_off[t] = o;
    *n_nodes = t;
    return 0;
}

// FeaturesGrid::AssignFeatures as CSR: cell c = cx * 48 + cy owns idx[cell_start[c] .. cell_start[c+1]).
int oracle_features_grid(const float* xy, const int32_t* octave, int n, const float* bounds, int32_t* cell_start,
                         int32_t* idx) {
    std::unique_ptr<FeaturesGrid> g(new FeaturesGrid);
    g->assign(xy, octave, n, bounds, 8);
    int k = 0;
    for (int cx = 0; cx < FeaturesGrid::COLS; cx++)
        for (int cy = 0; cy < FeaturesGrid::ROWS; cy++) {
            cell_start[cx * FeaturesGrid::ROWS + cy] = k;
            for (size_t i : g->grid[cx][cy]) idx[k++] = (int32_t)i;
        }
    cell_start[FeaturesGrid::COLS * FeaturesGrid::ROWS] = k;
    return k;
}

// FeaturesGrid::GetFeaturesInArea for one query; returns the count (out: up to cap indices, in order).
int oracle_features_in_area(const float* xy, const int32_t* octave, int n, const float* bounds, int nlevels,
                            float x, float y, float r, int minLevel, int maxLevel, int32_t* out, int cap) {
    std::unique_ptr<FeaturesGrid> g(new FeaturesGrid);
    g->assign(xy, octave, n, bounds, nlevels);
    const std::vector<size_t> v = g->in_area(x, y, r, minLevel, maxLevel);
    for (size_t i = 0; i < v.size() && (int)i < cap; i++) out[i] = (int32_t)v[i];
    return (int)v.size();
}

// ORBmatcher::SearchByProjection(Frame&, const std::vector<MapPoint*>&, float th) (:315-382) per frame.
// frame.mappoints is modelled by `owner` (claimed keypoints, :339) and kp_match (assignments).
int oracle_search_by_projection(const orbm_proj_batch* b, int32_t* kp_match, int32_t* n_matches) {
    const int TH_HIGH = 100;
    for (int f = 0; f < b->n_frames; f++) {
        const int k0 = b->kp_begin[f], nk = b->kp_begin[f + 1] - k0;
        const int m0 = b->mp_begin[f], nm = b->mp_begin[f + 1] - m0;
        std::unique_ptr<FeaturesGrid> g(new FeaturesGrid);
        g->assign(b->kp_xy + 2 * (size_t)k0, b->kp_octave + k0, nk, b->bounds + 4 * (size_t)f, b->n_levels);
        // keypoint "has a map point with Observations() > 0"
        std::vector<uint8_t> claimed(nk, 0);
        if (b->kp_claimed) for (int i = 0; i < nk; i++) claimed[i] = b->kp_claimed[k0 + i];
        for (int i = 0; i < nk; i++) kp_match[k0 + i] = -1;
        int nmatches = 0;
        for (int j = 0; j < nm; j++) {
            const int mj = m0 + j;
            if (!b->mp_valid[mj]) continue;
            const int predictedScale = b->mp_level[mj];
            const float viewCos = b->mp_view_cos[mj];
            const float r = viewCos > 0.998 ? 2.5f : 4.f;   // RadiusByViewingCos (:53)
            const float radius = b->th * r * b->scale_factors[predictedScale];
            const float u = b->mp_proj[3 * (size_t)mj], v = b->mp_proj[3 * (size_t)mj + 1];
            const float uR = b->mp_proj[3 * (size_t)mj + 2];
            const std::vector<size_t> indices = g->in_area(u, v, radius, predictedScale - 1, predictedScale);
            if (indices.empty()) continue;
            const uint8_t* desc1 = b->mp_desc + 32 * (size_t)mj;
            int bestDist = 256, bestLevel = -1, secondbestDist = 256, secondBestLevel = -1, bestIdx = -1;
            for (size_t idx : indices) {
                if (claimed[idx]) continue;
                const float ur = b->kp_uright[k0 + idx];
                if (ur > 0 && std::fabs(uR - ur) > radius) continue;
                const int dist = hamming(desc1, b->kp_desc + 32 * (size_t)(k0 + idx));
                if (dist < bestDist) {
                    secondbestDist = bestDist;
                    bestDist = dist;
                    secondBestLevel = bestLevel;
                    bestLevel = b->kp_octave[k0 + idx];
                    bestIdx = (int)idx;
                } else if (dist < secondbestDist) {
                    secondBestLevel = b->kp_octave[k0 + idx];
                    secondbestDist = dist;
                }
            }
            if (bestDist <= TH_HIGH) {
                if (bestLevel == secondBestLevel && bestDist > b->nnratio * secondbestDist) continue;
                kp_match[k0 + bestIdx] = j;
                if (b->mp_has_obs[mj]) claimed[bestIdx] = 1;
                nmatches++;
            }
        }
        n_matches[f] = nmatches;
    }
    return 0;
}

// SearchByProjection(Frame& currFrame, const Frame& lastFrame, th, monocular) (ORBmatcher.cc:1279-1362),
// literally, frame by frame: the caller's projection / validity (:1295-1311) in mp_valid / mp_proj.
int oracle_search_by_projection_motion(const orbm_motion_batch* b, int32_t* kp_match, int32_t* n_matches) {
    const int TH_HIGH = 100, HISTO_LENGTH = 30;
    for (int f = 0; f < b->n_frames; f++) {
        const int k0 = b->kp_begin[f], nk = b->kp_begin[f + 1] - k0;
        const int m0 = b->mp_begin[f], nm = b->mp_begin[f + 1] - m0;
        std::unique_ptr<FeaturesGrid> g(new FeaturesGrid);
        g->assign(b->kp_xy + 2 * (size_t)k0, b->kp_octave + k0, nk, b->bounds + 4 * (size_t)f, b->n_levels);
        // currFrame.mappoints[i]: -1 none, else the owner's has-observations flag decides the skip
        std::vector<int> owner(nk, -1);
        std::vector<uint8_t> claimed(nk, 0);
        if (b->kp_claimed) for (int i = 0; i < nk; i++) claimed[i] = b->kp_claimed[k0 + i];
        const int mot = b->motion ? b->motion[f] : 0;
        const bool forward = mot == 1, backward = mot == 2;
        std::vector<std::pair<int, int>> matchIds;
        int nmatches = 0;
        for (int idx1 = 0; idx1 < nm; idx1++) {
            const int mj = m0 + idx1;
            if (!b->mp_valid[mj]) continue;
            const float u = b->mp_proj[3 * (size_t)mj], v = b->mp_proj[3 * (size_t)mj + 1];
            const float ur = b->mp_proj[3 * (size_t)mj + 2];
            const int octave1 = b->mp_octave[mj];
            const float radius = b->th * b->scale_factors[octave1];
            const int minLevel = forward ? octave1 : (backward ? 0 : octave1 - 1);
            const int maxLevel = forward ? -1 : (backward ? octave1 : octave1 + 1);
            const std::vector<size_t> indices2 = g->in_area(u, v, radius, minLevel, maxLevel);
            if (indices2.empty()) continue;
            const uint8_t* desc1 = b->mp_desc + 32 * (size_t)mj;
            int bestDist = 256, bestIdx2 = -1;
            for (size_t idx2 : indices2) {
                if (claimed[idx2]) continue;
                const float u2 = b->kp_uright[k0 + idx2];
                if (u2 > 0 && std::fabs(ur - u2) > radius) continue;
                const int dist = hamming(desc1, b->kp_desc + 32 * (size_t)(k0 + idx2));
                if (dist < bestDist) {
                    bestDist = dist;
                    bestIdx2 = (int)idx2;
                }
            }
            if (bestDist <= TH_HIGH) {
                owner[bestIdx2] = idx1;
                claimed[bestIdx2] = b->mp_has_obs[mj] ? 1 : 0;
                nmatches++;
                if (b->check_orientation) matchIds.push_back(std::make_pair(idx1, bestIdx2));
            }
        }
        if (b->check_orientation) {
            const float factor = 1.f / HISTO_LENGTH;
            std::vector<int> hist[HISTO_LENGTH];
            for (const auto& m : matchIds) {
                float diff = b->mp_angle[m0 + m.first] - b->kp_angle[k0 + m.second];
                if (diff < 0) diff += 360;
                int bin = cv_round(factor * diff);
                if (bin == HISTO_LENGTH) bin = 0;
                if (bin < 0 || bin >= HISTO_LENGTH) return -1;
                hist[bin].push_back(m.second);
            }
            std::sort(std::begin(hist), std::end(hist),
                      [](const std::vector<int>& l, const std::vector<int>& r) { return l.size() > r.size(); });
            const size_t max1 = hist[0].size(), max2 = hist[1].size(), max3 = hist[2].size();
            int eraseBin = 3;
            if (max2 < 0.1 * max1) eraseBin = 1;
            else if (max3 < 0.1 * max1) eraseBin = 2;
            int reduction = 0;
            for (int bin = eraseBin; bin < HISTO_LENGTH; bin++)
                for (int i2 : hist[bin]) {
                    owner[i2] = -1;
                    reduction++;
                }
            nmatches = (int)matchIds.size() - reduction;
        }
        for (int i = 0; i < nk; i++) kp_match[k0 + i] = owner[i];
        n_matches[f] = nmatches;
    }
    return 0;
}

// ORBmatcher::SearchByProjection(Frame& frame, KeyFrame* keyframe, alreadyFound, th, ORBdist)
// (ORBmatcher.cc:1364-1445), literally, frame by frame: CameraProjection::WorldToImage
// (CameraProjection.h:44-60, cv::Matx float products s = 0; s += a(i,k) * b(k)), ImageBounds::Contains
// (Frame.cc:51-54), Ow = CameraPose::Invt() (CameraPose.h:45), dist3D = (float)cv::norm(PO) (double sum
// of squares), Get{Min,Max}DistanceInvariance (MapPoint.cc:382-392), PredictScale (MapPoint.cc:405-415)
// with log taken as ::log(double) (the float overload is not in scope there, as for cos / sin in
// ComputeOrbDescriptor), the window over predictedScale +- 1, the skip of every keypoint holding a map
// point, bestDist <= ORBdist, then CheckOrientation(keyframe->keypointsUn, frame.keypointsUn, ...).
int oracle_search_by_projection_reloc(const orbm_reloc_batch* b, int32_t* kp_match, int32_t* n_matches) {
    const int HISTO_LENGTH = 30;
    for (int f = 0; f < b->n_frames; f++) {
        const int k0 = b->kp_begin[f], nk = b->kp_begin[f + 1] - k0;
        const int m0 = b->mp_begin[f], nm = b->mp_begin[f + 1] - m0;
        std::unique_ptr<FeaturesGrid> g(new FeaturesGrid);
        g->assign(b->kp_xy + 2 * (size_t)k0, b->kp_octave + k0, nk, b->bounds + 4 * (size_t)f, b->n_levels);
        std::vector<uint8_t> holds(nk, 0);   // frame.mappoints[i] != NULL
        if (b->kp_claimed) for (int i = 0; i < nk; i++) holds[i] = b->kp_claimed[k0 + i];
        std::vector<int> owner(nk, -1);
        const float* R = b->pose + 12 * (size_t)f;
        const float* t = R + 9;
        const float* K = b->camera + 4 * (size_t)f;
        const float* bd = b->bounds + 4 * (size_t)f;
        float Ow[3];
        for (int i = 0; i < 3; i++) {   // -R^T * t: (-R^T)(i, k) = -R(k, i)
            float sacc = 0;
            for (int k = 0; k < 3; k++) sacc += (-R[3 * k + i]) * t[k];
            Ow[i] = sacc;
        }
        int nmatches = 0;
        std::vector<std::pair<int, int>> matchIds;
        for (int idx1 = 0; idx1 < nm; idx1++) {
            const int mj = m0 + idx1;
            if (!b->mp_valid[mj]) continue;
            const float* Xw = b->mp_xw + 3 * (size_t)mj;
            float Xc[3];
            for (int i = 0; i < 3; i++) {
                float sacc = 0;
                for (int k = 0; k < 3; k++) sacc += R[3 * i + k] * Xw[k];
                Xc[i] = sacc + t[i];
            }
            const float invZ = 1.f / Xc[2];
            const float u = invZ * K[0] * Xc[0] + K[2];
            const float v = invZ * K[1] * Xc[1] + K[3];
            if (!(u >= bd[0] && u < bd[1] && v >= bd[2] && v < bd[3])) continue;
            double sq = 0;
            for (int i = 0; i < 3; i++) {
                const double d = (double)(Xw[i] - Ow[i]);
                sq += d * d;
            }
            const float dist3D = static_cast<float>(std::sqrt(sq));
            const float maxDistance = 1.2f * b->mp_max_min[2 * (size_t)mj];
            const float minDistance = 0.8f * b->mp_max_min[2 * (size_t)mj + 1];
            if (dist3D < minDistance || dist3D > maxDistance) continue;
            const float ratio = b->mp_max_min[2 * (size_t)mj] / dist3D;
            const int scale = static_cast<int>(std::ceil(::log(static_cast<double>(ratio)) / b->log_scale_factor));
            const int predictedScale = std::max(0, std::min(scale, b->n_levels - 1));
            const float radius = b->th * b->scale_factors[predictedScale];
            const std::vector<size_t> indices = g->in_area(u, v, radius, predictedScale - 1, predictedScale + 1);
            if (indices.empty()) continue;
            const uint8_t* desc1 = b->mp_desc + 32 * (size_t)mj;
            int bestDist = 256, bestIdx2 = -1;
            for (size_t idx2 : indices) {
                if (holds[idx2]) continue;
                const int dist = hamming(desc1, b->kp_desc + 32 * (size_t)(k0 + idx2));
                if (dist < bestDist) {
                    bestDist = dist;
                    bestIdx2 = (int)idx2;
                }
            }
            if (bestDist <= b->orb_dist) {
                holds[bestIdx2] = 1;
                owner[bestIdx2] = idx1;
                nmatches++;
                if (b->check_orientation) matchIds.push_back(std::make_pair(idx1, bestIdx2));
            }
        }
        if (b->check_orientation) {
            const float factor = 1.f / HISTO_LENGTH;
            std::vector<int> hist[HISTO_LENGTH];
            for (const auto& m : matchIds) {
                float diff = b->mp_angle[m0 + m.first] - b->kp_angle[k0 + m.second];
                if (diff < 0) diff += 360;
                int bin = cv_round(factor * diff);
                if (bin == HISTO_LENGTH) bin = 0;
                if (bin < 0 || bin >= HISTO_LENGTH) return -1;
                hist[bin].push_back(m.second);
            }
            std::sort(std::begin(hist), std::end(hist),
                      [](const std::vector<int>& l, const std::vector<int>& r) { return l.size() > r.size(); });
            const size_t max1 = hist[0].size(), max2 = hist[1].size(), max3 = hist[2].size();
            int eraseBin = 3;
            if (max2 < 0.1 * max1) eraseBin = 1;
            else if (max3 < 0.1 * max1) eraseBin = 2;
            int reduction = 0;
            for (int bin = eraseBin; bin < HISTO_LENGTH; bin++)
                for (int i2 : hist[bin]) {
                    owner[i2] = -1;
                    reduction++;
                }
            nmatches = (int)matchIds.size() - reduction;
        }
        for (int i = 0; i < nk; i++) kp_match[k0 + i] = owner[i];
        n_matches[f] = nmatches;
    }
    return 0;
}

// ORBmatcher::SearchForInitialization(Frame& frame1, Frame& frame2, prevMatched, matches12, windowSize)
// (ORBmatcher.cc:614-694), literally, pair by pair: octave-0 queries in idx1 order, GetFeaturesInArea
// over octave 0 (:629-636), the matchedDistance skip (:650-651), best / second best (:653-662), the
// ratio test (:665), the take-over of an idx2 held by an earlier query (:667-676), CheckOrientation
// (frame2.keypointsUn, frame1.keypointsUn, matchIds, matches12) (:682-683) with matchIds in push
// order (stale pairs included) and the prevMatched update (:686-688).
int oracle_search_for_initialization(const orbm_init_batch* b, int32_t* matches12_out, int32_t* n_matches) {
    const int TH_LOW = 50, HISTO_LENGTH = 30;
    for (int p = 0; p < b->n_pairs; p++) {
        const int k0 = b->kp_begin[p], n2 = b->kp_begin[p + 1] - k0;
        const int q0 = b->q_begin[p], n1 = b->q_begin[p + 1] - q0;
        std::unique_ptr<FeaturesGrid> g(new FeaturesGrid);
        g->assign(b->kp_xy + 2 * (size_t)k0, b->kp_octave + k0, n2, b->bounds + 4 * (size_t)p, 8);
        int nmatches = 0;
        std::vector<int> matches12(n1, -1);
        std::vector<int> matchedDistance(n2, std::numeric_limits<int>::max());
        std::vector<int> matches21(n2, -1);
        std::vector<std::pair<int, int>> matchIds;
        const float radius = static_cast<float>(b->window);
        for (int idx1 = 0; idx1 < n1; idx1++) {
            const int level1 = b->q_octave[q0 + idx1];
            if (level1 > 0) continue;
            const float u = b->prev_matched[2 * (size_t)(q0 + idx1)], v = b->prev_matched[2 * (size_t)(q0 + idx1) + 1];
            const std::vector<size_t> indices2 = g->in_area(u, v, radius, level1, level1);
            if (indices2.empty()) continue;
            const uint8_t* desc1 = b->q_desc + 32 * (size_t)(q0 + idx1);
            int bestDist = std::numeric_limits<int>::max();
            int secondBestDist = std::numeric_limits<int>::max();
            int bestIdx2 = -1;
            for (size_t idx2 : indices2) {
                const int dist = hamming(desc1, b->kp_desc + 32 * (size_t)(k0 + idx2));
                if (matchedDistance[idx2] <= dist) continue;
                if (dist < bestDist) {
                    secondBestDist = bestDist;
                    bestDist = dist;
                    bestIdx2 = (int)idx2;
                } else if (dist < secondBestDist) {
                    secondBestDist = dist;
                }
            }
            if (bestDist <= TH_LOW && bestDist < secondBestDist * b->nnratio) {
                if (matches21[bestIdx2] >= 0) {
                    matches12[matches21[bestIdx2]] = -1;
                    nmatches--;
                }
                matches12[idx1] = bestIdx2;
                matches21[bestIdx2] = idx1;
                matchedDistance[bestIdx2] = bestDist;
                nmatches++;
                if (b->check_orientation) matchIds.push_back(std::make_pair(bestIdx2, idx1));
            }
        }
        if (b->check_orientation) {   // CheckOrientation(frame2.keypointsUn, frame1.keypointsUn, matchIds, matches12)
            const float factor = 1.f / HISTO_LENGTH;
            std::vector<int> hist[HISTO_LENGTH];
            for (const auto& m : matchIds) {
                float diff = b->kp_angle[k0 + m.first] - b->q_angle[q0 + m.second];
                if (diff < 0) diff += 360;
                int bin = cv_round(factor * diff);
                if (bin == HISTO_LENGTH) bin = 0;
                if (bin < 0 || bin >= HISTO_LENGTH) return -1;   // CV_Assert
                hist[bin].push_back(m.second);
            }
            std::sort(std::begin(hist), std::end(hist),
                      [](const std::vector<int>& l, const std::vector<int>& r) { return l.size() > r.size(); });
            const size_t max1 = hist[0].size(), max2 = hist[1].size(), max3 = hist[2].size();
            int eraseBin = 3;
            if (max2 < 0.1 * max1) eraseBin = 1;
            else if (max3 < 0.1 * max1) eraseBin = 2;
            int reduction = 0;
            for (int bin = eraseBin; bin < HISTO_LENGTH; bin++)
                for (int i2 : hist[bin]) {
                    matches12[i2] = -1;
                    reduction++;
                }
            nmatches = (int)matchIds.size() - reduction;
        }
        for (int i1 = 0; i1 < n1; i1++) {
            matches12_out[q0 + i1] = matches12[i1];
            if (matches12[i1] >= 0) {
                b->prev_matched[2 * (size_t)(q0 + i1)] = b->kp_xy[2 * (size_t)(k0 + matches12[i1])];
                b->prev_matched[2 * (size_t)(q0 + i1) + 1] = b->kp_xy[2 * (size_t)(k0 + matches12[i1]) + 1];
            }
        }
        n_matches[p] = nmatches;
    }
    return 0;
}

// Optimizer::PoseOptimization (src/Optimizer.cc:345-489), frame by frame.
// trace (may be null) receives the records; max_iters / max_trials are optimize()'s budget and g2o's
// _maxTrialsAfterFailure (both 10 in the reference; other values are a test's what-if).
static int pose_optimization_run(const orbba_pose_batch* in, orbba_pose_result* out, POTrace* trace, int max_iters,
                                 int max_trials) {
    const double maxChi2[2] = {5.991, 7.815};   // CHI2_MONO, CHI2_STEREO (:44-45)
    for (int f = 0; f < in->n_frames; f++) {
        const int e0 = in->edge_begin[f], E = in->edge_begin[f + 1] - e0;
        for (int e = 0; e < E; e++) out->outlier[e0 + e] = 0;   // frame->outlier[i] = false (:370)
        const double* R0 = in->pose_R + 9 * (size_t)f;
        const double* t0 = in->pose_t + 3 * (size_t)f;
        if (E < 3) {   // (:412-414) return 0, pose untouched
            std::memcpy(out->pose_R + 9 * (size_t)f, R0, 9 * sizeof(double));
            std::memcpy(out->pose_t + 3 * (size_t)f, t0, 3 * sizeof(double));
            out->n_inliers[f] = 0;
            continue;
        }
        PoseOpt po;
        po.trace = trace;
        if (trace) trace->f = f;
        po.E = E;
        po.xw = in->xw + 3 * (size_t)e0; po.obs = in->obs + 3 * (size_t)e0; po.info = in->inv_sigma2 + e0;
        const double* c = in->cam + 5 * (size_t)f;
        po.fx = c[0]; po.fy = c[1]; po.cx = c[2]; po.cy = c[3]; po.bf = c[4];
        po.stereo.resize(E);
        for (int e = 0; e < E; e++) po.stereo[e] = po.obs[3 * e + 2] < 0 ? 0 : 1;
        po.level.assign(E, 0);
        po.err.assign(3 * (size_t)E, 0);
        SE3 init;   // ToSE3Quat(frame->pose)
        int branch = 0;
        init.q = quat_from_R(R0, &branch);
        if (trace) {
            oracle_po_frame* fr = trace->push_frame();
            if (fr) { fr->branch = branch; fr->flipped = init.q.w < 0; }
        }
        quat_normalize_pos(init.q);
        for (int k = 0; k < 3; k++) init.t[k] = t0[k];
        int noutliers = 0;
        for (int k = 0; k < 4; k++) {   // (:422-484)
            po.pose = init;
            po.act.clear();   // initializeOptimization(0)
            for (int e = 0; e < E; e++) if (po.level[e] == 0) po.act.push_back(e);
            if (trace) trace->k = k;
            const int done = po.optimize(max_iters, max_trials);
            oracle_po_round* rr = trace ? trace->push_round() : nullptr;
            if (rr) {
                rr->n_active = (int)po.act.size(); rr->iterations = done < 0 ? 0 : done; rr->reason = po.end_reason;
                rr->min_margin = HUGE_VAL;
            }
            noutliers = 0;
            for (int e = 0; e < E; e++) {
                const bool was = out->outlier[e0 + e];
                if (was) po.compute_error(e);
                const double c = po.chi2(e), th = maxChi2[po.stereo[e]];
                if (rr) {
                    const double m = std::fabs(c - th) / th;
                    if (m < rr->min_margin) rr->min_margin = m;
                }
                if (c > th) {
                    out->outlier[e0 + e] = 1; po.level[e] = 1; noutliers++;
                } else {
                    out->outlier[e0 + e] = 0; po.level[e] = 0;
                    if (rr && was) rr->n_readmitted++;
                }
            }
            if (rr) rr->n_outliers = noutliers;
            if (k == 2) po.robust = false;   // setRobustKernel(0)
            if (E < 10) break;               // optimizer.edges().size() < 10
        }
        quat_to_R(po.pose.q, out->pose_R + 9 * (size_t)f);
        for (int k = 0; k < 3; k++) out->pose_t[3 * (size_t)f + k] = po.pose.t[k];
        out->n_inliers[f] = E - noutliers;
    }
    return 0;
}

int oracle_pose_optimization(const orbba_pose_batch* in, orbba_pose_result* out) {
    return pose_optimization_run(in, out, nullptr, 10, 10);
}

// The same run with its records written to the caller's arrays (caps in records).  n_out[3] receives the
// numbers of trial, round and frame records (more than a cap: that array was too short).
int oracle_pose_optimization_trace(const orbba_pose_batch* in, orbba_pose_result* out, int max_iters, int max_trials,
                                   oracle_po_trial* trials, int trial_cap, oracle_po_round* rounds, int round_cap,
                                   oracle_po_frame* frames, int frame_cap, int32_t* n_out) {
    POTrace t;
    t.trial = trials; t.trial_cap = trial_cap;
    t.round = rounds; t.round_cap = round_cap;
    t.frame = frames; t.frame_cap = frame_cap;
    const int rc = pose_optimization_run(in, out, &t, max_iters, max_trials);
    n_out[0] = t.n_trials; n_out[1] = t.n_rounds; n_out[2] = t.n_frames;
    return rc;
}

// std::sort of QuadTreeSuppression's DivisibleNode vector (src/ORBextractor.cc:635-643), real
// libstdc++: perm[k] = input index placed at position k.
void oracle_std_sort_sizes(const int32_t* sizes, int n, int32_t* perm) {
    struct DivisibleNode { size_t size; const int32_t* ptr; };
    std::vector<DivisibleNode> v(n);
    for (int i = 0; i < n; i++) v[i] = {(size_t)sizes[i], sizes + i};
    std::sort(v.begin(), v.end(), [](const DivisibleNode& a, const DivisibleNode& b) { return a.size > b.size; });
    for (int i = 0; i < n; i++) perm[i] = (int32_t)(v[i].ptr - sizes);
}

}  // extern "C"
