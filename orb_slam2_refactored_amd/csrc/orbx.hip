// orbx.hip — ORBextractor::Extract on gfx950: the host side.
//
// The kernels live in the stage headers included below, in pipeline order; they and this file are ONE
// translation unit (inlining and register allocation depend on it: no stage is compiled on its own).
// This file holds the extractor handle, the geometry / table set-up, the launch logic and the
// orbx_* C-ABI.
//
// Pipeline for a batch of F frames of identical size (every launch covers all frames of a chunk):
//   1. pyramid   (orbx_pyramid.h): cascaded cv::resize INTER_LINEAR 8U (src/ORBextractor.cc:455-470).
//                Level 0 is the caller's image.  pyramid_pair_kernel builds two levels per launch
//                (levels (1,2), (3,4), (5,6) by default), pyramid_level_kernel the levels left over.
//   2. FAST      (orbx_fast.h): fast_cells_kernel, one wavefront per (frame, column strip of up to
//                fast_cpw 30-px cells): crop -> LDS, FAST-9/16 corner score, cell-local 3x3 NMS at
//                iniThFAST, retry at minThFAST when the cell is empty (DetectFAST :489-540).
//   3. quadtree  (orbx_quadtree.h): quadtree_kernel, one workgroup per (frame, level):
//                QuadTreeSuppression (:542-693) in the reference's list order.
//   4. describe  (orbx_describe.h): describe_prefix_kernel (per-frame level prefix of the kept counts),
//                then describe_kernel, one wavefront per selection slot: IC_Angle, the 7x7 Gaussian
//                blur and the rotated rBRIEF, written in the reference's output order.
//   then once per batch fast_hint_kernel: the FAST speculation hints of the next batch.
// The run-time ORBX_* knobs (orbx_create) select the measured alternatives: the MFMA pyramid, PAIR
// FAST, the wave-per-tree quadtree, the dense describe grid.
// Compiled with -ffp-contract=off so every float expression rounds like the reference's
// ISO C++14 build (no FMA contraction).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

#include <hip/hip_ext.h>

#include "common.h"
#include "qt_sort.h"
#include "sincos_f.h"
#include "stereo.h"

#include "orbx_geom.h"
#include "orbx_pyramid.h"
#include "orbx_fast.h"
#include "orbx_quadtree.h"
#include "orbx_describe.h"

// ==============================================================================================
// Host side: extractor object and C-ABI
// ==============================================================================================
using namespace orbamd;

struct orbx_extractor {
    orbx_params p;
    int device = 0;
    hipStream_t stream = nullptr;
    std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
    std::vector<int> quota;
    std::mutex mu;   // one instance is not re-entrant (as the reference's mutable members)

    // geometry for the current image size
    int g_rows = -1, g_cols = -1;
    Geom geom;
    std::vector<CellDev> cells;
    int NC = 0, PTC = 0;
    size_t qt_lds = 0;
    int qt_ptc0 = 0;        // ORBX_QT_PTC0 (tuning knob): level 0 in its own launch with this LDS point capacity
    size_t qt_lds0 = 0;
    // round 6: the small levels [qtw_l0, nlevels) as one tree per wavefront (quadtree_kernel<true>),
    // four per workgroup, each with its own node capacity / LDS point capacity (ORBX_QT_WAVE=1; exact,
    // measured: pan quadtree -2 %, textured +13 % -- off by default, DESIGN §4 quadtree round 6)
    int qt_wave = 0, qt_wave_wg = 2, qtw_l0 = 0, qtw_nc = 0, qtw_ptc = 0;
    size_t qtw_lds = 0;
    FastLds fl;
    size_t fast_lds = 0;
    int fast_cpw = 16;  // FAST cells per wavefront (4 -> 16: -2 % pan, -17 % textured: fewer first cells without a speculation hint; ORBX_FAST_CPW)
    // a cell runs the speculative iniThFAST pass when the wavefront's previous cell kept at least
    // fast_spec corners at iniThFAST (texture-rich regions); 0 = never (ORBX_FAST_SPEC)
    int fast_spec = 8;
    int fast_pair = 0;      // ORBX_FAST_PAIR=1: fast_cells_kernel<..., PAIR> (two cells per pass; round 6)
    bool fast_pair_on = false;   // requested and the geometry allows it (consecutive strip cells adjacent)
    // a strip's first cell (no predecessor) speculates when its cell kept >= fast_spec corners in frame 0
    // (cell_cnt's frame-0 slot; ORBX_FAST_SPEC_FIRST=0: never)
    int fast_spec_first = 1;
    int nsub = 1;       // sub-batches on side streams (launch_batch; ORBX_NSUB)
    int debug_nc = 0;
    int debug_qt_block = 0;   // test hook (ORBX_DEBUG_QT_BLOCK): launch quadtree_kernel with this block size (FAULT_BLOCK_SIZE)
    uint32_t fault_host = 0;   // test hook (ORBX_DEBUG_NC): shrink the quadtree node capacity to induce FAULT_QT_NODES
    int pyr_mfma = 0;   // ORBX_PYR_MFMA=1: pyramid_pair_mfma_kernel where the level pair's tables fit (measured slower: DESIGN §4)
    std::vector<char> pyr_mfma_ok;   // per level l: the pair (l, l+1) fits pyramid_pair_mfma_kernel
    std::vector<int> pyr_pair_np;    // per level l: pyramid_pair_kernel's NP for the pair (l, l+1), 0: does not fit (pyr_pair_fits)
    DevBuf d_pyrmt, d_pyrkb;         // its A / C fragments per 16-column block, and the blocks' first tap column
    int pyr_pair = 2;   // pyramid_pair_kernel for levels (1,2), (3,4), (5,6) (level 0 16-byte aligned); 1: (2,3), (4,5), (6,7) (ORBX_PYR_PAIR)
    // OpenCV-build switches (orbx_set_opencv_compat; ORBX_TRIG / ORBX_RESIZE_TAIL)
    int trig_float = 0;    // ComputeOrbDescriptor's cos / sin: 0 ::cos(double), 1 cosf / sinf
    // the resize's tail mode V (0, default: the SIMD rounding on every column, as OpenCV's uchar
    // specialisation of VResizeLinear does in its unrolled and scalar tails too; 8-64: a tail with
    // FixedPtCast rounding after a V-byte vector loop; 1: FixedPtCast everywhere).  Parity unpinned.
    int resize_simd = 0;
    std::vector<std::pair<hipStream_t, hipEvent_t>> sub;
    hipEvent_t fork_ev = nullptr;
    // level-split overlap (launch_chunk): level 0's FAST + quadtree on a side stream.  Off by
    // default: measured no gain at C2 (the concurrent kernels share the CUs: pyramid 0.26 -> 0.42 ms,
    // wall time unchanged), and it keeps the per-kernel launch times uncontended.  ORBX_LEVEL_OVERLAP=1
    bool lvl_overlap = false;
    hipStream_t lvl_side = nullptr;
    hipEvent_t lvl_fork = nullptr, lvl_join = nullptr;
    DevBuf d_cells, d_xtab, d_ytab;
    DevBuf d_strips;                 // FAST work items: column strips of cells (fast_cells_kernel)
    DevBuf d_slottab;                // describe: selection slot -> level | rank << 8 (out_frame entries)
    DevBuf d_lvlpre;                 // describe: per-frame level prefix of the kept counts (LVP ints per frame)
    std::vector<int> strip_beg;      // first strip of each level (nlevels + 1 entries)

    // workspace for up to ws_frames frames
    int ws_frames = 0;
    DevBuf d_pyr, d_slots, d_cellcnt, d_P, d_T, d_sel, d_selcnt, d_fault;
    // single-frame host API buffers
    DevBuf d_img, d_kps, d_desc, d_counts;
    DevBuf d_stereo_sad;   // stereo scratch (orbx_stereo_matches_batch_device)
    // every DevBuf member of this struct: a new buffer is added here too (orbx_destroy)
    void release_buffers() {
        DevBuf* bufs[] = {&d_cells, &d_strips, &d_xtab, &d_ytab, &d_pyr, &d_slots, &d_cellcnt, &d_P,
                          &d_T, &d_sel, &d_selcnt, &d_fault, &d_img, &d_kps, &d_desc,
                          &d_counts, &d_stereo_sad, &d_pyrmt, &d_pyrkb, &d_slottab, &d_lvlpre,
                          &d_stereo_out, &d_dstat};
        for (DevBuf* b : bufs) b->release();
    }
    // stage profiling (events on the launch stream)
    int prof = 0;   // bit k: time stage k's launches (orbx_profile_enable)
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev[4];
    std::vector<hipEvent_t> ev_pool;
    // last batch (for GetImagePyramid)
    const uint8_t* last_in = nullptr;
    long long last_fstride = 0;
    size_t last_step = 0;
    int last_frames = 0;
    // dense describe grid (DescGrid): slots per frame from the previous batch's largest total
    int desc_dense = 0;         // ORBX_DESC_DENSE=1: the dense grid (measured no faster, DESIGN §4 describe round 6)
    int desc_force_c = 0;       // test hook (ORBX_DESC_C): this C for every batch (exercises the overflow kernel)
    int desc_c = 0;             // C of the next batch (0: unknown, out_frame)
    DevBuf d_dstat;             // stat[0] = the batch's largest frame total (describe_prefix_kernel)
    int32_t* h_dstat = nullptr; // pinned copy of it
    hipEvent_t dstat_ev = nullptr;
    bool dstat_pending = false;
    bool last_single = false;   // the last extraction was orbx_extract (outputs in d_kps / d_desc / d_counts)
    int last_kcap = 0;          // its output capacity (row stride of d_kps / d_desc)
    DevBuf d_stereo_out;        // orbx_stereo_matches_last: uright | depth on the device
    std::vector<uint8_t> h_stage;   // host staging of the pageable copies (one copy per level / call)
};

// First column that takes FixedPtCast<int, uchar, 22> rounding under tail mode V: after a V-byte
// vector loop ([ext] imgproc/src/resize.cpp VResizeLinearVec_32s8u: `for (; x <= w - V; x += V)` then
// `for (; x < w - V/2; x += V/2)`).  V = 0 (default): none -- the recalled uchar specialisation of
// VResizeLinear rounds its unrolled and scalar tails like the vector op, so every column takes the SIMD
// formula whatever the build's SIMD width.  V = 1: FixedPtCast everywhere.  Modes other than 0 model
// builds whose tail rounds differently; they are kept as sensitivity switches (parity unpinned).
static int resize_tail_x(int w, int V) {
    if (V <= 0) return w;
    if (V == 1) return 0;
    int x = 0;
    for (; x <= w - V; x += V) {}
    for (; x < w - V / 2; x += V / 2) {}
    return x;
}

static int cv_round_d(double v) { return (int)std::lrint(v); }
static int cv_round_f(float v) { return (int)std::lrintf(v); }

static void compute_tables(orbx_extractor* h) {
    const orbx_params& p = h->p;
    const int L = p.nlevels;
    h->scale.resize(L); h->inv_scale.resize(L); h->sigma2.resize(L); h->inv_sigma2.resize(L);
    h->quota.resize(L);
    float s = 1.f;
    for (int l = 0; l < L; l++) {   // ORBextractor::Init (:728-737)
        h->scale[l] = s;
        h->inv_scale[l] = 1.f / s;
        h->sigma2[l] = s * s;
        h->inv_sigma2[l] = 1.f / (s * s);
        s *= p.scaleFactor;
    }
    const double factor = 1 / p.scaleFactor;   // ComputeNumFeaturesPerScale (:472-487)
    double nf = p.nfeatures * (1 - factor) / (1 - std::pow(factor, L));
    int sum = 0;
    for (int l = 0; l < L - 1; l++) {
        h->quota[l] = cv_round_d(nf);
        sum += h->quota[l];
        nf *= factor;
    }
    h->quota[L - 1] = std::max(p.nfeatures - sum, 0);
}

// Level sizes, resize tables, FAST cell grid, buffer layout for a rows x cols input.
static int setup_geometry(orbx_extractor* h, int rows, int cols) {
    if (h->g_rows == rows && h->g_cols == cols) return ORB_OK;
    const int Lc = h->p.nlevels;
    Geom g;
    std::memset(&g, 0, sizeof(g));
    g.nlevels = Lc;
    for (int l = Lc; l < MAX_LEVELS; l++) g.lv[l].out_base = INT_MAX;   // describe's level count
    std::vector<int2> xtab, ytab;
    std::vector<PyrMfmaLane> mt;
    std::vector<int> mkb;
    std::vector<CellDev> cells;
    long long pyr_off = 0, slot = 0, cand = 0;
    int out = 0, NC = 64;
    int prev_w = cols, prev_h = rows;
    for (int l = 0; l < Lc; l++) {
        LevelDev& L = g.lv[l];
        if (l == 0) {
            L.w = cols; L.h = rows; L.stride = cols; L.off = -1; L.tail_x = cols; L.mt_off = -1;
        } else {
            L.h = cv_round_f(h->inv_scale[l] * rows);
            L.w = cv_round_f(h->inv_scale[l] * cols);
            if (L.w <= 0 || L.h <= 0) {
                set_error("pyramid level collapses to zero size");
                return ORB_EINVAL;
            }
            L.stride = (int)align_up(L.w, 16);
            L.off = pyr_off;
            pyr_off += (long long)align_up((size_t)L.stride * L.h, 256);
            // cv::resize tables (same arithmetic as the oracle / OpenCV: pyr_resize_tables)
            L.xtab_off = (int)xtab.size();
            L.ytab_off = (int)ytab.size();
            L.ssx = (double)prev_w / L.w;
            L.ssy = (double)prev_h / L.h;
            L.tail_x = resize_tail_x(L.w, h->resize_simd);
            pyr_resize_tables(prev_w, prev_h, L.w, L.h, xtab, ytab);
            L.mt_off = h->pyr_mfma ? pyr_mfma_tables(xtab.data() + L.xtab_off, L.w, mt, mkb) : -1;
        }
        if (l > 0) {   // the pyramid kernel's LDS source tile must hold a 64x16 output tile's footprint
            const double sc = (double)prev_w / L.w, scy = (double)prev_h / L.h;
            if (sc * PYR_TW + 12 > PYR_SW || scy * PYR_TH + 6 > PYR_SH) {   // conservative rectangle + margins
                set_error("scaleFactor too large for the pyramid tile (max ~1.9)");
                return ORB_EINVAL;
            }
        }
        if (L.w >= 4096 || L.h >= 4096) {
            set_error("image dimensions must be < 4096");
            return ORB_EINVAL;
        }
        prev_w = L.w; prev_h = L.h;
        L.rx = 16; L.ry = 16; L.rw = L.w - 32; L.rh = L.h - 32;
        L.scale = h->scale[l];
        L.size = h->scale[l] * 31;
        L.quota = h->quota[l];
        L.cell_base = (int)cells.size();
        L.ncells = 0;
        L.cand_base = cand;
        L.cand_cap = 0;
        L.nroots = 0;
        L.out_base = out;
        L.out_cap = 0;
        if (L.rw > 0 && L.rh > 0) {
            const int gridw = L.rw / 30, gridh = L.rh / 30;
            if (gridw > 0 && gridh > 0) {
                const int cellw = (int)std::ceil(1. * L.rw / gridw), cellh = (int)std::ceil(1. * L.rh / gridh);
                const int maxx = L.rx + L.rw, maxy = L.ry + L.rh;
                for (int cy = 0, y0 = L.ry; cy < gridh && y0 + 6 < maxy; cy++, y0 += cellh)
                    for (int cx = 0, x0 = L.rx; cx < gridw && x0 + 6 < maxx; cx++, x0 += cellw) {
                        const int y1 = std::min(y0 + cellh + 6, maxy), x1 = std::min(x0 + cellw + 6, maxx);
                        const int zw = x1 - x0 - 6, zh = y1 - y0 - 6;
                        if (zw > MAX_ZONE || zh > MAX_ZONE) {
                            set_error("FAST cell larger than supported zone");
                            return ORB_EINVAL;
                        }
                        CellDev c;
                        c.level = l;
                        c.x0y0 = x0 | (y0 << 16);
                        c.zwzh = zw | (zh << 16);
                        c.slot = (int)slot;
                        const int cap = ((zw + 1) / 2) * ((zh + 1) / 2);
                        slot += cap;
                        L.cand_cap += cap;
                        cells.push_back(c);
                        L.ncells++;
                    }
                L.nroots = cv_round_d(1. * L.rw / L.rh);
                if (L.nroots <= 0 || L.nroots > MAX_ROOTS) {
                    set_error("unsupported aspect ratio (quadtree root count)");
                    return ORB_EINVAL;
                }
                L.hx = 1. * L.rw / L.nroots;
                L.out_cap = std::max(L.quota + 3, 4 * L.nroots) + 1;
                NC = std::max(NC, L.out_cap + 8);
            }
        }
        cand += L.cand_cap;
        out += L.out_cap;
    }
    g.ncells_total = (int)cells.size();
    g.pyr_frame_bytes = std::max<long long>(pyr_off, 256);
    g.slot_frame = std::max<long long>(slot, 1);
    g.cand_frame = std::max<long long>(cand, 1);
    g.out_frame = std::max(out, 1);
    if (g.out_frame >= 0x7fff) {   // describe's u16 level starts (a frame of > 32k selected keypoints)
        set_error("ORBextractor: more than 32766 selection slots per frame (nfeatures too large)");
        return ORB_EINVAL;
    }
    for (int d = 0; d < MAX_LEVELS / 2; d++) g.lv_start[d] = 0x7fff7fffu;
    for (int l = 1; l < Lc; l++)
        g.lv_start[l >> 1] = (g.lv_start[l >> 1] & ~(0xffffu << (16 * (l & 1)))) | ((unsigned)g.lv[l].out_base << (16 * (l & 1)));
    {   // round-up magic for n / out_frame (Granlund-Montgomery; d = 1: t = 0, shifts 0)
        const unsigned d = (unsigned)g.out_frame;
        int lg = 0;
        while ((1ull << lg) < d) lg++;
        g.of_m = (unsigned)((((1ull << lg) - d) << 32) / d + 1);
        g.of_s1 = lg > 0 ? 1 : 0;
        g.of_s2 = lg > 0 ? lg - 1 : 0;
    }
    NC = (int)align_up(std::max(NC, 256), 64);   // >= blockDim: the gather reuses the node scratch
    if (h->debug_nc > 0) NC = (int)align_up(std::max(h->debug_nc, 256), 64);
    // PTC: candidate points kept in LDS (P and T) when a level has at most this many (more: HBM).
    // Sized for workgroups per CU first: the largest multiple of 64 (<= 2048) that fits 4 of them
    // in the 160 KiB (123 VGPRs allow 4), else 3, else 2, each with at least 512 points.  At C2
    // (NC = 448) that is 960 points and 4 workgroups per CU instead of 2048 and 3: quadtree 1.44 ->
    // 1.14 ms per 2048 pan frames, 3.20 -> 2.82 ms per 1024 textured ones.
    const size_t node_lds = (size_t)NC * (2 * sizeof(QtNode) + sizeof(int4) + 2 * sizeof(QtItem) + 2 * sizeof(int));
    int PTC = 2048;
    {
        hipFuncAttributes fa{};
        const size_t stat = hipFuncGetAttributes(&fa, (const void*)quadtree_kernel<false>) == hipSuccess ? fa.sharedSizeBytes : 1024;
        for (int t = QT_WAVES_DEF; t >= 2; t--) {
            const long long room = (long long)(160 * 1024 / t) - (long long)stat - (long long)node_lds;
            const int p = (int)std::min<long long>(2048, room / 8) & ~63;
            if (p >= 512) { PTC = p; break; }
        }
    }
    if (const char* e = getenv("ORBX_QT_PTC")) PTC = std::max(256, std::min(4096, atoi(e)));   // tuning knob
    const size_t lds = node_lds + (size_t)PTC * 8;
    if (lds > 156 * 1024) {   // gfx950: 160 KiB LDS per workgroup
        set_error("nfeatures too large for the quadtree LDS budget (per-level quota <= ~2100)");
        return ORB_EINVAL;
    }
    int PTC0 = 0;
    size_t lds0 = 0;
    if (const char* e = getenv("ORBX_QT_PTC0")) {   // level 0 (the densest) in its own launch
        PTC0 = std::max(256, std::min(8192, atoi(e))) & ~63;
        lds0 = node_lds + (size_t)PTC0 * 8;
        if (lds0 > 156 * 1024) { PTC0 = 0; lds0 = 0; }
    }
    if (std::max(lds, lds0) > 48 * 1024)
        ORB_HIP_TRY(hipFuncSetAttribute((const void*)quadtree_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                        (int)std::max(lds, lds0)));
    // Wave-per-tree levels: the trailing levels whose cells the partitioned gather of one wavefront takes
    // (<= 4 x 64 cells, <= 4 roots); node capacity from their own quotas; LDS points so that
    // qt_wave_wg workgroups of four trees fit a CU (a level with more points keeps them in HBM).
    h->qtw_l0 = g.nlevels;
    if (h->qt_wave) {
        int l0w = g.nlevels;
        while (l0w > 0 && g.lv[l0w - 1].ncells <= 4 * 64 && g.lv[l0w - 1].nroots <= 4) l0w--;
        int ncw = 64;
        for (int l = l0w; l < g.nlevels; l++) ncw = std::max(ncw, g.lv[l].out_cap + 8);
        ncw = (int)align_up(ncw, 64);
        hipFuncAttributes fa{};
        const size_t stat = hipFuncGetAttributes(&fa, (const void*)quadtree_kernel<true>) == hipSuccess ? fa.sharedSizeBytes : 2048;
        const long long per_wave = ((long long)(160 * 1024 / std::max(1, h->qt_wave_wg)) - (long long)stat) / 4;
        const int ptcw = (int)std::min<long long>(2048, (per_wave - (long long)ncw * QT_NODE_BYTES) / 8) & ~63;
        if (l0w < g.nlevels && ptcw >= 64) {
            h->qtw_l0 = l0w;
            h->qtw_nc = ncw;
            h->qtw_ptc = ptcw;
            h->qtw_lds = 4 * ((size_t)ncw * QT_NODE_BYTES + (size_t)ptcw * 8);
            if (h->qtw_lds > 48 * 1024)
                ORB_HIP_TRY(hipFuncSetAttribute((const void*)quadtree_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                (int)h->qtw_lds));
        }
    }
    int rc;
    if ((rc = h->d_cells.reserve(std::max<size_t>(1, cells.size()) * sizeof(CellDev)))) return rc;
    if ((rc = h->d_xtab.reserve(std::max<size_t>(1, xtab.size()) * sizeof(int2)))) return rc;
    if ((rc = h->d_ytab.reserve(std::max<size_t>(1, ytab.size()) * sizeof(int2)))) return rc;
    if (!cells.empty())
        ORB_HIP_TRY(hipMemcpy(h->d_cells.ptr, cells.data(), cells.size() * sizeof(CellDev), hipMemcpyHostToDevice));
    if (!xtab.empty())
        ORB_HIP_TRY(hipMemcpy(h->d_xtab.ptr, xtab.data(), xtab.size() * sizeof(int2), hipMemcpyHostToDevice));
    if (!ytab.empty())
        ORB_HIP_TRY(hipMemcpy(h->d_ytab.ptr, ytab.data(), ytab.size() * sizeof(int2), hipMemcpyHostToDevice));
    {   // describe's slot table: slot s of level l's [out_base, out_base + out_cap) -> l | (s - out_base) << 8
        std::vector<uint32_t> st((size_t)g.out_frame, 0u);
        for (int l = 0; l < Lc; l++)
            for (int i = 0; i < g.lv[l].out_cap; i++) st[(size_t)g.lv[l].out_base + i] = (uint32_t)l | ((uint32_t)i << 8);
        if ((rc = h->d_slottab.reserve(st.size() * sizeof(uint32_t)))) return rc;
        ORB_HIP_TRY(hipMemcpy(h->d_slottab.ptr, st.data(), st.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    // (only with ORBX_PYR_MFMA=1: the default path allocates nothing for it)
    if (!mt.empty() && (rc = h->d_pyrmt.reserve(mt.size() * sizeof(PyrMfmaLane)))) return rc;
    if (!mkb.empty() && (rc = h->d_pyrkb.reserve(mkb.size() * sizeof(int)))) return rc;
    if (!mt.empty())
        ORB_HIP_TRY(hipMemcpy(h->d_pyrmt.ptr, mt.data(), mt.size() * sizeof(PyrMfmaLane), hipMemcpyHostToDevice));
    if (!mkb.empty())
        ORB_HIP_TRY(hipMemcpy(h->d_pyrkb.ptr, mkb.data(), mkb.size() * sizeof(int), hipMemcpyHostToDevice));
    h->pyr_mfma_ok.assign(Lc, 0);
    for (int l = 1; l + 1 < Lc; l++) h->pyr_mfma_ok[l] = h->pyr_mfma && pyr_mfma_pair_fits(g, l, mkb, ytab);
    h->pyr_pair_np.assign(Lc, 0);
    for (int l = 1; l + 1 < Lc; l++) h->pyr_pair_np[l] = pyr_pair_fits(g, l, xtab, ytab);
    h->geom = g;
    h->cells = cells;
    {   // FAST column strips: up to fast_cpw vertically consecutive cells of one column per wavefront
        // (the speculation hint comes from the cell above); consecutive strips are neighbouring
        // columns of the same row block, so the wavefronts running together read adjacent crops
        // and share their cache lines (rows of one level all have the same cell count).
        std::vector<int2> strips;
        h->strip_beg.assign(g.nlevels + 1, 0);
        const int cpw = std::max(1, std::min(h->fast_cpw, 255));
        for (int l = 0; l < g.nlevels; l++) {
            h->strip_beg[l] = (int)strips.size();
            const LevelDev& L = g.lv[l];
            if (L.ncells <= 0) continue;
            const int x00 = cells[L.cell_base].x0y0 & 0xffff;
            int ncx = 0;
            while (ncx < L.ncells && (cells[L.cell_base + ncx].x0y0 >> 16) == (cells[L.cell_base].x0y0 >> 16)) ncx++;
            const int ncy = L.ncells / ncx;
            if (ncx * ncy != L.ncells || (cells[L.cell_base + ncx - 1].x0y0 & 0xffff) < x00) {
                set_error("FAST cell grid is not a rectangle");
                return ORB_EINTERNAL;
            }
            for (int rb = 0; rb < ncy; rb += cpw)
                for (int cx = 0; cx < ncx; cx++) {
                    const int c0 = L.cell_base + rb * ncx + cx, n = std::min(cpw, ncy - rb);
                    for (int k = 1; k < n; k++)   // the kernel takes the zone width from the first cell
                        if ((cells[c0 + k * ncx].zwzh & 0xffff) != (cells[c0].zwzh & 0xffff)) {
                            set_error("FAST strip with unequal zone widths");
                            return ORB_EINTERNAL;
                        }
                    strips.push_back(make_int2(c0, n | (ncx << 8)));
                }
        }
        h->strip_beg[g.nlevels] = (int)strips.size();
        if ((rc = h->d_strips.reserve(std::max<size_t>(1, strips.size()) * sizeof(int2)))) return rc;
        if (!strips.empty())
            ORB_HIP_TRY(hipMemcpy(h->d_strips.ptr, strips.data(), strips.size() * sizeof(int2), hipMemcpyHostToDevice));
    }
    {
        int mzw = 1, mzh = 1;
        for (const CellDev& c : cells) { mzw = std::max(mzw, c.zwzh & 0xffff); mzh = std::max(mzh, c.zwzh >> 16); }
        if (mzw > 64 || mzh > (2 * GR_RING + FQ2_RING) / 8) {   // DetectFAST cells are < 60 px (:508-511)
            set_error("FAST cell larger than the kernel supports");
            return ORB_EINTERNAL;
        }
        // PAIR: every strip's consecutive cells adjacent (zone B starts where zone A ends, same x0), the
        // merged zone's rows within the 7 bits of the pair encoding, and a dense pair's 3 ballot words
        // per pass within the drained ring
        h->fast_pair_on = false;
        if (h->fast_pair) {
            bool ok = 2 * mzh < 128 && 24 * ((2 * mzh + 1) / (mzw <= 32 ? 2 : 1) + 1) <= 2 * (2 * GR_RING + FQ2_RING);
            for (int l = 0; l < g.nlevels && ok; l++) {
                const LevelDev& L = g.lv[l];
                if (L.ncells <= 0) continue;
                int ncx = 0;   // cells per grid row (the strips' cell stride)
                while (ncx < L.ncells && (cells[L.cell_base + ncx].x0y0 >> 16) == (cells[L.cell_base].x0y0 >> 16)) ncx++;
                for (int c = L.cell_base; c + ncx < L.cell_base + L.ncells && ok; c++) {
                    const CellDev &A = cells[c], &B = cells[c + ncx];
                    ok = (A.x0y0 & 0xffff) == (B.x0y0 & 0xffff) && (B.x0y0 >> 16) == (A.x0y0 >> 16) + (A.zwzh >> 16);
                }
            }
            h->fast_pair_on = ok;
        }
        const int zrows = h->fast_pair_on ? 2 * mzh + 1 : mzh;   // zone rows per pass (+ the separator)
        FastLds fl;
        fl.CS = (int)align_up(mzw + 6 + 8, 4);         // +1 shift, +4 dword over-read each side
        if (fl.CS < 4 * ((mzw + 6 + 1 + 3) / 4)) fl.CS = 4 * ((mzw + 6 + 1 + 3) / 4);
        fl.ZS = (int)align_up(mzw + 2, 4);             // zone map with a zero border of 1
        // rows: the tallest crop + slack, and at least the CROP_NG row groups of 4 rows the staging's first
        // batch always stores
        fl.crop_bytes = (int)align_up((size_t)fl.CS * std::max(zrows + 6 + FAST_CROP_SLACK, 4 * CROP_NG), 16);
        fl.mz_bytes = (int)align_up((size_t)fl.ZS * (zrows + 2), 16);
        fl.qcap = 2 * GR_RING + FQ2_RING;   // in u16 entries
        fl.ccap = std::min(FAST_CLIST_CAP, (int)align_up((size_t)mzw * mzh, 8));
        const int nbal = (fl.ccap + 63) / 64;
        h->fast_lds = (size_t)fl.crop_bytes + fl.mz_bytes + 2 * (size_t)(fl.qcap + fl.ccap) +
                      (h->fast_pair_on ? 24 : 16) * (size_t)nbal;
        h->fl = fl;
    }
    h->NC = NC;
    h->PTC = PTC;
    h->qt_lds = lds;
    h->qt_ptc0 = PTC0;
    h->qt_lds0 = lds0;
    h->g_rows = rows;
    h->g_cols = cols;
    h->ws_frames = 0;   // force workspace re-layout
    return ORB_OK;
}

// Output rows a frame can need: the sum of the levels' selection capacities (orbx_max_keypoints).
static int max_keypoints(const Geom& g) {
    int c = 0;
    for (int l = 0; l < g.nlevels; l++) c += g.lv[l].out_cap;
    return c;
}

static int reserve_workspace(orbx_extractor* h, int frames) {
    if (frames <= h->ws_frames) return ORB_OK;
    const Geom& g = h->geom;
    int rc;
    if ((rc = h->d_pyr.reserve((size_t)frames * g.pyr_frame_bytes))) return rc;
    if ((rc = h->d_slots.reserve((size_t)frames * g.slot_frame * 4))) return rc;
    if ((rc = h->d_cellcnt.reserve((size_t)frames * std::max(1, g.ncells_total) * 4))) return rc;
    if ((rc = h->d_P.reserve((size_t)frames * g.cand_frame * 4))) return rc;
    if ((rc = h->d_T.reserve((size_t)frames * g.cand_frame * 4))) return rc;
    if ((rc = h->d_sel.reserve((size_t)frames * g.out_frame * 4))) return rc;
    // + 64 B: describe reads 16 counts from a frame's first (scalar loads, past the last frame too)
    if ((rc = h->d_selcnt.reserve((size_t)frames * g.nlevels * 4 + 64))) return rc;
    if ((rc = h->d_lvlpre.reserve((size_t)frames * LVP * 4))) return rc;
    if (!h->d_fault.ptr) {   // sticky until read (orbx_batch_status / the host Extract)
        if ((rc = h->d_fault.reserve(16))) return rc;
        ORB_HIP_TRY(hipMemset(h->d_fault.ptr, 0, 16));
    }
    h->ws_frames = frames;
    return ORB_OK;
}

static hipEvent_t prof_event(orbx_extractor* h) {
    if (!h->ev_pool.empty()) {
        hipEvent_t e = h->ev_pool.back();
        h->ev_pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

constexpr int ORBX_MIN_SUB_FRAMES = 16;

// Per-launch timing when profiling: hipExtLaunchKernel records the two events as part of the
// kernel's own dispatch (start / completion of that kernel, no marker packets in the stream), so a
// stage's time is the sum of its kernels' durations, as rocprofv3 reports them.
template <typename... KArgs, typename... Args>
static void launch_timed(orbx_extractor* h, int stage, void (*kernel)(KArgs...), dim3 grid, dim3 block,
                         uint32_t shmem, hipStream_t s, Args... args) {
    if (h->prof & (1 << stage)) {
        hipEvent_t a = prof_event(h), b = prof_event(h);
        hipExtLaunchKernelGGL(kernel, grid, block, shmem, s, a, b, 0, static_cast<KArgs>(args)...);
        h->prof_ev[stage].push_back({a, b});
    } else {
        hipLaunchKernelGGL(kernel, grid, block, shmem, s, static_cast<KArgs>(args)...);
    }
}

// fast_cells_kernel's instantiation for a launch: the C1-C3 geometries' row strides at compile time,
// any other geometry's from FastLds
static auto fast_kernel_for(const FastLds& fl, bool pair) -> decltype(&fast_cells_kernel<0, 0, false>) {
    if (pair)
        return fl.CS == 48 && fl.ZS == 36   ? fast_cells_kernel<48, 36, true>
               : fl.CS == 52 && fl.ZS == 40 ? fast_cells_kernel<52, 40, true>
                                            : fast_cells_kernel<0, 0, true>;
    return fl.CS == 48 && fl.ZS == 36   ? fast_cells_kernel<48, 36, false>
           : fl.CS == 52 && fl.ZS == 40 ? fast_cells_kernel<52, 40, false>
                                        : fast_cells_kernel<0, 0, false>;
}

// All four stages for frames [f0, f0 + F) of the workspace, enqueued on st.  Every kernel indexes
// its per-frame buffers from the frame index within the launch, so a chunk is launched with base
// pointers advanced by f0 frames.  planted (orbx_debug_describe): the selection words and counts are already
// in d_sel / d_selcnt, so FAST and the quadtree are left out; the pyramid and describe launches are the same.
static void launch_chunk(orbx_extractor* h, int f0, const uint8_t* d_imgs, int F, long long fstride, int step,
                         orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_counts, int cap, hipStream_t st,
                         hipStream_t side = nullptr, bool planted = false) {
    const Geom& g = h->geom;
    uint8_t* pyr = h->d_pyr.as<uint8_t>() + (long long)f0 * g.pyr_frame_bytes;
    d_imgs += (long long)f0 * fstride;
    d_kps += (long long)f0 * cap;
    d_desc += (long long)f0 * cap * 32;
    d_counts += f0;
    uint32_t* slots = h->d_slots.as<uint32_t>() + (long long)f0 * g.slot_frame;
    int* cellcnt = h->d_cellcnt.as<int>() + (long long)f0 * g.ncells_total;
    uint32_t* Pb = h->d_P.as<uint32_t>() + (long long)f0 * g.cand_frame;
    uint32_t* Tb = h->d_T.as<uint32_t>() + (long long)f0 * g.cand_frame;
    uint32_t* sel = h->d_sel.as<uint32_t>() + (long long)f0 * g.out_frame;
    int* selcnt = h->d_selcnt.as<int>() + (long long)f0 * g.nlevels;
    uint32_t* fault = h->d_fault.as<uint32_t>();
    auto fast = [&](int l0, int l1, hipStream_t s) {   // levels [l0, l1)
        const int sb = h->strip_beg[l0], ns = h->strip_beg[l1] - sb;
        if (ns <= 0) return;
        launch_timed(h, 1, fast_kernel_for(h->fl, h->fast_pair_on), dim3((unsigned)(ns * F)), dim3(64), (uint32_t)h->fast_lds, s,
                           g, h->d_cells.as<CellDev>(), h->d_strips.as<int2>(), d_imgs, fstride, step, pyr, h->p.iniThFAST,
                           h->p.minThFAST, slots, cellcnt, fault, h->fl, sb, ns,
                           h->fast_spec > 0 && h->fast_spec_first ? h->fast_spec | (1 << 29) : h->fast_spec);
    };
    const unsigned qt_block = h->debug_qt_block ? (unsigned)h->debug_qt_block : (unsigned)QT_THREADS;
    auto quadtree = [&](int l0, int nl, hipStream_t s) {
        if (nl <= 0) return;
        // levels from qtw_l0 on: one tree per wavefront, four per workgroup (quadtree_kernel<true>)
        const int lw = std::max(l0, h->qtw_l0), nw_lv = l0 + nl - lw;
        if (nw_lv > 0) {
            launch_timed(h, 2, quadtree_kernel<true>, dim3((unsigned)F, (unsigned)((nw_lv + 3) / 4)), dim3(qt_block),
                         (uint32_t)h->qtw_lds, s, g, cellcnt, slots, h->d_cells.as<CellDev>(), Pb, Tb, sel, selcnt, h->qtw_nc,
                         h->qtw_ptc, fault, lw, nw_lv);
            nl -= nw_lv;
            if (nl <= 0) return;
        }
        if (h->qt_ptc0 > 0 && l0 == 0) {   // tuning knob: level 0 alone, with its own LDS point capacity
            launch_timed(h, 2, quadtree_kernel<false>, dim3((unsigned)F, 1u), dim3(qt_block), (uint32_t)h->qt_lds0, s, g,
                         cellcnt, slots, h->d_cells.as<CellDev>(), Pb, Tb, sel, selcnt, h->NC, h->qt_ptc0, fault, 0, 1);
            l0 = 1;
            if (--nl <= 0) return;
        }
        launch_timed(h, 2, quadtree_kernel<false>, dim3((unsigned)F, (unsigned)nl), dim3(qt_block), (uint32_t)h->qt_lds, s,
                     g, cellcnt, slots, h->d_cells.as<CellDev>(), Pb, Tb, sel, selcnt, h->NC, h->PTC, fault, l0, nl);
    };
    // levels l and l+1 in one pyramid_pair_kernel launch where the shapes fit its LDS rectangles
    // (returns the number of extra levels built)
    auto pyramid = [&](int l) -> int {
        const int first = h->pyr_pair == 2 ? 1 : 2;   // pairs (1,2), (3,4), (5,6) or (2,3), (4,5), (6,7)
        const bool a16 = l > 1 || (((uintptr_t)d_imgs | (uintptr_t)fstride | (uintptr_t)step) & 15) == 0;
        const bool pair = h->pyr_pair && l >= first && (l - first) % 2 == 0 && l + 1 < g.nlevels && a16;
        // one workgroup per 64x64 tile of the launch's last level
        auto tiles = [&](int lt) {
            return dim3((unsigned)((g.lv[lt].w + PYR_TW - 1) / PYR_TW), (unsigned)((g.lv[lt].h + PYR_TH - 1) / PYR_TH),
                        (unsigned)F);
        };
        if (pair && h->pyr_mfma && h->pyr_mfma_ok[l]) {
            launch_timed(h, 0, pyramid_pair_mfma_kernel, tiles(l + 1), dim3(256), 0u, st, g, l, d_imgs, fstride, step, pyr,
                         h->d_ytab.as<int2>(), h->d_pyrmt.as<PyrMfmaLane>(), h->d_pyrkb.as<int>());
            return 1;
        }
        if (pair && h->pyr_pair_np[l]) {
            launch_timed(h, 0, h->pyr_pair_np[l] <= 7 ? pyramid_pair_kernel<7> : pyramid_pair_kernel<PP_MAXP>, tiles(l + 1),
                         dim3(256), 0u, st, g, l, d_imgs, fstride, step, pyr, h->d_xtab.as<int2>(), h->d_ytab.as<int2>());
            return 1;
        }
        launch_timed(h, 0, pyramid_level_kernel, tiles(l), dim3(256), 0u, st, g, l, d_imgs, fstride, step, pyr,
                     h->d_xtab.as<int2>(), h->d_ytab.as<int2>());
        return 0;
    };
    const int nc0 = g.lv[0].ncells;
    if (side && nc0 > 0 && g.nlevels > 1 && !planted) {
        // Level 0 needs no pyramid: its FAST + quadtree run on the side stream while the main
        // stream builds levels 1..7 (latency-bound cascade) and runs their FAST / quadtree, so the
        // level-0 tree's serial rounds overlap the FAST work of the other levels.
        (void)hipStreamWaitEvent(side, h->lvl_fork, 0);
        fast(0, 1, side);
        quadtree(0, 1, side);
        (void)hipEventRecord(h->lvl_join, side);
        {
            for (int l = 1; l < g.nlevels; l++) l += pyramid(l);
        }
        fast(1, g.nlevels, st);
        quadtree(1, g.nlevels - 1, st);
        (void)hipStreamWaitEvent(st, h->lvl_join, 0);
    } else {
        {
            for (int l = 1; l < g.nlevels; l++) l += pyramid(l);
        }
        if (!planted) {
            fast(0, g.nlevels, st);
            quadtree(0, g.nlevels, st);
        }
    }
    int* lvlpre = h->d_lvlpre.as<int>() + (long long)f0 * LVP;
    hipLaunchKernelGGL(describe_prefix_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, st, (const int*)selcnt,
                       g.nlevels, F, lvlpre, d_counts, h->d_dstat.as<int>());
    // the dense grid: C slots per frame (from the previous batch's largest total), the overflow kernel for
    // rows >= C of any frame with more (DescGrid); or the slot-table grid (out_frame slots)
    const int rows_max = std::min(g.out_frame, cap);
    const int C = h->desc_dense ? std::max(1, std::min(h->desc_c > 0 ? h->desc_c : rows_max, rows_max)) : 0;
    DescGrid dg{};
    if (C > 0) {
        dg.C = C;
        const unsigned d = (unsigned)C;
        int lg = 0;
        while ((1ull << lg) < d) lg++;
        dg.m = (unsigned)((((1ull << lg) - d) << 32) / d + 1);
        dg.s1 = lg > 0 ? 1 : 0;
        dg.s2 = lg > 0 ? lg - 1 : 0;
    }
    launch_timed(h, 3, h->trig_float ? describe_kernel<1> : describe_kernel<0>,
                 dim3((unsigned)(C > 0 ? C : g.out_frame), (unsigned)F), dim3(64), 0u, st, g, d_imgs, fstride, step, pyr,
                 sel, selcnt, d_kps, d_desc, d_counts, cap, h->d_slottab.as<uint32_t>(), lvlpre, dg);
    if (C > 0 && C < rows_max)
        launch_timed(h, 3, h->trig_float ? describe_overflow_kernel<1> : describe_overflow_kernel<0>,
                     dim3((unsigned)std::min(F, 2048)), dim3(64), 0u, st, g, d_imgs, fstride, step, pyr, sel, d_kps, d_desc,
                     cap, (const int*)lvlpre, F, C);
}

// The first-cell hint bits for the next launch (fast_hint_kernel): once per batch, on st after every
// sub-batch and side stream has joined, so no fast_cells launch of this batch is still reading the strip
// descriptors it rewrites, and frame 0's cell counts (the first chunk's) are final.
static int launch_fast_hint(orbx_extractor* h, hipStream_t st) {
    if (!(h->fast_spec > 0 && h->fast_spec_first)) return ORB_OK;
    const int ns = h->strip_beg[h->geom.nlevels];
    if (ns <= 0) return ORB_OK;
    hipLaunchKernelGGL(fast_hint_kernel, dim3((unsigned)((ns + 255) / 256)), dim3(256), 0, st, h->d_strips.as<int2>(),
                       h->d_cellcnt.as<int>(), ns);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

// Frames are split into sub-batches on the handle's side streams (fork/join with events on st) so
// that one sub-batch's latency-bound stages (the short pyramid levels, the quadtree's level-0 tail)
// overlap another's FAST / describe work.
// The dense describe grid's C for this batch: the previous batch's largest frame total (read back
// asynchronously; a copy not yet landed keeps the last C) plus a margin, rounded up to 64.
static int describe_grid_begin(orbx_extractor* h, hipStream_t st) {
    if (!h->dstat_ev) {
        ORB_HIP_TRY(hipEventCreateWithFlags(&h->dstat_ev, hipEventDisableTiming));
        ORB_HIP_TRY(hipHostMalloc((void**)&h->h_dstat, 64, hipHostMallocDefault));
        int rc;
        if ((rc = h->d_dstat.reserve(64))) return rc;
    }
    if (h->dstat_pending && hipEventQuery(h->dstat_ev) == hipSuccess) {
        const int mx = *h->h_dstat;
        h->desc_c = (int)align_up((size_t)std::max(mx + 32, 64), 64);
        h->dstat_pending = false;
    }
    if (h->desc_force_c > 0) h->desc_c = h->desc_force_c;
    ORB_HIP_TRY(hipMemsetAsync(h->d_dstat.ptr, 0, 4, st));
    return ORB_OK;
}
static int describe_grid_end(orbx_extractor* h, hipStream_t st) {
    if (h->dstat_pending) return ORB_OK;   // the previous read-back has not landed: keep its slot
    ORB_HIP_TRY(hipMemcpyAsync(h->h_dstat, h->d_dstat.ptr, 4, hipMemcpyDeviceToHost, st));
    ORB_HIP_TRY(hipEventRecord(h->dstat_ev, st));
    h->dstat_pending = true;
    return ORB_OK;
}

static int launch_batch(orbx_extractor* h, const uint8_t* d_imgs, int F, long long fstride, int step,
                        orbx_keypoint* d_kps, uint8_t* d_desc, int32_t* d_counts, int cap, hipStream_t st) {
    {
        const int rc = describe_grid_begin(h, st);
        if (rc) return rc;
    }
    int nsub = std::min(h->nsub, F / ORBX_MIN_SUB_FRAMES);
    if (nsub <= 1) {
        hipStream_t side = nullptr;
        if (h->lvl_overlap) {
            if (!h->lvl_side) {
                ORB_HIP_TRY(hipStreamCreateWithFlags(&h->lvl_side, hipStreamNonBlocking));
                ORB_HIP_TRY(hipEventCreateWithFlags(&h->lvl_fork, hipEventDisableTiming));
                ORB_HIP_TRY(hipEventCreateWithFlags(&h->lvl_join, hipEventDisableTiming));
            }
            ORB_HIP_TRY(hipEventRecord(h->lvl_fork, st));
            side = h->lvl_side;
        }
        launch_chunk(h, 0, d_imgs, F, fstride, step, d_kps, d_desc, d_counts, cap, st, side);
    } else {
        while ((int)h->sub.size() < nsub) {
            hipStream_t s2;
            ORB_HIP_TRY(hipStreamCreateWithFlags(&s2, hipStreamNonBlocking));
            hipEvent_t e;
            ORB_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
            h->sub.push_back({s2, e});
        }
        if (!h->fork_ev) ORB_HIP_TRY(hipEventCreateWithFlags(&h->fork_ev, hipEventDisableTiming));
        ORB_HIP_TRY(hipEventRecord(h->fork_ev, st));
        int f0 = 0;
        for (int i = 0; i < nsub; i++) {
            const int Fi = F / nsub + (i < F % nsub ? 1 : 0);
            ORB_HIP_TRY(hipStreamWaitEvent(h->sub[i].first, h->fork_ev, 0));
            launch_chunk(h, f0, d_imgs, Fi, fstride, step, d_kps, d_desc, d_counts, cap, h->sub[i].first);
            ORB_HIP_TRY(hipEventRecord(h->sub[i].second, h->sub[i].first));
            ORB_HIP_TRY(hipStreamWaitEvent(st, h->sub[i].second, 0));
            f0 += Fi;
        }
    }
    ORB_HIP_TRY(hipGetLastError());
    const int rc = describe_grid_end(h, st);
    return rc ? rc : launch_fast_hint(h, st);
}

static int check_fault(orbx_extractor* h) {
    uint32_t f = 0;
    ORB_HIP_TRY(hipMemcpy(&f, h->d_fault.ptr, 4, hipMemcpyDeviceToHost));
    if (f) {
        ORB_HIP_TRY(hipMemset(h->d_fault.ptr, 0, 4));
        set_error("device capacity check failed (fault mask " + std::to_string(f) + ")");
        return ORB_EINTERNAL;
    }
    return ORB_OK;
}

namespace orbamd {
// One workgroup per frame: rows [0, counts[f]) of the frame's slots -> out rows from incl[f] - counts[f],
// each 32-byte row as two uint4 (lanes take consecutive 16-byte halves: coalesced both ways).
__global__ __launch_bounds__(256) void pack_rows_kernel(const uint4* __restrict__ desc, int cap,
                                                        const int* __restrict__ counts, const int* __restrict__ incl,
                                                        uint4* __restrict__ out, int out_rows) {
    const int f = blockIdx.x;
    const int c = counts[f];
    const int n = min(max(c, 0), cap);                // never read past the frame's slots
    const long long start = (long long)incl[f] - c;   // the caller's layout
    const long long r0 = max(start, 0ll), r1 = min(start + n, (long long)out_rows);   // never write past out
    const uint4* src = desc + (long long)f * cap * 2;
    for (long long i = 2 * r0 + threadIdx.x; i < 2 * r1; i += blockDim.x) out[i] = src[i - 2 * start];
}

}  // namespace orbamd

extern "C" {

int orbx_create(const orbx_params* params, int device, orbx_extractor** out) {
    ORB_CHECK_ARG(params && out, "null argument");
    ORB_CHECK_ARG(params->nlevels >= 1 && params->nlevels <= MAX_LEVELS, "nlevels must be in [1,16]");
    ORB_CHECK_ARG(params->nfeatures >= 0 && params->scaleFactor > 1.0f, "bad nfeatures / scaleFactor");
    int ndev = 0;
    ORB_HIP_TRY(hipGetDeviceCount(&ndev));
    ORB_CHECK_ARG(device >= 0 && device < ndev, "no such HIP device");
    ORB_HIP_TRY(hipSetDevice(device));
    orbx_extractor* h = new orbx_extractor();
    h->p = *params;
    h->device = device;
    if (const char* e = getenv("ORBX_FAST_CPW")) h->fast_cpw = std::max(1, std::min(64, atoi(e)));   // tuning knobs
    if (const char* e = getenv("ORBX_FAST_SPEC")) h->fast_spec = std::max(-1, atoi(e));   // -1: every cell
    if (const char* e = getenv("ORBX_FAST_PAIR")) h->fast_pair = atoi(e) != 0;
    if (const char* e = getenv("ORBX_QT_WAVE")) h->qt_wave = atoi(e) != 0;
    if (const char* e = getenv("ORBX_QT_WAVE_WG")) h->qt_wave_wg = std::max(1, std::min(4, atoi(e)));
    if (const char* e = getenv("ORBX_FAST_SPEC_FIRST")) h->fast_spec_first = atoi(e) != 0;

    if (const char* e = getenv("ORBX_NSUB")) h->nsub = std::max(1, std::min(8, atoi(e)));
    if (const char* e = getenv("ORBX_PYR_PAIR")) h->pyr_pair = std::max(0, std::min(2, atoi(e)));
    if (const char* e = getenv("ORBX_PYR_MFMA")) h->pyr_mfma = atoi(e) != 0;
    if (const char* e = getenv("ORBX_LEVEL_OVERLAP")) h->lvl_overlap = atoi(e) != 0;
    if (const char* e = getenv("ORBX_DEBUG_NC")) h->debug_nc = atoi(e);
    if (const char* e = getenv("ORBX_DESC_DENSE")) h->desc_dense = atoi(e) != 0;
    if (const char* e = getenv("ORBX_DESC_C")) h->desc_force_c = std::max(0, atoi(e));
    if (const char* e = getenv("ORBX_DEBUG_QT_BLOCK")) {
        const int b = atoi(e);
        if (b >= 64 && b <= QT_THREADS && b % 64 == 0) h->debug_qt_block = b;
    }
    // OpenCV-build switches (orbx_set_opencv_compat): ORBX_TRIG=double|float, ORBX_RESIZE_TAIL=V
    if (const char* e = getenv("ORBX_TRIG")) h->trig_float = (e[0] == 'f' || e[0] == '1') ? 1 : 0;
    if (const char* e = getenv("ORBX_RESIZE_TAIL")) {
        const int v = atoi(e);
        if (v == 0 || v == 1 || v == 8 || v == 16 || v == 32 || v == 64) h->resize_simd = v;
    }
    compute_tables(h);
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete h;
        set_error(std::string("hipStreamCreate: ") + hipGetErrorString(e));
        return ORB_EHIP;
    }
    *out = h;
    return ORB_OK;
}

int orbx_destroy(orbx_extractor* h) {
    if (!h) return ORB_OK;
    (void)hipSetDevice(h->device);
    h->release_buffers();
    for (auto& v : h->prof_ev)
        for (auto& pr : v) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    for (auto& se : h->sub) { (void)hipStreamDestroy(se.first); (void)hipEventDestroy(se.second); }
    if (h->fork_ev) (void)hipEventDestroy(h->fork_ev);
    if (h->lvl_side) (void)hipStreamDestroy(h->lvl_side);
    if (h->lvl_fork) (void)hipEventDestroy(h->lvl_fork);
    if (h->lvl_join) (void)hipEventDestroy(h->lvl_join);
    if (h->dstat_ev) (void)hipEventDestroy(h->dstat_ev);
    if (h->h_dstat) (void)hipHostFree(h->h_dstat);
    delete h;
    return ORB_OK;
}

int orbx_set_opencv_compat(orbx_extractor* h, int trig_mode, int resize_simd) {
    ORB_CHECK_ARG(h, "null extractor");
    ORB_CHECK_ARG(trig_mode >= -1 && trig_mode <= 1, "trig_mode must be -1 (keep), 0 (double) or 1 (float)");
    ORB_CHECK_ARG(resize_simd == -1 || resize_simd == 0 || resize_simd == 1 || resize_simd == 8 || resize_simd == 16 ||
                      resize_simd == 32 || resize_simd == 64,
                  "resize_simd must be -1 (keep), 0, 1, 8, 16, 32 or 64");
    std::lock_guard<std::mutex> lk(h->mu);
    if (trig_mode >= 0) h->trig_float = trig_mode;
    if (resize_simd >= 0 && resize_simd != h->resize_simd) {
        h->resize_simd = resize_simd;
        h->g_rows = h->g_cols = -1;   // the levels' tail columns change: rebuild the geometry
    }
    return ORB_OK;
}

int orbx_get_opencv_compat(const orbx_extractor* h, int* trig_mode, int* resize_simd) {
    ORB_CHECK_ARG(h, "null extractor");
    if (trig_mode) *trig_mode = h->trig_float;
    if (resize_simd) *resize_simd = h->resize_simd;
    return ORB_OK;
}

int orbx_scale_tables(const orbx_extractor* h, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2,
                      int32_t* features_per_level) {
    ORB_CHECK_ARG(h, "null extractor");
    for (int l = 0; l < h->p.nlevels; l++) {
        if (scale) scale[l] = h->scale[l];
        if (inv_scale) inv_scale[l] = h->inv_scale[l];
        if (sigma2) sigma2[l] = h->sigma2[l];
        if (inv_sigma2) inv_sigma2[l] = h->inv_sigma2[l];
        if (features_per_level) features_per_level[l] = h->quota[l];
    }
    return ORB_OK;
}

int orbx_max_keypoints(const orbx_extractor* hc, int rows, int cols, int32_t* cap) {
    ORB_CHECK_ARG(hc && cap && rows > 0 && cols > 0, "bad argument");
    orbx_extractor* h = const_cast<orbx_extractor*>(hc);
    std::lock_guard<std::mutex> lk(h->mu);
    ORB_HIP_TRY(hipSetDevice(h->device));
    int rc = setup_geometry(h, rows, cols);
    if (rc) return rc;
    *cap = max_keypoints(h->geom);
    return ORB_OK;
}

int orbx_extract_batch_device(orbx_extractor* h, const uint8_t* d_imgs, int n_frames, int rows, int cols,
                              size_t frame_stride, size_t step, orbx_keypoint* d_kps, uint8_t* d_desc,
                              int32_t* d_counts, int cap, void* stream) {
    ORB_CHECK_ARG(h && d_imgs && d_kps && d_desc && d_counts, "null argument");
    ORB_CHECK_ARG(n_frames > 0 && n_frames <= 65535 && rows > 0 && cols > 0, "bad batch shape");
    ORB_CHECK_ARG(step >= (size_t)cols && step < (1u << 31), "bad row step");
    std::lock_guard<std::mutex> lk(h->mu);
    ORB_HIP_TRY(hipSetDevice(h->device));
    int rc = setup_geometry(h, rows, cols);
    if (rc) return rc;
    if (cap < max_keypoints(h->geom)) {
        set_error("cap < orbx_max_keypoints()");
        return ORB_ECAP;
    }
    if ((rc = reserve_workspace(h, n_frames))) return rc;
    hipStream_t st = (hipStream_t)stream;   // NULL = the default stream, like every HIP API
    h->last_in = d_imgs;
    h->last_single = false;
    h->last_fstride = (long long)frame_stride;
    h->last_step = step;
    h->last_frames = n_frames;
    return launch_batch(h, d_imgs, n_frames, (long long)frame_stride, (int)step, d_kps, d_desc, d_counts, cap, st);
}

int orbx_extract(orbx_extractor* h, const uint8_t* img, int rows, int cols, size_t step, orbx_keypoint* kps,
                 uint8_t* desc, int cap, int* n) {
    ORB_CHECK_ARG(h && img && n, "null argument");
    ORB_CHECK_ARG(rows > 0 && cols > 0 && step >= (size_t)cols, "image must be a non-empty CV_8U matrix");
    std::lock_guard<std::mutex> lk(h->mu);
    ORB_HIP_TRY(hipSetDevice(h->device));
    int rc = setup_geometry(h, rows, cols);
    if (rc) return rc;
    const int kcap = max_keypoints(h->geom);
    if ((rc = reserve_workspace(h, 1))) return rc;
    if ((rc = h->d_img.reserve((size_t)rows * cols))) return rc;
    if ((rc = h->d_kps.reserve((size_t)kcap * sizeof(orbx_keypoint)))) return rc;
    if ((rc = h->d_desc.reserve((size_t)kcap * 32))) return rc;
    if ((rc = h->d_counts.reserve(16))) return rc;
    hipStream_t st = h->stream;
    // a contiguous image (the usual cv::Mat) goes up in one 1D copy: a pitched copy from pageable memory
    // may be staged row by row
    if (step == (size_t)cols)
        ORB_HIP_TRY(hipMemcpyAsync(h->d_img.ptr, img, (size_t)rows * cols, hipMemcpyHostToDevice, st));
    else
        ORB_HIP_TRY(hipMemcpy2DAsync(h->d_img.ptr, cols, img, step, cols, rows, hipMemcpyHostToDevice, st));
    h->last_in = h->d_img.as<uint8_t>();
    h->last_fstride = (long long)rows * cols;
    h->last_step = cols;
    h->last_frames = 1;
    h->last_single = true;
    h->last_kcap = kcap;
    rc = launch_batch(h, h->d_img.as<uint8_t>(), 1, (long long)rows * cols, cols, h->d_kps.as<orbx_keypoint>(),
                      h->d_desc.as<uint8_t>(), h->d_counts.as<int32_t>(), kcap, st);
    if (rc) return rc;
    int32_t total = 0;
    ORB_HIP_TRY(hipMemcpyAsync(&total, h->d_counts.ptr, 4, hipMemcpyDeviceToHost, st));
    ORB_HIP_TRY(hipStreamSynchronize(st));
    if ((rc = check_fault(h))) return rc;
    *n = total;
    if (total == 0) return ORB_OK;   // reference: keypoints left untouched (:778-782)
    if (total > cap) {
        set_error("output capacity too small");
        return ORB_ECAP;
    }
    ORB_CHECK_ARG(kps && desc, "null output");
    ORB_HIP_TRY(hipMemcpyAsync(kps, h->d_kps.ptr, (size_t)total * sizeof(orbx_keypoint), hipMemcpyDeviceToHost, st));
    ORB_HIP_TRY(hipMemcpyAsync(desc, h->d_desc.ptr, (size_t)total * 32, hipMemcpyDeviceToHost, st));
    ORB_HIP_TRY(hipStreamSynchronize(st));
    return ORB_OK;
}

int orbx_batch_status(orbx_extractor* h, void* stream, uint32_t* fault_mask) {
    ORB_CHECK_ARG(h && fault_mask, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    ORB_HIP_TRY(hipSetDevice(h->device));
    *fault_mask = 0;
    if (!h->d_fault.ptr) return ORB_OK;   // nothing has run
    hipStream_t st = (hipStream_t)stream;
    ORB_HIP_TRY(hipMemcpyAsync(&h->fault_host, h->d_fault.ptr, 4, hipMemcpyDeviceToHost, st));
    ORB_HIP_TRY(hipMemsetAsync(h->d_fault.ptr, 0, 4, st));
    ORB_HIP_TRY(hipStreamSynchronize(st));
    *fault_mask = h->fault_host;
    if (h->fault_host) {
        set_error("device capacity check failed in a batch (fault mask " + std::to_string(h->fault_host) + ")");
        return ORB_EINTERNAL;
    }
    return ORB_OK;
}

int orbx_fault_word_device(orbx_extractor* h, uint32_t** d_fault) {
    ORB_CHECK_ARG(h && d_fault, "null argument");
    std::lock_guard<std::mutex> lk(h->mu);
    ORB_HIP_TRY(hipSetDevice(h->device));
    int rc;
    if (!h->d_fault.ptr) {
        if ((rc = h->d_fault.reserve(16))) return rc;
        ORB_HIP_TRY(hipMemset(h->d_fault.ptr, 0, 16));
    }
    *d_fault = h->d_fault.as<uint32_t>();
    return ORB_OK;
}

int orbx_pyramid_device(const orbx_extractor* h, int frame, int level, const uint8_t** ptr, int* rows, int* cols,
                        size_t* step) {
    ORB_CHECK_ARG(h && ptr && h->last_in, "no extraction has run");
    ORB_CHECK_ARG(frame >= 0 && frame < h->last_frames && level >= 0 && level < h->geom.nlevels, "bad index");
    const LevelDev& L = h->geom.lv[level];
    if (level == 0) {
        *ptr = h->last_in + (long long)frame * h->last_fstride;
        if (step) *step = h->last_step;
    } else {
        *ptr = h->d_pyr.as<uint8_t>() + (long long)frame * h->geom.pyr_frame_bytes + L.off;
        if (step) *step = (size_t)L.stride;
    }
    if (rows) *rows = L.h;
    if (cols) *cols = L.w;
    return ORB_OK;
}

int orbx_pyramid_level(const orbx_extractor* h, int level, uint8_t* dst, size_t dst_step, int* rows, int* cols) {
    const uint8_t* p = nullptr;
    int r = 0, c = 0;
    size_t st = 0;
    int rc = orbx_pyramid_device(h, 0, level, &p, &r, &c, &st);
    if (rc) return rc;
    if (rows) *rows = r;
    if (cols) *cols = c;
    if (!dst) return ORB_OK;
    ORB_CHECK_ARG(dst_step >= (size_t)c, "dst_step too small");
    ORB_HIP_TRY(hipSetDevice(h->device));
    ORB_HIP_TRY(hipStreamSynchronize(h->stream));
    if (dst_step == st) {
        ORB_HIP_TRY(hipMemcpy(dst, p, (size_t)(r - 1) * st + c, hipMemcpyDeviceToHost));
    } else {   // one 1D copy of the level's rows into host staging, then the row repack on the host: a
               // pitched copy into pageable memory may be staged row by row (ms per level)
        std::vector<uint8_t>& tmp = const_cast<orbx_extractor*>(h)->h_stage;
        tmp.resize((size_t)(r - 1) * st + c);
        ORB_HIP_TRY(hipMemcpy(tmp.data(), p, tmp.size(), hipMemcpyDeviceToHost));
        for (int y = 0; y < r; y++) std::memcpy(dst + (size_t)y * dst_step, tmp.data() + (size_t)y * st, (size_t)c);
    }
    return ORB_OK;
}

int orbx_debug_level_candidates(const orbx_extractor* h, int frame, int level, uint32_t* out, int cap, int* n) {
    ORB_CHECK_ARG(h && n && h->last_frames > 0, "no extraction has run");
    ORB_CHECK_ARG(frame >= 0 && frame < h->last_frames && level >= 0 && level < h->geom.nlevels, "bad index");
    ORB_HIP_TRY(hipSetDevice(h->device));
    ORB_HIP_TRY(hipDeviceSynchronize());
    const Geom& g = h->geom;
    const LevelDev& L = g.lv[level];
    std::vector<int> cnt(std::max(1, L.ncells));
    if (L.ncells)
        ORB_HIP_TRY(hipMemcpy(cnt.data(), h->d_cellcnt.as<int>() + (long long)frame * g.ncells_total + L.cell_base,
                              4 * (size_t)L.ncells, hipMemcpyDeviceToHost));
    std::vector<uint32_t> slots((size_t)g.slot_frame);
    ORB_HIP_TRY(hipMemcpy(slots.data(), h->d_slots.as<uint32_t>() + (long long)frame * g.slot_frame,
                          4 * (size_t)g.slot_frame, hipMemcpyDeviceToHost));
    int m = 0;
    for (int c = 0; c < L.ncells; c++) {
        const CellDev& cd = h->cells[L.cell_base + c];
        for (int j = 0; j < (cnt[c] & CELL_CNT_MASK); j++) {
            if (out && m < cap) out[m] = slots[cd.slot + j];
            m++;
        }
    }
    *n = m;
    return ORB_OK;
}

int orbx_debug_level_selected(const orbx_extractor* h, int frame, int level, uint32_t* out, int cap, int* n) {
    ORB_CHECK_ARG(h && n && h->last_frames > 0, "no extraction has run");
    ORB_CHECK_ARG(frame >= 0 && frame < h->last_frames && level >= 0 && level < h->geom.nlevels, "bad index");
    ORB_HIP_TRY(hipSetDevice(h->device));
    ORB_HIP_TRY(hipDeviceSynchronize());
    const Geom& g = h->geom;
    int c = 0;
    ORB_HIP_TRY(hipMemcpy(&c, h->d_selcnt.as<int>() + frame * g.nlevels + level, 4, hipMemcpyDeviceToHost));
    *n = c;
    if (out && c > 0)
        ORB_HIP_TRY(hipMemcpy(out, h->d_sel.as<uint32_t>() + (long long)frame * g.out_frame + g.lv[level].out_base,
                              4 * (size_t)std::min(c, cap), hipMemcpyDeviceToHost));
    return ORB_OK;
}

int orbx_debug_describe(orbx_extractor* h, const uint8_t* imgs, int n_frames, int rows, int cols, size_t step,
                        const int32_t* points, int n, orbx_keypoint* kps, uint8_t* desc) {
    ORB_CHECK_ARG(h && imgs && points && kps && desc, "null argument");
    ORB_CHECK_ARG(n_frames >= 1 && n_frames <= 65535 && n >= 1, "bad frame / point count");
    ORB_CHECK_ARG(rows > 0 && cols > 0 && step >= (size_t)cols, "frames must be non-empty CV_8U matrices");
    std::lock_guard<std::mutex> lk(h->mu);
    ORB_HIP_TRY(hipSetDevice(h->device));
    int rc = setup_geometry(h, rows, cols);
    if (rc) return rc;
    const Geom& g = h->geom;
    // the planted selection of one frame (level-major, plant order inside a level): every point inside
    // what FAST can return, so describe reads nothing Extract could not reach
    std::vector<uint32_t> sel1((size_t)g.out_frame, 0u);
    std::vector<int> cnt1((size_t)g.nlevels, 0);
    for (int i = 0; i < n; i++) {
        const int l = points[4 * i], x = points[4 * i + 1], y = points[4 * i + 2], s = points[4 * i + 3];
        ORB_CHECK_ARG(l >= 0 && l < g.nlevels, "planted point: level outside [0, nlevels)");
        const LevelDev& L = g.lv[l];
        ORB_CHECK_ARG(L.out_cap > 0, "planted point: the level takes no keypoints");
        ORB_CHECK_ARG(x >= 19 && x < L.w - 19 && y >= 19 && y < L.h - 19, "planted point outside [19, w - 19) x [19, h - 19)");
        ORB_CHECK_ARG(s >= 0 && s <= 255, "planted point: score outside 0..255");
        ORB_CHECK_ARG(cnt1[l] < L.out_cap, "more planted points on a level than its selection capacity");
        sel1[(size_t)L.out_base + cnt1[l]++] = (uint32_t)x | ((uint32_t)y << 12) | ((uint32_t)s << 24);
    }
    const int F = n_frames, kcap = max_keypoints(g);
    if ((rc = reserve_workspace(h, F))) return rc;
    if ((rc = h->d_img.reserve((size_t)F * rows * cols))) return rc;
    if ((rc = h->d_kps.reserve((size_t)F * kcap * sizeof(orbx_keypoint)))) return rc;
    if ((rc = h->d_desc.reserve((size_t)F * kcap * 32))) return rc;
    if ((rc = h->d_counts.reserve(std::max<size_t>(16, (size_t)F * 4)))) return rc;
    hipStream_t st = h->stream;
    const long long fstride = (long long)rows * cols;
    // frames are rows * step bytes apart: F * rows rows of one pitched copy (tight on the device, as orbx_extract)
    if (step == (size_t)cols)
        ORB_HIP_TRY(hipMemcpyAsync(h->d_img.ptr, imgs, (size_t)F * rows * cols, hipMemcpyHostToDevice, st));
    else
        ORB_HIP_TRY(hipMemcpy2DAsync(h->d_img.ptr, cols, imgs, step, cols, (size_t)F * rows, hipMemcpyHostToDevice, st));
    std::vector<uint32_t> sel((size_t)F * g.out_frame);
    std::vector<int> cnt((size_t)F * g.nlevels);
    for (int f = 0; f < F; f++) {
        std::copy(sel1.begin(), sel1.end(), sel.begin() + (size_t)f * g.out_frame);
        std::copy(cnt1.begin(), cnt1.end(), cnt.begin() + (size_t)f * g.nlevels);
    }
    ORB_HIP_TRY(hipMemcpyAsync(h->d_sel.ptr, sel.data(), sel.size() * 4, hipMemcpyHostToDevice, st));
    ORB_HIP_TRY(hipMemcpyAsync(h->d_selcnt.ptr, cnt.data(), cnt.size() * 4, hipMemcpyHostToDevice, st));
    h->last_in = h->d_img.as<uint8_t>();
    h->last_fstride = fstride;
    h->last_step = cols;
    h->last_frames = F;
    h->last_single = false;
    if ((rc = describe_grid_begin(h, st))) return rc;
    launch_chunk(h, 0, h->d_img.as<uint8_t>(), F, fstride, cols, h->d_kps.as<orbx_keypoint>(), h->d_desc.as<uint8_t>(),
                 h->d_counts.as<int32_t>(), kcap, st, nullptr, true);
    ORB_HIP_TRY(hipGetLastError());
    if ((rc = describe_grid_end(h, st))) return rc;
    for (int f = 0; f < F; f++) {   // the frame's first n rows: level-major, plant order
        ORB_HIP_TRY(hipMemcpyAsync(kps + (size_t)f * n, h->d_kps.as<orbx_keypoint>() + (size_t)f * kcap,
                                   (size_t)n * sizeof(orbx_keypoint), hipMemcpyDeviceToHost, st));
        ORB_HIP_TRY(hipMemcpyAsync(desc + (size_t)f * n * 32, h->d_desc.as<uint8_t>() + (size_t)f * kcap * 32, (size_t)n * 32,
                                   hipMemcpyDeviceToHost, st));
    }
    ORB_HIP_TRY(hipStreamSynchronize(st));
    return check_fault(h);
}

int orbx_profile_enable(orbx_extractor* h, int enable) {
    ORB_CHECK_ARG(h, "null extractor");
    std::lock_guard<std::mutex> lk(h->mu);
    h->prof = enable > 0 ? 0xf : (-enable) & 0xf;   // > 0: every stage; < 0: the stages of bitmask -enable

    return ORB_OK;
}

int orbx_pack_descriptors(const uint8_t* desc, int32_t cap, const int32_t* counts, const int32_t* incl,
                          int32_t n_frames, uint8_t* out, int32_t out_rows, void* stream) {
    ORB_CHECK_ARG(n_frames >= 0 && cap >= 0 && out_rows >= 0, "negative sizes");
    if (n_frames == 0 || out_rows == 0) return ORB_OK;
    ORB_CHECK_ARG(desc && counts && incl && out, "null argument");
    ORB_CHECK_ARG(((reinterpret_cast<uintptr_t>(desc) | reinterpret_cast<uintptr_t>(out)) & 15) == 0,
                  "desc / out must be 16-byte aligned");
    hipLaunchKernelGGL(orbamd::pack_rows_kernel, dim3((unsigned)n_frames), dim3(256), 0, (hipStream_t)stream,
                       reinterpret_cast<const uint4*>(desc), (int)cap, counts, incl, reinterpret_cast<uint4*>(out),
                       (int)out_rows);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

int orbx_profile_read(orbx_extractor* h, double* ms, int32_t* launches) {
    ORB_CHECK_ARG(h, "null extractor");
    std::lock_guard<std::mutex> lk(h->mu);
    ORB_HIP_TRY(hipSetDevice(h->device));
    for (int k = 0; k < 4; k++) {
        double tot = 0;
        for (auto& pr : h->prof_ev[k]) {
            ORB_HIP_TRY(hipEventSynchronize(pr.second));
            float t = 0;
            ORB_HIP_TRY(hipEventElapsedTime(&t, pr.first, pr.second));
            tot += t;
            h->ev_pool.push_back(pr.first);
            h->ev_pool.push_back(pr.second);
        }
        if (ms) ms[k] = tot;
        if (launches) launches[k] = (int32_t)h->prof_ev[k].size();
        h->prof_ev[k].clear();
    }
    return ORB_OK;
}

int orbx_debug_qt_sort(const int32_t* sizes, int n, int32_t* perm) {
    ORB_CHECK_ARG(n >= 0 && (n == 0 || (sizes && perm)), "bad argument");
    if (n == 0) return ORB_OK;
    std::vector<QtItem> h(n);
    for (int i = 0; i < n; i++) h[i] = QtItem{sizes[i], i};
    DevBuf d;
    int rc;
    if ((rc = d.reserve((size_t)n * sizeof(QtItem) + ((size_t)n * 8 + 16) * sizeof(int) + 64))) return rc;
    QtItem* items = d.as<QtItem>();
    int* scratch = reinterpret_cast<int*>(items + n);
    ORB_HIP_TRY(hipMemcpy(items, h.data(), n * sizeof(QtItem), hipMemcpyHostToDevice));
    // the kernel keeps items in global memory (same code path as LDS: generic pointers)
    hipLaunchKernelGGL(qt_sort_test_kernel, dim3(1), dim3(256), 0, 0, items, n, scratch);
    ORB_HIP_TRY(hipGetLastError());
    ORB_HIP_TRY(hipMemcpy(h.data(), items, n * sizeof(QtItem), hipMemcpyDeviceToHost));
    d.release();
    for (int i = 0; i < n; i++) perm[i] = h[i].node;
    return ORB_OK;
}

static void stereo_side(const orbx_extractor* h, StereoSide& s) {
    std::memset(&s, 0, sizeof(s));
    const Geom& g = h->geom;
    s.nlevels = g.nlevels;
    s.lvl0 = h->last_in;
    s.fstride0 = h->last_fstride;
    s.step0 = (int)h->last_step;
    s.pyr = h->d_pyr.as<uint8_t>();
    s.pyr_frame = g.pyr_frame_bytes;
    for (int l = 0; l < g.nlevels; l++) {
        s.off[l] = g.lv[l].off;
        s.stride[l] = g.lv[l].stride;
        s.rows[l] = g.lv[l].h;
        s.cols[l] = g.lv[l].w;
    }
}

// The argument check both stereo entry points share (same_cap: the sides' output capacities agree, where
// the entry point depends on it).
static int stereo_check_pair(const orbx_extractor* left, const orbx_extractor* right, bool same_cap) {
    ORB_CHECK_ARG(left->g_rows == right->g_rows && left->g_cols == right->g_cols &&
                      left->p.nlevels == right->p.nlevels && left->p.scaleFactor == right->p.scaleFactor && same_cap,
                  "left / right extractors differ in image size or pyramid parameters");
    ORB_CHECK_ARG(left->p.nlevels <= ST_MAX_LEVELS, "too many levels");
    return ORB_OK;
}

// Both sides' pyramids, the scale tables and the left handle's stereo scratch for n_frames frame pairs of
// cap slots each.
static int stereo_setup(orbx_extractor* left, const orbx_extractor* right, float bf, float baseline, int n_frames, int cap,
                        StereoSide& L, StereoSide& R, StereoParams& sp) {
    stereo_side(left, L);
    stereo_side(right, R);
    std::memset(&sp, 0, sizeof(sp));
    for (int l = 0; l < left->p.nlevels; l++) {
        sp.scale[l] = left->scale[l];
        sp.inv_scale[l] = left->inv_scale[l];
    }
    sp.bf = bf;
    sp.baseline = baseline;
    const size_t ints = stereo_scratch_ints(n_frames, cap, L.rows[0], stereo_row_span(sp, left->p.nlevels));
    return left->d_stereo_sad.reserve(ints * sizeof(int32_t));
}

int orbx_stereo_matches_batch_device(orbx_extractor* left, orbx_extractor* right, int n_frames,
                                     const orbx_keypoint* d_kps_l, const uint8_t* d_desc_l,
                                     const int32_t* d_counts_l, const orbx_keypoint* d_kps_r,
                                     const uint8_t* d_desc_r, const int32_t* d_counts_r, int cap, float bf,
                                     float baseline, float* d_uright, float* d_depth, void* stream) {
    ORB_CHECK_ARG(left && right && d_kps_l && d_desc_l && d_counts_l && d_kps_r && d_desc_r && d_counts_r && d_uright &&
                      d_depth, "null argument");
    ORB_CHECK_ARG(n_frames > 0 && cap > 0, "bad sizes");
    ORB_CHECK_ARG(left->last_in && right->last_in && left->last_frames >= n_frames && right->last_frames >= n_frames,
                  "both extractors need a batch of >= n_frames frames first");
    if (int rc = stereo_check_pair(left, right, true)) return rc;
    std::lock_guard<std::mutex> lk(left->mu);
    ORB_HIP_TRY(hipSetDevice(left->device));
    int rc;
    StereoSide L, R;
    StereoParams sp;
    if ((rc = stereo_setup(left, right, bf, baseline, n_frames, cap, L, R, sp))) return rc;
    return launch_stereo(L, R, sp, n_frames, d_kps_l, d_desc_l, d_counts_l, 0, d_kps_r, d_desc_r, d_counts_r, 0, cap,
                         d_uright, d_depth, left->d_stereo_sad.as<int32_t>(), (hipStream_t)stream);
}

int orbx_stereo_matches_last(orbx_extractor* left, orbx_extractor* right, float bf, float baseline, float* uright,
                             float* depth, int n_left) {
    ORB_CHECK_ARG(left && right && left != right && uright && depth, "null argument");
    ORB_CHECK_ARG(left->last_single && right->last_single, "both extractors need a single-frame orbx_extract first");
    if (int rc = stereo_check_pair(left, right, left->last_kcap == right->last_kcap)) return rc;
    std::unique_lock<std::mutex> la(left->mu, std::defer_lock), lb(right->mu, std::defer_lock);
    std::lock(la, lb);
    ORB_HIP_TRY(hipSetDevice(left->device));
    const int cap = left->last_kcap;
    int32_t nl = 0;
    ORB_HIP_TRY(hipMemcpy(&nl, left->d_counts.ptr, 4, hipMemcpyDeviceToHost));
    ORB_CHECK_ARG(n_left == nl, "n_left differs from the left extractor's keypoint count");
    if (nl == 0) return ORB_OK;
    int rc;
    StereoSide L, R;
    StereoParams sp;
    if ((rc = stereo_setup(left, right, bf, baseline, 1, cap, L, R, sp))) return rc;
    if ((rc = left->d_stereo_out.reserve(2 * (size_t)cap * sizeof(float)))) return rc;
    float* d_u = left->d_stereo_out.as<float>();
    float* d_d = d_u + cap;
    hipStream_t st = left->stream;
    if ((rc = launch_stereo(L, R, sp, 1, left->d_kps.as<orbx_keypoint>(), left->d_desc.as<uint8_t>(),
                            left->d_counts.as<int32_t>(), 0, right->d_kps.as<orbx_keypoint>(), right->d_desc.as<uint8_t>(),
                            right->d_counts.as<int32_t>(), 0, cap, d_u, d_d, left->d_stereo_sad.as<int32_t>(), st)))
        return rc;
    ORB_HIP_TRY(hipMemcpyAsync(uright, d_u, (size_t)nl * sizeof(float), hipMemcpyDeviceToHost, st));
    ORB_HIP_TRY(hipMemcpyAsync(depth, d_d, (size_t)nl * sizeof(float), hipMemcpyDeviceToHost, st));
    ORB_HIP_TRY(hipStreamSynchronize(st));
    return ORB_OK;
}

int orbx_debug_fast_stamps(unsigned long long* out, int n_words) {
#ifdef ORB_FAST_STAMPS
    ORB_CHECK_ARG(out && n_words > 0 && n_words <= FAST_NSAMP * 8, "bad stamp buffer");
    ORB_HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_fast_stamps), (size_t)n_words * 8));
    return ORB_OK;
#else
    (void)out;
    (void)n_words;
    set_error("built without ORB_FAST_STAMPS");
    return ORB_EINVAL;
#endif
}

int orbx_debug_qt_stamps(unsigned long long* out) {
#if defined(ORB_DESC_STAMPS)
    ORB_HIP_TRY(hipDeviceSynchronize());
    ORB_HIP_TRY(hipMemcpyFromSymbol(out + 64, HIP_SYMBOL(g_desc_stamps), 1024 * 8 * 8));
    return ORB_OK;
#elif defined(ORB_QT_STAMPS)
    ORB_HIP_TRY(hipDeviceSynchronize());
    ORB_HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_qt_stamps), 64 * 8));
    ORB_HIP_TRY(hipMemcpyFromSymbol(out + 64, HIP_SYMBOL(g_qt_wg), 4096 * 2 * 8));
    return ORB_OK;
#else
    (void)out;
    set_error("built without ORB_QT_STAMPS");
    return ORB_EINVAL;
#endif
}

}  // extern "C"
