// orbm.hip — the ORBmatcher Hamming searches on gfx950: the C entries.  The
// kernels and their launch sequences live in one header per search, included below in dependency order:
//   orbm_mfma.h      the matrix-core matcher: the i8 / FP4 operand expansions, the LDS layouts (Top2Lds,
//                    TriMmLds), the running top-2 (update, carry, row merge and result write),
//                    hamming_top2_mfma_kernel / hamming_top2_fp4_kernel, launch_top2 and the ORBM_FP4 /
//                    ORBM_TRI_MM / ORBM_TRI_SPLIT switches
//   orbm_orient.h    CheckOrientation on a query-indexed match list (check_orientation_kernel)
//   orbm_tri.h       SearchForTriangulation: the gates, the five kernels (tri_mm_kernel on the FP4 tile
//                    stream) and launch_triangulation with the path choice
//   orbm_bow.h       SearchByBoW, both forms (search_by_bow_kernel and its launch)
//   orbm_distinct.h  MapPoint::ComputeDistinctiveDescriptors
#include <cstring>
#include <vector>

#include "common.h"
#include "qt_sort.h"
#include "orbm_mfma.h"
#include "orbm_orient.h"
#include "orbm_tri.h"
#include "orbm_bow.h"
#include "orbm_distinct.h"

using namespace orbamd;

namespace {
struct HostScratch {
    DevBuf a, b, o1, o2, o3, o4;
};
thread_local HostScratch g_scratch;
}  // namespace

extern "C" {

int orbm_descriptor_distance(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int i = 0; i < 8; i++) {
        uint32_t x, y;
        std::memcpy(&x, a + 4 * i, 4);
        std::memcpy(&y, b + 4 * i, 4);
        d += __builtin_popcount(x ^ y);
    }
    return d;
}

int orbm_hamming_top2_device(const uint8_t* d_A, int nA, const uint8_t* d_B, int nB, int32_t* d_best_idx,
                             int32_t* d_best, int32_t* d_second, void* stream) {
    ORB_CHECK_ARG(nA >= 0 && nB >= 0 && (nA == 0 || d_A) && (nB == 0 || d_B), "bad matcher arguments");
    if (nA == 0) return ORB_OK;
    launch_top2(d_A, nullptr, nA, nA, d_B, nullptr, nB, std::max(nB, 1), nullptr, 1, 0.6f, 50, d_best_idx, d_best,
                d_second, nullptr, (hipStream_t)stream);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

int orbm_bf_match_batch_device(const uint8_t* d_A, const int32_t* d_nA, int strideA, const uint8_t* d_B,
                               const int32_t* d_nB, int strideB, const int32_t* d_pair_b, int n_pairs, float nnratio,
                               int th_low, int32_t* d_best_idx, int32_t* d_best, int32_t* d_second,
                               int32_t* d_match, void* stream) {
    ORB_CHECK_ARG(d_A && d_B && d_nA && d_nB && n_pairs >= 0 && strideA > 0 && strideB > 0, "bad matcher arguments");
    if (n_pairs == 0) return ORB_OK;
    ORB_CHECK_ARG(n_pairs <= 65535, "too many pairs in one launch");
    launch_top2(d_A, d_nA, 0, strideA, d_B, d_nB, 0, strideB, d_pair_b, n_pairs, nnratio, th_low, d_best_idx, d_best,
                d_second, d_match, (hipStream_t)stream);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

int orbm_bf_match(const uint8_t* A, int nA, const uint8_t* B, int nB, float nnratio, int th_low, int32_t* best_idx,
                  int32_t* best, int32_t* second, int32_t* match) {
    ORB_CHECK_ARG(nA >= 0 && nB >= 0, "negative sizes");
    if (nA == 0) return ORB_OK;
    ORB_CHECK_ARG(A && (nB == 0 || B), "null descriptors");
    HostScratch& s = g_scratch;
    int rc;
    if ((rc = s.a.reserve((size_t)nA * 32))) return rc;
    if ((rc = s.b.reserve((size_t)std::max(nB, 1) * 32))) return rc;
    if ((rc = s.o1.reserve((size_t)nA * 16))) return rc;
    int32_t* o = s.o1.as<int32_t>();
    ORB_HIP_TRY(hipMemcpy(s.a.ptr, A, (size_t)nA * 32, hipMemcpyHostToDevice));
    if (nB) ORB_HIP_TRY(hipMemcpy(s.b.ptr, B, (size_t)nB * 32, hipMemcpyHostToDevice));
    launch_top2(s.a.as<uint8_t>(), nullptr, nA, nA, s.b.as<uint8_t>(), nullptr, nB, std::max(nB, 1), nullptr, 1, nnratio,
                th_low, o, o + nA, o + 2 * nA, o + 3 * nA, (hipStream_t)0);
    ORB_HIP_TRY(hipGetLastError());
    std::vector<int32_t> h((size_t)nA * 4);
    ORB_HIP_TRY(hipMemcpy(h.data(), o, (size_t)nA * 16, hipMemcpyDeviceToHost));
    for (int i = 0; i < nA; i++) {
        if (best_idx) best_idx[i] = h[i];
        if (best) best[i] = h[nA + i];
        if (second) second[i] = h[2 * nA + i];
        if (match) match[i] = h[3 * nA + i];
    }
    return ORB_OK;
}

int orbm_check_orientation_batch_device(const float* d_angA, int kstrideA, int capA, const int32_t* d_nA,
                                        const float* d_angB, int kstrideB, int capB, const int32_t* d_pair_b,
                                        int n_pairs, int32_t* d_match, int strideM, int32_t* d_nmatches,
                                        void* stream) {
    ORB_CHECK_ARG(n_pairs >= 0 && kstrideA > 0 && kstrideB > 0 && capA > 0 && capB > 0 && strideM > 0,
                  "bad CheckOrientation arguments");
    if (n_pairs == 0) return ORB_OK;
    ORB_CHECK_ARG(d_angA && d_angB && d_nA && d_match, "null CheckOrientation argument");
    hipLaunchKernelGGL(check_orientation_kernel, dim3((unsigned)n_pairs), dim3(256), 0, (hipStream_t)stream, d_angA,
                       kstrideA, capA, d_nA, d_angB, kstrideB, capB, d_pair_b, d_match, strideM, d_nmatches,
                       (const int32_t*)nullptr);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

int orbm_check_orientation(const float* angA, int nA, const float* angB, int nB, int32_t* match, int32_t* nmatches) {
    ORB_CHECK_ARG(nA >= 0 && nB >= 0 && match && (nA == 0 || angA), "bad CheckOrientation arguments");
    for (int i = 0; i < nA; i++) {
        ORB_CHECK_ARG(match[i] < nB && match[i] >= -1, "match index out of range");
        ORB_CHECK_ARG(!(match[i] >= 0) || (angA[i] >= 0.f && angA[i] < 360.f && angB[match[i]] >= 0.f &&
                                           angB[match[i]] < 360.f),
                      "keypoint angle outside [0, 360) (CV_Assert in CheckOrientation)");
    }
    if (nmatches) *nmatches = 0;
    if (nA == 0) return ORB_OK;
    HostScratch& s = g_scratch;
    int rc;
    const size_t offB = align_up((size_t)nA * 4, 256);
    if ((rc = s.o3.reserve(offB + (size_t)std::max(nB, 1) * 4))) return rc;
    if ((rc = s.o4.reserve((size_t)nA * 4 + 8))) return rc;   // matches | nA | match count
    float* dA = s.o3.as<float>();
    float* dB = reinterpret_cast<float*>(s.o3.as<char>() + offB);
    int32_t* dM = s.o4.as<int32_t>();
    ORB_HIP_TRY(hipMemcpy(dA, angA, (size_t)nA * 4, hipMemcpyHostToDevice));
    if (nB) ORB_HIP_TRY(hipMemcpy(dB, angB, (size_t)nB * 4, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(dM, match, (size_t)nA * 4, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(dM + nA, &nA, 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(check_orientation_kernel, dim3(1), dim3(256), 0, (hipStream_t)0, dA, 1, nA, dM + nA, dB, 1,
                       std::max(nB, 1), nullptr, dM, nA, dM + nA + 1, (const int32_t*)nullptr);
    ORB_HIP_TRY(hipGetLastError());
    ORB_HIP_TRY(hipMemcpy(match, dM, (size_t)nA * 4, hipMemcpyDeviceToHost));
    int32_t nm = 0;
    ORB_HIP_TRY(hipMemcpy(&nm, dM + nA + 1, 4, hipMemcpyDeviceToHost));
    if (nmatches) *nmatches = nm;
    return ORB_OK;
}

int orbm_search_by_bow_batch_device(const orbm_bow_batch* b, int32_t* d_match, int32_t* d_nmatches, void* stream) {
    return search_by_bow(b, 0, d_match, d_nmatches, stream);
}

int orbm_search_by_bow_kf_batch_device(const orbm_bow_batch* b, int32_t* d_match12, int32_t* d_nmatches, void* stream) {
    return search_by_bow(b, 1, d_match12, d_nmatches, stream);
}

int orbm_search_for_triangulation_batch_device(const orbm_tri_batch* b, int32_t* d_match12, int32_t* d_nmatches,
                                               void* stream) {
    ORB_CHECK_ARG(b && d_match12 && d_nmatches, "null argument");
    ORB_CHECK_ARG(b->n_pairs >= 0 && b->cap1 > 0 && b->cap2 > 0, "bad pair count / capacities");
    ORB_CHECK_ARG(b->n_levels > 0 && b->n_levels <= ORBM_TRI_MAX_LEVELS && b->scale_factors2 && b->sigma2,
                  "n_levels must be 1..ORBM_TRI_MAX_LEVELS with host scale / sigma2 tables");
    if (b->n_pairs == 0) return ORB_OK;
    ORB_CHECK_ARG(b->kps1 && b->desc1 && b->counts1 && b->kps2 && b->desc2 && b->counts2 && b->F12 && b->ep2,
                  "null keyframe arrays");
    const bool fv1 = b->fv_node1 || b->fv_off1 || b->fv_idx1 || b->fv_n_nodes1;
    const bool fv2 = b->fv_node2 || b->fv_off2 || b->fv_idx2 || b->fv_n_nodes2;
    ORB_CHECK_ARG(fv1 == fv2, "give FeatureVectors for both keyframe sets or for neither");
    if (fv1)
        ORB_CHECK_ARG(b->fv_node1 && b->fv_off1 && b->fv_idx1 && b->fv_n_nodes1 && b->fv_node2 && b->fv_off2 &&
                          b->fv_idx2 && b->fv_n_nodes2 && b->fv_cap1 > 0 && b->fv_cap2 > 0,
                      "incomplete FeatureVector arrays");
    ORB_CHECK_ARG(b->n_pairs <= 65535, "too many pairs in one launch");
    ORB_CHECK_ARG(fv1 || b->cap2 <= 65535, "cap2 must be <= 65535 for the all-pairs search");
    TriTables t{};
    for (int l = 0; l < b->n_levels; l++) {
        t.scale2[l] = b->scale_factors2[l];
        t.sigma2[l] = b->sigma2[l];
    }
    t.n_levels = b->n_levels;
    TriArgs a{b->kps1, b->desc1, b->counts1, b->uright1, b->has_mappoint1, b->kps2, b->desc2, b->counts2, b->uright2,
              b->has_mappoint2, b->frame1, b->frame2, b->F12, b->ep2, b->fv_node1, b->fv_off1, b->fv_idx1,
              b->fv_n_nodes1, b->fv_node2, b->fv_off2, b->fv_idx2, b->fv_n_nodes2, b->cap1, b->cap2, b->fv_cap1,
              b->fv_cap2, b->only_stereo ? 1 : 0, d_match12, d_nmatches};
    return launch_triangulation(a, t, fv1, b->n_pairs, (hipStream_t)stream);
}

int orbm_search_for_triangulation(const orbm_tri_frame* kf1, const orbm_tri_frame* kf2, const float* F12,
                                  const float* ep2, const float* scale2, const float* sigma2, int n_levels,
                                  int only_stereo, int32_t* match12, int32_t* nmatches) {
    ORB_CHECK_ARG(kf1 && kf2 && F12 && ep2 && scale2 && sigma2 && match12 && n_levels > 0, "null argument");
    for (int i = 0; i < kf1->n; i++) match12[i] = -1;
    if (nmatches) *nmatches = 0;
    // FeatureVectorIterator (:406-450): walk the two ascending node lists; queries are the
    // kf1 features of shared nodes without a MapPoint (and stereo when onlyStereo).
    std::vector<TriQuery> qs;
    int a = 0, b = 0;
    while (a < kf1->n_nodes && b < kf2->n_nodes) {
        if (kf1->node_id[a] == kf2->node_id[b]) {
            for (int u = kf1->node_off[a]; u < kf1->node_off[a + 1]; u++) {
                const int i1 = kf1->indices[u];
                ORB_CHECK_ARG(i1 >= 0 && i1 < kf1->n, "kf1 feature index out of range");
                if (kf1->has_mappoint[i1]) continue;
                if (only_stereo && !(kf1->uright[i1] >= 0)) continue;
                qs.push_back(TriQuery{i1, kf2->node_off[b], kf2->node_off[b + 1]});
            }
            a++;
            b++;
        } else if (kf1->node_id[a] < kf2->node_id[b]) {
            a++;
        } else {
            b++;
        }
    }
    for (int o = 0; o < kf2->n; o++) ORB_CHECK_ARG(kf2->octave[o] >= 0 && kf2->octave[o] < n_levels, "bad octave");
    if (qs.empty()) return ORB_OK;
    const int n1 = kf1->n, n2 = kf2->n, ni2 = kf2->node_off[kf2->n_nodes];
    // one device slab: queries | kf1 xy,ur,desc | kf2 xy,oct,ur,mp,desc,idx | F | scale | sigma | out
    std::vector<size_t> sz = {qs.size() * sizeof(TriQuery), (size_t)n1 * 8, (size_t)n1 * 4, (size_t)n1 * 32,
                              (size_t)n2 * 8, (size_t)n2 * 4, (size_t)n2 * 4, (size_t)n2, (size_t)n2 * 32,
                              (size_t)std::max(ni2, 1) * 4, 36, (size_t)n_levels * 4, (size_t)n_levels * 4,
                              (size_t)n1 * 4};
    std::vector<size_t> off(sz.size());
    size_t tot = 0;
    for (size_t i = 0; i < sz.size(); i++) { off[i] = tot; tot += align_up(std::max<size_t>(sz[i], 1), 256); }
    DevBuf& s = g_scratch.o2;
    int rc;
    if ((rc = s.reserve(tot))) return rc;
    char* base = s.as<char>();
    const void* src[] = {qs.data(), kf1->kp_xy, kf1->uright, kf1->desc, kf2->kp_xy, kf2->octave, kf2->uright,
                         kf2->has_mappoint, kf2->desc, kf2->indices, F12, scale2, sigma2};
    for (int i = 0; i < 13; i++)
        if (sz[i]) ORB_HIP_TRY(hipMemcpy(base + off[i], src[i], sz[i], hipMemcpyHostToDevice));
    const int nq = (int)qs.size();
    ORB_HIP_TRY(hipMemset(base + off[13], 0xff, sz[13]));   // -1: no match
    hipLaunchKernelGGL(triangulation_kernel, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, (hipStream_t)0,
                       (const TriQuery*)(base + off[0]), nq, (const float*)(base + off[1]),
                       (const uint8_t*)(base + off[3]), (const float*)(base + off[4]),
                       (const int32_t*)(base + off[5]), (const float*)(base + off[6]),
                       (const uint8_t*)(base + off[7]), (const uint8_t*)(base + off[8]),
                       (const int32_t*)(base + off[9]), (const float*)(base + off[2]), (const float*)(base + off[10]),
                       ep2[0], ep2[1], (const float*)(base + off[11]), (const float*)(base + off[12]), only_stereo,
                       (int32_t*)(base + off[13]));
    ORB_HIP_TRY(hipGetLastError());
    ORB_HIP_TRY(hipMemcpy(match12, base + off[13], (size_t)n1 * 4, hipMemcpyDeviceToHost));
    int nm = 0;
    for (int i = 0; i < n1; i++) nm += match12[i] >= 0;
    if (nmatches) *nmatches = nm;
    return ORB_OK;
}

int orbm_distinctive_descriptors_device(const uint8_t* desc, const int32_t* begin, int32_t n_points, int32_t* best,
                                        int32_t* best_median, uint8_t* out_desc, void* stream) {
    ORB_CHECK_ARG(n_points >= 0, "negative sizes");
    if (n_points == 0) return ORB_OK;
    ORB_CHECK_ARG(desc && begin && best, "null argument");
    return launch_distinct(DistinctArgs{desc, begin, n_points, best, best_median, out_desc}, (hipStream_t)stream);
}

int orbm_distinctive_descriptors(const uint8_t* desc, const int32_t* begin, int32_t n_points, int32_t* best,
                                 int32_t* best_median, uint8_t* out_desc, int device) {
    ORB_CHECK_ARG(n_points >= 0, "negative sizes");
    if (n_points == 0) return ORB_OK;
    ORB_CHECK_ARG(begin && best, "null argument");
    ORB_CHECK_ARG(begin[0] == 0, "begin must start at 0");
    for (int p = 0; p < n_points; p++) {
        ORB_CHECK_ARG(begin[p + 1] >= begin[p], "offsets must be non-decreasing");
        ORB_CHECK_ARG(begin[p + 1] - begin[p] <= ORBM_DISTINCT_MAX_OBS, "map point has more than ORBM_DISTINCT_MAX_OBS observations");
    }
    const size_t total = (size_t)begin[n_points], P = (size_t)n_points;
    ORB_CHECK_ARG(total == 0 || desc, "null descriptors");
    ORB_HIP_TRY(hipSetDevice(device));
    HostScratch& s = g_scratch;
    int rc;
    const size_t o_bg = align_up(std::max<size_t>(total, 1) * 32, 256), o_bi = o_bg + align_up((P + 1) * 4, 256),
                 o_bm = o_bi + align_up(P * 4, 256), o_od = o_bm + align_up(P * 4, 256);
    if ((rc = s.a.reserve(o_od + P * 32))) return rc;
    char* d = s.a.as<char>();
    if (total) ORB_HIP_TRY(hipMemcpy(d, desc, total * 32, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(d + o_bg, begin, (P + 1) * 4, hipMemcpyHostToDevice));
    if (out_desc) ORB_HIP_TRY(hipMemcpy(d + o_od, out_desc, P * 32, hipMemcpyHostToDevice));   // empty points keep theirs
    if ((rc = orbm_distinctive_descriptors_device((const uint8_t*)d, (const int32_t*)(d + o_bg), n_points, (int32_t*)(d + o_bi),
                                                  (int32_t*)(d + o_bm), out_desc ? (uint8_t*)(d + o_od) : nullptr, nullptr)))
        return rc;
    ORB_HIP_TRY(hipMemcpy(best, d + o_bi, P * 4, hipMemcpyDeviceToHost));
    if (best_median) ORB_HIP_TRY(hipMemcpy(best_median, d + o_bm, P * 4, hipMemcpyDeviceToHost));
    if (out_desc) ORB_HIP_TRY(hipMemcpy(out_desc, d + o_od, P * 32, hipMemcpyDeviceToHost));
    return ORB_OK;
}

}  // extern "C"
