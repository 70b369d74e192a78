/*
 * orbslam2_amd.h — C-ABI of the MI355X (gfx950) ORB front end + local BA.
 *
 * This is the drop-in boundary for the hot path of tiantianxuabc/ORB_SLAM2_Refactored
 * (SURVEY.md §8b).  Every entry point cites the reference interface it replaces.
 * Plain pointers and sizes only; no torch / OpenCV / Eigen types cross it.
 *
 *   status codes: 0 = ok, < 0 = error (orb_last_error() has a thread-local message)
 *   host pointers  : functions without the _device suffix take host memory and are
 *                    synchronous (the reference's calling convention).
 *   device pointers: *_device functions take HBM pointers and a hipStream_t (void*);
 *                    they only enqueue work (no host sync) unless stated.
 */
#ifndef ORBSLAM2_AMD_H
#define ORBSLAM2_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORB_OK          0
#define ORB_EINVAL     -1   /* bad argument (the reference throws cv::Exception via CV_Assert) */
#define ORB_EHIP       -2   /* HIP runtime error */
#define ORB_ENOMEM     -3
#define ORB_ECAP       -4   /* caller's output capacity too small */
#define ORB_EINTERNAL  -5   /* a device-side capacity / consistency check failed */

/* ------------------------------------------------------------------------------------------
 * Extractor.  Replaces ORB_SLAM2::ORBextractor (include/ORBextractor.h:35-81).
 * ---------------------------------------------------------------------------------------- */

/* == ORBextractor::Parameters (include/ORBextractor.h:39-47, defaults src/ORBextractor.cc:830-833) */
typedef struct orbx_params {
    int32_t nfeatures;    /* 2000 */
    float   scaleFactor;  /* 1.2f */
    int32_t nlevels;      /* 8 */
    int32_t iniThFAST;    /* 20 */
    int32_t minThFAST;    /* 7 */
} orbx_params;

/* Byte-compatible with cv::KeyPoint (28 B): pt.x, pt.y, size, angle, response, octave, class_id. */
typedef struct orbx_keypoint {
    float   x, y, size, angle, response;
    int32_t octave, class_id;
} orbx_keypoint;

typedef struct orbx_extractor orbx_extractor;

/* ORBextractor(const Parameters&) + Init() (src/ORBextractor.cc:695-741).  device = HIP ordinal. */
int orbx_create(const orbx_params* params, int device, orbx_extractor** out);
int orbx_destroy(orbx_extractor* h);

/* GetLevels/GetScaleFactors/GetInverseScaleFactors/GetScaleSigmaSquares/
 * GetInverseScaleSigmaSquares (src/ORBextractor.cc:822-827) plus the per-level feature quota
 * (ComputeNumFeaturesPerScale, :472-487).  Each array has nlevels entries; any may be NULL. */
int orbx_scale_tables(const orbx_extractor* h, float* scale, float* inv_scale, float* sigma2,
                      float* inv_sigma2, int32_t* features_per_level);

/* OpenCV-build switches.  Two results of the reference depend on how its OpenCV / C++ headers were
 * built, not on its own source; each is a switch here (default in brackets), restated identically by
 * the CPU oracle (oracle_set_compat).  INTEGRATION.md §1 says how to pick them for a given build.
 *   trig_mode   ComputeOrbDescriptor's `cos(angle)` / `sin(angle)` on a float (src/ORBextractor.cc:107):
 *               [0] ::cos(double) / ::sin(double), the overload visible without `using namespace std`;
 *               1 std::cos(float) / std::sin(float) = glibc cosf / sinf (a `using namespace std`, or a
 *               libstdc++ <math.h> wrapper, before :107).
 *   resize_simd tail mode V of cv::resize INTER_LINEAR 8U's vertical pass (src/ORBextractor.cc:468).
 *               VResizeLinearVec_32s8u rounds via ((S >> 4) * b) >> 16, and OpenCV's uchar
 *               specialisation of VResizeLinear repeats that rounding in its unrolled and scalar tails
 *               [ext, recalled], so [0] (the vector rounding on every column) is every build's result.
 *               8 / 16 / 32 / 64: a FixedPtCast tail (S0*b0 + S1*b1 + 2^21) >> 22 after a V-byte vector
 *               loop; 1: FixedPtCast everywhere.  These are sensitivity switches (parity unpinned).
 * -1 keeps a switch.  Environment defaults at orbx_create: ORBX_TRIG=double|float, ORBX_RESIZE_TAIL=V. */
int orbx_set_opencv_compat(orbx_extractor* h, int trig_mode, int resize_simd);
int orbx_get_opencv_compat(const orbx_extractor* h, int* trig_mode, int* resize_simd);

/* Upper bound on keypoints Extract can return for an image of rows x cols (per-level
 * quadtree output <= max(quota, 4*roots) + 3). */
int orbx_max_keypoints(const orbx_extractor* h, int rows, int cols, int32_t* cap);

/* void ORBextractor::Extract(const cv::Mat& image, KeyPoints& keypoints, cv::Mat& descriptors)
 * (include/ORBextractor.h:55, src/ORBextractor.cc:743-820).  Host memory, synchronous.
 * img: CV_8U rows x cols, row stride `step` bytes.  kps: cap entries; desc: cap x 32 bytes.
 * On return *n = number of keypoints.  Reference quirk kept: when the image yields no keypoint
 * at all *n = 0 and kps/desc are NOT written (Extract returns before keypoints.clear(), :778-782).
 * Returns ORB_ECAP (and *n = required count) if cap is too small. */
int orbx_extract(orbx_extractor* h, const uint8_t* img, int rows, int cols, size_t step,
                 orbx_keypoint* kps, uint8_t* desc, int cap, int* n);

/* GetImagePyramid() (src/ORBextractor.cc:828): copy level `level` of the last extracted image
 * (frame 0 of the last batch) to host memory dst (row stride dst_step; NULL dst = query only). */
int orbx_pyramid_level(const orbx_extractor* h, int level, uint8_t* dst, size_t dst_step,
                       int* rows, int* cols);

/* Batched, HBM-resident Extract over n_frames independent frames of identical size.
 * d_imgs: frame f at d_imgs + f*frame_stride, rows of `step` bytes.
 * Outputs per frame f: d_kps[f*cap .. ], d_desc[(f*cap)*32 .. ], d_counts[f].
 * Keypoint/descriptor order per frame is the reference's (level-major, quadtree list order).
 * Enqueue only (no host sync) on `stream` (a hipStream_t; NULL = the default stream, ordered like
 * any other HIP work on it).  cap must be >= orbx_max_keypoints(). */
int orbx_extract_batch_device(orbx_extractor* h, const uint8_t* d_imgs, int n_frames, int rows,
                              int cols, size_t frame_stride, size_t step, orbx_keypoint* d_kps,
                              uint8_t* d_desc, int32_t* d_counts, int cap, void* stream);

/* Device-side capacity checks of the batched path.  Every kernel of an extraction ORs a fault bit
 * into the handle's fault word when a capacity bound is violated (1 quadtree node array, 2 keypoint
 * outside the root nodes = the reference's CV_Assert :569, 4 FAST cell slot, 8 per-level output,
 * 16 a kernel launched with a block size it is not written for: it exits before touching memory);
 * the batch is then truncated, never written out of bounds.  The word is sticky across batches
 * until read.  orbx_batch_status waits for `stream`, returns the mask in *fault_mask, clears it and
 * returns ORB_EINTERNAL when it was non-zero (the single-frame orbx_extract checks it itself).
 * orbx_fault_word_device returns the word's device address so a pipeline can copy it
 * asynchronously (e.g. into pinned memory) instead of synchronising. */
int orbx_batch_status(orbx_extractor* h, void* stream, uint32_t* fault_mask);
int orbx_fault_word_device(orbx_extractor* h, uint32_t** d_fault);

/* Device pointer to the batch's pyramid (frame f, level s) for downstream consumers
 * (ComputeStereoMatches reads GetImagePyramid(), ORBmatcher.cc:165-166). */
int orbx_pyramid_device(const orbx_extractor* h, int frame, int level, const uint8_t** ptr,
                        int* rows, int* cols, size_t* step);

/* ------------------------------------------------------------------------------------------
 * Matcher.  Replaces the Hamming kernels of ORB_SLAM2::ORBmatcher (src/ORBmatcher.cc).
 * ---------------------------------------------------------------------------------------- */

/* static int ORBmatcher::DescriptorDistance(const cv::Mat&, const cv::Mat&)
 * (include/ORBmatcher.h:54, src/ORBmatcher.cc:1449-1457).  Two 32-byte rows. */
int orbm_descriptor_distance(const uint8_t* a, const uint8_t* b);

/* Brute-force best / second-best Hamming search with the reference's loop semantics
 * (SearchByBoW inner loop, src/ORBmatcher.cc:477-498): for each query row i of A scan B in
 * ascending j; best starts at 256 / idx -1, strict '<' updates (lowest j wins ties,
 * second = 2nd order statistic).  Device pointers, enqueue only. */
int orbm_hamming_top2_device(const uint8_t* d_A, int nA, const uint8_t* d_B, int nB,
                             int32_t* d_best_idx, int32_t* d_best, int32_t* d_second, void* stream);

/* Batched pairs: pair p matches A_p (rows d_A + p*strideA*32, count d_nA[p]) against
 * B_q (d_B + q*strideB*32, count d_nB[q]) with q = d_pair_b ? d_pair_b[p] : p (so a batch of
 * frames can be matched against its own predecessors without a copy).  Outputs at p*strideA.
 * Also applies the acceptance test of :500 when d_match != NULL: match = best_idx if
 * best <= th_low and (float)best < nnratio * (float)second, else -1. */
int orbm_bf_match_batch_device(const uint8_t* d_A, const int32_t* d_nA, int strideA,
                               const uint8_t* d_B, const int32_t* d_nB, int strideB,
                               const int32_t* d_pair_b, int n_pairs, float nnratio, int th_low,
                               int32_t* d_best_idx, int32_t* d_best, int32_t* d_second,
                               int32_t* d_match, void* stream);

/* Host-memory convenience form of the two above (synchronous). */
int orbm_bf_match(const uint8_t* A, int nA, const uint8_t* B, int nB, float nnratio, int th_low,
                  int32_t* best_idx, int32_t* best, int32_t* second, int32_t* match);

/* CheckOrientation (src/ORBmatcher.cc:249-309) on a query-indexed match result, applied as
 * SearchForInitialization applies it (:676-686): for every accepted query i (match[i] = j >= 0, in
 * ascending i) the rotation bin is cvRound((angleB[j] - angleA[i] (+360 if < 0)) / 30), 30 bins
 * (bin 30 -> 0); the bins are sorted by size with std::sort's unstable order (libstdc++), the top
 * 1-3 are kept (a 2nd / 3rd bin below 10 % of the largest ends the kept set, :293-298) and every
 * other match is reset to -1.  *nmatches = matches kept.  ORBmatcher(nnratio, checkOri=true)
 * applies it after the brute-force search.  Angles are cv::KeyPoint::angle in [0, 360)
 * (ORB_EINVAL otherwise; the reference CV_Asserts the bin).  Host memory, synchronous. */
int orbm_check_orientation(const float* angleA, int nA, const float* angleB, int nB, int32_t* match,
                           int32_t* nmatches);

/* Batched device form on orbm_bf_match_batch_device's output: pair p's queries have angles
 * d_angA[(p*capA + i)*kstrideA] (kstrideA = 7 with d_angA = &kps[0].angle of an orbx_keypoint
 * array), its targets d_angB[(q*capB + j)*kstrideB] with q = d_pair_b ? d_pair_b[p] : p; d_nA[p]
 * queries; d_match at p*strideM is updated in place; d_nmatches[p] (may be NULL).  One workgroup
 * per pair; enqueue only. */
int orbm_check_orientation_batch_device(const float* d_angA, int kstrideA, int capA, const int32_t* d_nA,
                                        const float* d_angB, int kstrideB, int capB, const int32_t* d_pair_b,
                                        int n_pairs, int32_t* d_match, int strideM, int32_t* d_nmatches,
                                        void* stream);

/* One keyframe's view for SearchForTriangulation (src/ORBmatcher.cc:768-866). */
typedef struct orbm_tri_frame {
    int32_t        n;           /* keyframe->N */
    const float*   kp_xy;       /* keypointsUn pt, n x 2 */
    const int32_t* octave;      /* keypointsUn octave, n */
    const float*   uright;      /* n (< 0: mono) */
    const uint8_t* has_mappoint;/* GetMapPoint(idx) != nullptr, n (0/1) */
    const uint8_t* desc;        /* descriptorsL, n x 32 */
    /* DBoW2 FeatureVector as CSR: node ids ascending, node k owns
     * indices[node_off[k] .. node_off[k+1]) (ascending feature indices). */
    int32_t        n_nodes;
    const uint32_t* node_id;
    const int32_t* node_off;
    const int32_t* indices;
} orbm_tri_frame;

/* int ORBmatcher::SearchForTriangulation(const KeyFrame* kf1, const KeyFrame* kf2,
 *   const cv::Mat& F12, std::vector<std::pair<size_t,size_t>>& matchIds, bool onlyStereo)
 * (include/ORBmatcher.h:84-85).  F12 row-major 3x3 (cv::Mat1f); ep2 = projection of kf1's
 * camera centre in kf2 (:772-773); scale2/sigma2: kf2 pyramid scaleFactors / sigmaSq.
 * Host memory.  match12[idx1] = idx2 or -1 (pairs sorted by idx1 are the non-negative
 * entries); *nmatches = count.  checkOrientation is false at the only caller
 * (LocalMapping.cc:388), so it is not applied. */
int orbm_search_for_triangulation(const orbm_tri_frame* kf1, const orbm_tri_frame* kf2,
                                  const float* F12, const float* ep2, const float* scale2,
                                  const float* sigma2, int n_levels, int only_stereo,
                                  int32_t* match12, int32_t* nmatches);

/* Batched SearchForTriangulation on HBM-resident extractor output (orbx_extract_batch_device slots),
 * e.g. one round of the neighbour-keyframe loop of LocalMapping::CreateNewMapPoints
 * (LocalMapping.cc:380-430; the loop itself, which is sequential through keyframe 1's MapPoint flags, is
 * orblm_create_new_map_points_device).  Pair p matches keyframe frame1[p] of set 1 (slots at kps1 / desc1 +
 * frame*cap1, counts1[frame]) against frame2[p] of set 2 (NULL index arrays: p).  Sets 1 and 2 may
 * be the same arrays.  Per pair: F12 (9 floats, row-major, from ComputeF12 :55-71) and ep2 (2
 * floats, kf1's camera centre projected by kf2, :772-773; may be non-finite).  uright / has_mappoint
 * per slot (NULL: every keypoint monocular / without a MapPoint).  FeatureVectors in
 * orbv_transform_batch_device's layout (node ids / offsets / indices at frame*fv_cap, offsets at
 * frame*(fv_cap+1), fv_n_nodes[frame]); NULL for both sets = one node holding every keypoint
 * (all-pairs search under the gates, the vocabulary-free C3 setup).  kf2's scale factors / sigma^2
 * are host arrays of n_levels (<= ORBM_TRI_MAX_LEVELS).  Outputs: d_match12[p*cap1 + idx1] = idx2
 * or -1 for idx1 < counts1; d_nmatches[p].  checkOrientation is false at the caller
 * (LocalMapping.cc:388).  Enqueue only on `stream`. */
#define ORBM_TRI_MAX_LEVELS 32
typedef struct orbm_tri_batch {
    int32_t n_pairs;
    int32_t cap1, cap2;
    const orbx_keypoint* kps1; const uint8_t* desc1; const int32_t* counts1;
    const float* uright1; const uint8_t* has_mappoint1;
    const orbx_keypoint* kps2; const uint8_t* desc2; const int32_t* counts2;
    const float* uright2; const uint8_t* has_mappoint2;
    const int32_t* frame1; const int32_t* frame2;
    const float* F12;           /* n_pairs x 9 */
    const float* ep2;           /* n_pairs x 2 */
    const uint32_t* fv_node1; const int32_t* fv_off1; const int32_t* fv_idx1; const int32_t* fv_n_nodes1;
    const uint32_t* fv_node2; const int32_t* fv_off2; const int32_t* fv_idx2; const int32_t* fv_n_nodes2;
    int32_t fv_cap1, fv_cap2;
    int32_t n_levels;
    const float* scale_factors2; /* host, n_levels */
    const float* sigma2;         /* host, n_levels */
    int32_t only_stereo;
} orbm_tri_batch;

int orbm_search_for_triangulation_batch_device(const orbm_tri_batch* b, int32_t* d_match12, int32_t* d_nmatches,
                                               void* stream);

/* int ORBmatcher::SearchByBoW(KeyFrame* keyframe, Frame& frame, std::vector<MapPoint*>& matches)
 * (include/ORBmatcher.h:77, src/ORBmatcher.cc:452-516; callers Tracking.cc TrackReferenceKeyFrame /
 * Relocalization), batched on HBM-resident extractor slots.  Pair p matches keyframe frame1[p] of
 * set 1 (NULL: p) against frame p of set 2.  FeatureVectorIterator (:406-450) joins equal node ids;
 * in a common node every keyframe feature idx1 (ascending, as stored) with mp_valid1 != 0
 * (GetMapPointMatches()[idx1] non-null and not isBad(); NULL = all valid) scans the node's frame
 * features that no earlier idx1 claimed (the reference's `if (matches[idx2]) continue`), keeps the
 * lowest-index best and the second-best distance, and claims bestIdx2 when best <= TH_LOW (50) and
 * (float)best < nnratio * (float)second.  A frame feature sits in one node only, so the claims of
 * different nodes are independent and the result is the reference's.  With check_orientation the
 * rotation-histogram filter (CheckOrientation(keyframe->keypointsUn, frame.keypointsUn, ...),
 * :249-309, :512-513) erases the matches outside the top bins.  FeatureVectors in
 * orbv_transform_batch_device's layout (both sets required).  Outputs: d_match[p*cap2 + idx2] =
 * idx1 (the MapPoint of keyframe feature idx1) or -1 for idx2 < counts2[p]; d_nmatches[p] = the
 * return value.  Enqueue only on `stream`. */
typedef struct orbm_bow_batch {
    int32_t n_pairs;
    int32_t cap1, cap2;
    const orbx_keypoint* kps1; const uint8_t* desc1; const uint8_t* mp_valid1;
    const int32_t* frame1;
    const orbx_keypoint* kps2; const uint8_t* desc2; const int32_t* counts2;
    const uint32_t* fv_node1; const int32_t* fv_off1; const int32_t* fv_idx1; const int32_t* fv_n_nodes1;
    const uint32_t* fv_node2; const int32_t* fv_off2; const int32_t* fv_idx2; const int32_t* fv_n_nodes2;
    int32_t fv_cap1, fv_cap2;
    float nnratio;
    int32_t check_orientation;
    /* KeyFrame-KeyFrame form only (NULL in the Frame form): */
    const int32_t* counts1;      /* kf1 keypoint counts (CheckOrientation) */
    const uint8_t* mp_valid2;    /* kf2 MapPoint valid (NULL: all) */
    const int32_t* frame2;       /* kf2 slot of pair p (NULL: p) */
} orbm_bow_batch;

int orbm_search_by_bow_batch_device(const orbm_bow_batch* b, int32_t* d_match, int32_t* d_nmatches, void* stream);

/* int ORBmatcher::SearchByBoW(KeyFrame* keyframe1, KeyFrame* keyframe2, std::vector<MapPoint*>& matches12)
 * (include/ORBmatcher.h:78, src/ORBmatcher.cc:696-766) on the same batch layout: pair p = (kf1
 * frame1[p] of set 1, kf2 frame2[p] of set 2).  Differences from the Frame form: candidates need a
 * valid kf2 MapPoint (mp_valid2) besides being unclaimed (matched2, :733), acceptance is
 * bestDist < TH_LOW (strict, :750), the result is indexed by idx1 (d_match12[p*cap1 + idx1] = idx2,
 * i.e. matches12[idx1] = mappoints2[idx2]) and CheckOrientation(keypoints2, keypoints1, ...)
 * (:762-763) bins angle2[idx2] - angle1[idx1] and erases matches12[idx1] (needs counts1).
 * Enqueue only on `stream`. */
int orbm_search_by_bow_kf_batch_device(const orbm_bow_batch* b, int32_t* d_match12, int32_t* d_nmatches,
                                       void* stream);

/* Stereo matching.  Replaces ComputeStereoMatches (src/ORBmatcher.cc:72-247, PatchDistance
 * :60-68; called from Frame construction for stereo input, System.cc:458-461): per left keypoint the
 * best right keypoint in the row band (+-2*scale[octave_R] rows), octave +-1 and disparity
 * [0, bf/baseline], Hamming < (TH_HIGH+TH_LOW)/2; then 11x11 SAD over +-5 px on the unblurred
 * level of the left octave, parabola refinement, and the median-distance outlier filter.
 * Outputs uright[i] / depth[i] (-1 = no match), one per left keypoint.
 * A view is one frame: its keypoints (level-0 coordinates, cv::KeyPoint layout), descriptors and
 * unblurred pyramid levels (GetImagePyramid()).  The right keypoints' row table (vRowIndices) is
 * built on the device for images of at most 4096 rows (ORB_EINVAL above); a row band reaching past
 * the image is clipped to it (the reference indexes outside vRowIndices there).  At most 12286
 * keypoints per side and frame (slots, for the device entries), ORB_EINVAL above.  Not checked, as
 * in the reference: the left 11x11 patch and the right window from column suR - 10 on must lie inside
 * the left octave's level for every candidate below the Hamming gate. */
typedef struct orbm_stereo_view {
    int32_t n;
    const orbx_keypoint* kps;
    const uint8_t* desc;                 /* n x 32 */
    int32_t n_levels;
    const uint8_t* const* level;         /* n_levels level images */
    const int32_t* level_rows;
    const int32_t* level_cols;
    const int32_t* level_step;           /* bytes per row */
} orbm_stereo_view;

int orbm_compute_stereo_matches(const orbm_stereo_view* left, const orbm_stereo_view* right,
                                const float* scale_factors, const float* inv_scale_factors, float bf,
                                float baseline, float* uright, float* depth);

/* Batched device version on the frames of two extractors' last batches (left frame f with right
 * frame f; both extractors with the same Parameters and image size).  Keypoints / descriptors /
 * counts are those batches' outputs.  d_uright / d_depth: n_frames * cap floats, slot f*cap + i.
 * Enqueue only, on `stream` (NULL = default stream). */
int orbx_stereo_matches_batch_device(orbx_extractor* left, orbx_extractor* right, int n_frames,
                                     const orbx_keypoint* d_kps_l, const uint8_t* d_desc_l,
                                     const int32_t* d_counts_l, const orbx_keypoint* d_kps_r,
                                     const uint8_t* d_desc_r, const int32_t* d_counts_r, int cap,
                                     float bf, float baseline, float* d_uright, float* d_depth,
                                     void* stream);

/* ComputeStereoMatches for the reference's own call shape (System.cc:449-461, Frame's stereo
 * constructor: two Extract calls, then ComputeStereoMatches on mvKeys / mvKeysRight and the two
 * extractors' mvImagePyramid): `left` / `right` are the handles whose last call was orbx_extract on
 * the pair's images; their keypoints, descriptors and pyramids are still on the device, so nothing but
 * uright / depth (n_left floats each, -1 = no match) crosses PCIe.  n_left must equal the left
 * Extract's keypoint count.  Synchronous; call after both Extract calls have returned. */
int orbx_stereo_matches_last(orbx_extractor* left, orbx_extractor* right, float bf, float baseline, float* uright,
                             float* depth, int n_left);

/* ------------------------------------------------------------------------------------------
 * Local-map search.  Replaces ORBmatcher::SearchByProjection(Frame&, const std::vector<MapPoint*>&,
 * float th) (include/ORBmatcher.h:58, src/ORBmatcher.cc:315-382) together with the frame's
 * FeaturesGrid (include/Frame.h:62-80; AssignFeatures / GetFeaturesInArea, src/Frame.cc:71-145),
 * batched over frames.  Per frame f: keypoints [kp_begin[f], kp_begin[f+1]) (keypointsUn order)
 * and the local map points [mp_begin[f], mp_begin[f+1]) (vector order) with the fields
 * IsInFrustum filled (Tracking.cc:554-605).
 * ---------------------------------------------------------------------------------------- */
#define ORBM_GRID_COLS 64
#define ORBM_GRID_ROWS 48
#define ORBM_PROJ_MAX_KP 8192   /* keypoints per frame */

typedef struct orbm_proj_batch {
    int32_t        n_frames;
    int32_t        total_kp, total_mp;   /* kp_begin[n_frames], mp_begin[n_frames] (workspace sizing) */
    const int32_t* kp_begin;     /* n_frames + 1 */
    const float*   kp_xy;        /* keypointsUn pt, total_kp x 2 */
    const int32_t* kp_octave;    /* keypointsUn octave */
    const float*   kp_uright;    /* uright */
    const uint8_t* kp_desc;      /* descriptors, total_kp x 32 */
    const uint8_t* kp_claimed;   /* mappoints[i] && mappoints[i]->Observations() > 0 on entry (NULL: none) */
    const float*   bounds;       /* n_frames x 4: imageBounds minx, maxx, miny, maxy */
    const int32_t* mp_begin;     /* n_frames + 1 */
    const uint8_t* mp_valid;     /* trackInView && !isBad() (:320) */
    const float*   mp_proj;      /* total_mp x 3: trackProjX, trackProjY, trackProjXR */
    const float*   mp_view_cos;  /* trackViewCos */
    const int32_t* mp_level;     /* trackScaleLevel (0 .. n_levels-1) */
    const uint8_t* mp_desc;      /* GetDescriptor(), total_mp x 32 */
    const uint8_t* mp_has_obs;   /* Observations() > 0 (a keypoint it claims is then skipped, :339) */
    int32_t        n_levels;
    const float*   scale_factors;/* n_levels (frame.pyramid.scaleFactors), host memory in both entries */
    float          th;           /* SearchLocalPoints: 1, 3 (RGB-D) or 5 after relocalisation (Tracking.cc:1246) */
    float          nnratio;      /* ORBmatcher(0.8f) in SearchLocalPoints (Tracking.cc:646) */
} orbm_proj_batch;

/* kp_match[k]: frame-relative index of the map point the call assigned to keypoint k (the last
 * assignment of frame.mappoints[bestIdx] = mappoint, :376), -1 when the call assigned none.
 * n_matches[f]: SearchByProjection's return value; -1 (device entry) when a frame has more than
 * ORBM_PROJ_MAX_KP keypoints.  Host entry: every pointer is host memory, synchronous. */
int orbm_search_by_projection(const orbm_proj_batch* b, int32_t* kp_match, int32_t* n_matches, int device);
/* Device entry: every array in HBM except scale_factors; enqueue only on `stream`. */
int orbm_search_by_projection_device(const orbm_proj_batch* b, int32_t* kp_match, int32_t* n_matches,
                                     void* stream);

/* int ORBmatcher::SearchByProjection(Frame& currFrame, const Frame& lastFrame, float th, bool monocular)
 * (include/ORBmatcher.h:61, src/ORBmatcher.cc:1279-1362; Tracking::TrackWithMotionModel), batched over
 * frames.  Current frame f: keypoints [kp_begin[f], kp_begin[f+1]) as in orbm_proj_batch, plus
 * kp_angle (keypointsUn angle, for CheckOrientation).  Last frame's points [mp_begin[f], mp_begin[f+1])
 * in idx1 order: mp_valid = mappoints[idx1] && !outlier[idx1] && Xc.z >= 0 && imageBounds.Contains(u, v)
 * (:1295-1311, the caller projects), mp_proj = (u, v, ur = u - DepthToDisparity(Xc.z)), mp_octave =
 * lastFrame.keypoints[idx1].octave, mp_desc = GetDescriptor(), mp_has_obs = Observations() > 0,
 * mp_angle = lastFrame.keypointsUn[idx1].angle.  motion[f]: 0, 1 = forward, 2 = backward (:1286-1288).
 * Window th * scaleFactors[octave] over the levels of :1318-1319, claimed keypoints skipped, the
 * stereo gate with the window radius, best distance <= TH_HIGH; then CheckOrientation(lastFrame,
 * currFrame, ...) (:1358-1359) over every accepted (idx1, bestIdx2) pair in order (overwritten ones
 * included, as the reference's matchIds).  kp_match[k] = frame-relative idx1 the call assigned to
 * keypoint k (-1: none, or erased by the rotation filter); n_matches[f] = the return value (-1 when
 * the frame has more than ORBM_PROJ_MAX_KP keypoints).  Enqueue only on `stream`. */
typedef struct orbm_motion_batch {
    int32_t        n_frames, total_kp, total_mp;
    const int32_t* kp_begin;
    const float*   kp_xy;
    const int32_t* kp_octave;
    const float*   kp_uright;
    const uint8_t* kp_desc;
    const float*   kp_angle;
    const uint8_t* kp_claimed;   /* currFrame.mappoints[i] with Observations() > 0 on entry (NULL: none) */
    const float*   bounds;       /* n_frames x 4 */
    const int32_t* mp_begin;
    const uint8_t* mp_valid;
    const float*   mp_proj;      /* total_mp x 3 */
    const int32_t* mp_octave;
    const uint8_t* mp_desc;
    const uint8_t* mp_has_obs;
    const float*   mp_angle;
    const int32_t* motion;       /* n_frames (NULL: all 0) */
    int32_t        n_levels;
    const float*   scale_factors;/* host, n_levels */
    float          th;
    int32_t        check_orientation;
} orbm_motion_batch;

int orbm_search_by_projection_motion_device(const orbm_motion_batch* b, int32_t* kp_match, int32_t* n_matches,
                                            void* stream);

/* int ORBmatcher::SearchByProjection(Frame& frame, KeyFrame* keyframe, const std::set<MapPoint*>& alreadyFound,
 * float th, int ORBdist) (include/ORBmatcher.h:66, src/ORBmatcher.cc:1364-1445; Tracking::Relocalization
 * calls it with th 10 / ORBdist 100, then th 3 / ORBdist 64, Tracking.cc:403,417), batched over
 * (frame, candidate keyframe) pairs.  Frame f: keypoints [kp_begin[f], kp_begin[f+1]) as in
 * orbm_motion_batch (no uright: the search has no stereo gate), kp_claimed = frame.mappoints[i] != NULL
 * on entry (every non-null entry blocks, :1413-1414), its pose Rcw / tcw and intrinsics.  Keyframe
 * points [mp_begin[f], mp_begin[f+1]) = GetMapPointMatches() in idx1 order: mp_valid = mappoint &&
 * !isBad() && !alreadyFound.count(mappoint), mp_xw = GetWorldPos(), mp_max_min = (maxDistance_,
 * minDistance_) (MapPoint.cc:369-377), mp_angle = keyframe->keypointsUn[idx1].angle.  On the device:
 * the projection and imageBounds.Contains (:1385-1391), the distance-invariance gate with 0.8f /
 * 1.2f (:1393-1401, MapPoint.cc:382-392), PredictScale (MapPoint.cc:405-415: ceil(log(ratio) /
 * logScaleFactor), log taken as ::log(double)), the window th * scaleFactors[predictedScale] over
 * levels predictedScale +- 1, the first-best distance over the keypoints not yet holding a map point,
 * bestDist <= ORBdist (< 256), the claim, then CheckOrientation(keyframe->keypointsUn,
 * frame.keypointsUn, ...) (:1439-1440).  kp_match[k] = idx1 assigned to frame keypoint k (-1: none or
 * erased), n_matches[f] = the return value (-1 when the frame has more than ORBM_PROJ_MAX_KP
 * keypoints). */
typedef struct orbm_reloc_batch {
    int32_t        n_frames, total_kp, total_mp;
    const int32_t* kp_begin;
    const float*   kp_xy;        /* frame keypointsUn pt */
    const int32_t* kp_octave;
    const uint8_t* kp_desc;
    const float*   kp_angle;
    const uint8_t* kp_claimed;   /* frame.mappoints[i] != NULL on entry (NULL: none) */
    const float*   bounds;       /* n_frames x 4: imageBounds minx, maxx, miny, maxy */
    const float*   pose;         /* n_frames x 12: Rcw (row-major 3x3) then tcw */
    const float*   camera;       /* n_frames x 4: fx, fy, cx, cy */
    const int32_t* mp_begin;
    const uint8_t* mp_valid;
    const float*   mp_xw;        /* total_mp x 3 */
    const float*   mp_max_min;   /* total_mp x 2: maxDistance_, minDistance_ */
    const uint8_t* mp_desc;
    const float*   mp_angle;
    int32_t        n_levels;
    const float*   scale_factors;/* host, n_levels */
    float          log_scale_factor; /* pyramid.logScaleFactor */
    float          th;
    int32_t        orb_dist;     /* ORBdist, 0 .. 255 */
    int32_t        check_orientation;
} orbm_reloc_batch;

/* Host entry: every pointer host memory, synchronous. */
int orbm_search_by_projection_reloc(const orbm_reloc_batch* b, int32_t* kp_match, int32_t* n_matches, int device);
/* Device entry: every array in HBM except scale_factors; enqueue only on `stream`. */
int orbm_search_by_projection_reloc_device(const orbm_reloc_batch* b, int32_t* kp_match, int32_t* n_matches,
                                           void* stream);

/* int ORBmatcher::Fuse(KeyFrame* keyframe, const std::vector<MapPoint*>& mappoints, float th)
 * (src/ORBmatcher.cc:868-980; LocalMapping::SearchInNeighbors, LocalMapping.cc:606,624, th 3) and
 * int ORBmatcher::Fuse(KeyFrame* keyframe, const Sim3& Scw, const std::vector<MapPoint*>& mappoints, float th,
 * std::vector<MapPoint*>& replacePoints) (src/ORBmatcher.cc:982-1088; LoopClosing.cc:648, th 4), batched
 * over (keyframe, point list) items.  Item i: the keyframe's keypoints [kp_begin[i], kp_begin[i+1])
 * (keypointsUn pt / octave, uright, descriptorsL rows), its imageBounds, pose and intrinsics; the
 * candidate points [mp_begin[i], mp_begin[i+1]) in list order.  pose = Rcw then tcw of GetPose(); for
 * the Sim3 overload Scw.R() and Scw.t() / s (:987).  mp_valid is the caller's skip test, evaluated on
 * entry over a list of distinct points: mappoint && !isBad() && !IsInKeyFrame(keyframe) (:876), or
 * !isBad() && !alreadyFound.count(mappoint) (:1002).  mp_xw = GetWorldPos(), mp_max_min = (maxDistance_,
 * minDistance_) raw (MapPoint.cc:369-377), mp_normal = GetNormal(), mp_desc = GetDescriptor().
 * On the device, in the reference's order and float expressions: Xc = Rcw * Xw + tcw, Xc.z < 0 rejects
 * (:883), CameraToImage and imageBounds.Contains (:886-892), ur = u - bf / Xc.z (:894), the
 * distance-invariance gate with 0.8f / 1.2f (:896-903, MapPoint.cc:382-392), the viewing-angle gate
 * PO.dot(Pn) < 0.5 * dist3D (:905-908), PredictScale (MapPoint.cc:394-403, ::log(double)), the window
 * GetFeaturesInArea(u, v, th * scaleFactors[predictedScale]) (:913-915), the levels [predictedScale - 1,
 * predictedScale] (:930), with chi2_gate the reprojection gates 7.8 (uright >= 0) / 5.99 on
 * NormSq * invSigmaSq[octave] (:933-945; the Sim3 overload has none), and the first minimum descriptor
 * distance in scan order (:947-953).  Keypoints holding a map point are not skipped, and the per-point
 * result does not depend on the Replace / AddObservation calls of earlier iterations, so the caller
 * applies :957-976 (or :1070-1084) in list order from best_idx. */
typedef struct orbm_fuse_batch {
    int32_t        n_items, total_kp, total_mp;
    const int32_t* kp_begin;     /* n_items + 1 */
    const float*   kp_xy;        /* keyframe keypointsUn pt, total_kp x 2 */
    const int32_t* kp_octave;
    const float*   kp_uright;    /* uright (-1: monocular keypoint); read with chi2_gate only */
    const uint8_t* kp_desc;      /* total_kp x 32 */
    const float*   bounds;       /* n_items x 4: imageBounds minx, maxx, miny, maxy */
    const float*   pose;         /* n_items x 12: Rcw (row-major 3x3) then tcw */
    const float*   camera;       /* n_items x 5: fx, fy, cx, cy, bf */
    const int32_t* mp_begin;     /* n_items + 1 */
    const uint8_t* mp_valid;
    const float*   mp_xw;        /* total_mp x 3 */
    const float*   mp_max_min;   /* total_mp x 2: maxDistance_, minDistance_ */
    const float*   mp_normal;    /* total_mp x 3 */
    const uint8_t* mp_desc;      /* total_mp x 32 */
    int32_t        n_levels;
    const float*   scale_factors;/* host, n_levels (keyframe->pyramid.scaleFactors) */
    const float*   inv_sigma2;   /* host, n_levels (pyramid.invSigmaSq); read with chi2_gate only */
    float          log_scale_factor; /* pyramid.logScaleFactor */
    float          th;
    int32_t        chi2_gate;    /* 1: the first overload (:933-945); 0: the Sim3 overload */
} orbm_fuse_batch;

/* best_idx[m]: keyframe-relative bestIdx of point m when bestDist <= TH_LOW (50), else -1.
 * best_dist[m]: the minimum distance found, 256 when no candidate passed the gates.  n_fused[i]: Fuse's
 * return value (nfused++ runs on both branches of :957-976), the count of best_idx >= 0; -1 (device
 * entry, with every best_idx of the item -1) when the keyframe has more than ORBM_PROJ_MAX_KP keypoints.
 * Host entry: every pointer is host memory, synchronous, offsets validated. */
int orbm_fuse(const orbm_fuse_batch* b, int32_t* best_idx, int32_t* best_dist, int32_t* n_fused, int device);
/* Device entry: every array in HBM except scale_factors / inv_sigma2; enqueue only on `stream`. */
int orbm_fuse_device(const orbm_fuse_batch* b, int32_t* best_idx, int32_t* best_dist, int32_t* n_fused, void* stream);

/* int ORBmatcher::SearchByProjection(const KeyFrame* keyframe, const Sim3& Scw, const std::vector<MapPoint*>&
 * mappoints, std::vector<MapPoint*>& matched, int th) (src/ORBmatcher.cc:518-612; LoopClosing::ComputeSim3,
 * LoopClosing.cc:277, th 10) on an orbm_fuse_batch (pose = Scw.R(), Scw.t() / s (:523); mp_valid =
 * !isBad() && !alreadyFound.count(mappoint) (:537); kp_uright, inv_sigma2, chi2_gate and the camera's bf
 * are not read) plus kp_claimed[k] = matched[k] != NULL on entry (total_kp, NULL: none).  The same
 * projection and gates (:540-572), then for each point in list order the first minimum distance over
 * the window's keypoints of levels [predictedScale - 1, predictedScale] that hold no match yet (:588),
 * bestDist <= TH_LOW, and the claim matched[bestIdx] = mappoint (:604-608).  kp_match[k] = item-relative
 * index of the point the call assigned to keypoint k, -1 when none; n_matches[i] = the return value (-1,
 * device entry, when the keyframe has more than ORBM_PROJ_MAX_KP keypoints).
 * Host entry: every pointer is host memory, synchronous, offsets validated. */
int orbm_search_by_projection_sim3(const orbm_fuse_batch* b, const uint8_t* kp_claimed, int32_t* kp_match,
                                   int32_t* n_matches, int device);
/* Device entry: every array in HBM except scale_factors; enqueue only on `stream`. */
int orbm_search_by_projection_sim3_device(const orbm_fuse_batch* b, const uint8_t* kp_claimed, int32_t* kp_match,
                                          int32_t* n_matches, void* stream);

/* int ORBmatcher::SearchBySim3(KeyFrame* keyframe1, KeyFrame* keyframe2, std::vector<MapPoint*>& matches12,
 * const Sim3& S12, float th) (src/ORBmatcher.cc:1090-1277; LoopClosing::FindLoopInCandidateKFs,
 * LoopClosing.cc:137, th 7.5), batched over (keyframe1, keyframe2, S12) pairs.  Pair p: side s in {1, 2} has
 * the keypoint slots [kp{s}_begin[p], kp{s}_begin[p+1]) (keypointsUn pt / octave, descriptorsL rows), the
 * keyframe's imageBounds, GetPose() (Rcw then tcw) and intrinsics, and one map point row per slot.
 * mp1_valid[i1] = mappoints1[i1] && !matches12[i1] && !mappoints1[i1]->isBad() (:1130) and mp2_valid[i2] =
 * mappoints2[i2] && !alreadyMatched2[i2] && !mappoints2[i2]->isBad() (:1197, alreadyMatched2 from
 * GetIndexInKeyFrame(keyframe2) over the incoming matches12, :1111-1121), both evaluated on entry; for a
 * valid slot mp_xw = GetWorldPos(), mp_max_min = (maxDistance_, minDistance_) raw, mp_desc =
 * GetDescriptor() (the map point's descriptor, not the slot's keypoint row).  s12 = S12's R (row-major), t, s.
 * On the device, in the reference's order and float expressions, for every valid slot of keyframe 1:
 * Xc1 = R1w * Xw + t1w, Xc2 = S21.Map(Xc1) with S21 = S12.Inverse() derived there (Sim3.h:40-47: (s * R) * x
 * + t; R21 = R12^T, t21 = ((-(1 / s)) * R12^T) * t12, s21 = 1 / s), Xc2.z < 0 rejects (:1138), CameraToImage
 * with keyframe 2's intrinsics and its half-open bounds (:1141-1147), dist3D = (float)cv::norm(Xc2) against
 * 0.8f * minDistance_ / 1.2f * maxDistance_ (:1149-1155; no viewing-angle and no chi2 gate), PredictScale
 * (MapPoint.cc:394-403), the window GetFeaturesInArea(u, v, th * scaleFactors[predictedScale]) on keyframe
 * 2's grid, the levels [predictedScale - 1, predictedScale], the first minimum descriptor distance in scan
 * order, and match1[i1] = bestIdx iff bestDist <= TH_HIGH (100) (:1163-1190).  The mirror image with
 * S12.Map gives match2 (:1194-1258).  match12[i1] = match1[i1] iff match1[i1] >= 0 && match2[match1[i1]]
 * == i1, else -1 (:1261-1274).  Nothing is claimed during the loops, so no slot depends on another; the
 * caller then writes matches12[i1] = mappoints2[match12[i1]]. */
typedef struct orbm_sim3_batch {
    int32_t        n_pairs, total_kp1, total_kp2;
    const int32_t* kp1_begin;    /* n_pairs + 1 */
    const int32_t* kp2_begin;    /* n_pairs + 1 */
    const float*   kp1_xy;       /* keyframe 1 keypointsUn pt, total_kp1 x 2 */
    const int32_t* kp1_octave;
    const uint8_t* kp1_desc;     /* total_kp1 x 32 */
    const float*   kp2_xy;       /* keyframe 2, total_kp2 rows */
    const int32_t* kp2_octave;
    const uint8_t* kp2_desc;
    const float*   bounds1;      /* n_pairs x 4: imageBounds minx, maxx, miny, maxy */
    const float*   pose1;        /* n_pairs x 12: Rcw (row-major 3x3) then tcw */
    const float*   camera1;      /* n_pairs x 4: fx, fy, cx, cy */
    const float*   bounds2;
    const float*   pose2;
    const float*   camera2;
    const uint8_t* mp1_valid;    /* total_kp1 */
    const float*   mp1_xw;       /* total_kp1 x 3 */
    const float*   mp1_max_min;  /* total_kp1 x 2: maxDistance_, minDistance_ */
    const uint8_t* mp1_desc;     /* total_kp1 x 32 */
    const uint8_t* mp2_valid;    /* total_kp2 rows */
    const float*   mp2_xw;
    const float*   mp2_max_min;
    const uint8_t* mp2_desc;
    const float*   s12;          /* n_pairs x 13: R12 (row-major 3x3), t12, s */
    int32_t        n_levels;
    const float*   scale_factors;/* host, n_levels (pyramid.scaleFactors) */
    float          log_scale_factor;
    float          th;
} orbm_sim3_batch;

/* match12 [total_kp1]: keyframe-2-relative index agreed for slot i1 or -1; match1 [total_kp1] / match2
 * [total_kp2]: the one-way results (may be NULL); n_found[p]: the return value, the count of match12 >= 0.
 * Host entry: every pointer is host memory, synchronous, offsets validated; a keyframe with more than
 * ORBM_PROJ_MAX_KP keypoints is refused. */
int orbm_search_by_sim3(const orbm_sim3_batch* b, int32_t* match12, int32_t* match1, int32_t* match2,
                        int32_t* n_found, int device);
/* Device entry: every array in HBM except scale_factors; enqueue only on `stream`.  A pair either of whose
 * keyframes has more than ORBM_PROJ_MAX_KP keypoints gets n_found = -1 and every match* of the pair -1;
 * the other pairs are unaffected. */
int orbm_search_by_sim3_device(const orbm_sim3_batch* b, int32_t* match12, int32_t* match1, int32_t* match2,
                               int32_t* n_found, void* stream);

/* void MapPoint::ComputeDistinctiveDescriptors() (src/MapPoint.cc:257-320; after every AddObservation and at
 * the end of Replace; LocalMapping::SearchInNeighbors runs one per map point of the keyframe,
 * LocalMapping.cc:626-635), batched over map points.  Point p holds the rows [begin[p], begin[p+1]) of
 * desc: its observations' descriptorsL.row(idx) from non-bad keyframes, gathered in the reference's
 * iteration order.  best[p] = the point-relative row with the least median Hamming distance to the rows
 * of the point, the median being sorted(row of the N x N matrix, zero diagonal included)[(N - 1) / 2] and
 * the lowest row winning a tie (:300-314); best_median[p] = that median; out_desc[p] = the winning row.
 * An empty point gets best = best_median = -1 and its out_desc row is not written, so out_desc may be the
 * caller's resident map point descriptor array, updated in place. */
#define ORBM_DISTINCT_MAX_OBS 1024   /* rows per map point */
/* Host entry: host pointers, synchronous; a point with more than ORBM_DISTINCT_MAX_OBS rows is refused. */
int orbm_distinctive_descriptors(const uint8_t* desc /* total x 32 */, const int32_t* begin /* n_points + 1 */,
                                 int32_t n_points, int32_t* best, int32_t* best_median /* or NULL */,
                                 uint8_t* out_desc /* n_points x 32 or NULL */, int device);
/* Device entry: every array in HBM; enqueue only on `stream`.  A point over the limit gets best =
 * best_median = -1 and its out_desc row is not written. */
int orbm_distinctive_descriptors_device(const uint8_t* desc, const int32_t* begin, int32_t n_points, int32_t* best,
                                        int32_t* best_median, uint8_t* out_desc, void* stream);

/* int ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, std::vector<cv::Point2f>& vbPrevMatched,
 * std::vector<int>& vnMatches12, int windowSize) (include/ORBmatcher.h:81, src/ORBmatcher.cc:614-694;
 * Tracking::MonocularInitialization, Tracking.cc:1052), batched over initialisation pairs.
 * Pair p: frame F1 (queries idx1) = [q_begin[p], q_begin[p+1]) and frame F2 (searched) =
 * [kp_begin[p], kp_begin[p+1]), both keypointsUn.  Only octave-0 queries search, over the octave-0
 * features of F2 inside FeaturesGrid::GetFeaturesInArea(prevMatched, windowSize) (Frame.cc:102-145,
 * scan order cell by cell); a candidate is skipped when the distance it is already held at
 * (matchedDistance, INT_MAX on entry) is <= its own, so a later query can take a feature from an
 * earlier one (matches12 of the earlier query becomes -1, :669-673).  Accept best <= TH_LOW and
 * best < nnratio * second; then, with check_orientation, CheckOrientation(F2.keypointsUn,
 * F1.keypointsUn, matchIds, matches12) (:249-309) over every accepted (idx2, idx1) in order,
 * replaced ones included, whose count is the return value.  prev_matched[q] (total_q x 2, in/out)
 * becomes F2.keypointsUn[matches12[q]].pt for every surviving match (:690-692).
 * matches12[q] = F2-relative idx2 or -1; n_matches[p] = the return value, -1 (device entry) when a
 * frame of the pair has more than ORBM_PROJ_MAX_KP keypoints. */
typedef struct orbm_init_batch {
    int32_t        n_pairs, total_kp, total_q;
    const int32_t* kp_begin;     /* F2: n_pairs + 1 */
    const float*   kp_xy;        /* F2 keypointsUn pt, total_kp x 2 */
    const int32_t* kp_octave;    /* F2 keypointsUn octave */
    const uint8_t* kp_desc;      /* F2 descriptors, total_kp x 32 */
    const float*   kp_angle;     /* F2 keypointsUn angle (CheckOrientation) */
    const float*   bounds;       /* F2 imageBounds, n_pairs x 4 */
    const int32_t* q_begin;      /* F1: n_pairs + 1 */
    const int32_t* q_octave;     /* F1 keypointsUn octave */
    const uint8_t* q_desc;       /* F1 descriptors, total_q x 32 */
    const float*   q_angle;      /* F1 keypointsUn angle */
    float*         prev_matched; /* total_q x 2, in / out */
    int32_t        window;       /* windowSize (100 in MonocularInitialization) */
    float          nnratio;      /* ORBmatcher(0.9f, true) there */
    int32_t        check_orientation;
} orbm_init_batch;

/* Host entry: every pointer host memory, synchronous. */
int orbm_search_for_initialization(const orbm_init_batch* b, int32_t* matches12, int32_t* n_matches, int device);
/* Device entry: every array in HBM; enqueue only on `stream`. */
int orbm_search_for_initialization_device(const orbm_init_batch* b, int32_t* matches12, int32_t* n_matches,
                                          void* stream);

/* ------------------------------------------------------------------------------------------
 * Bag of words.  Replaces DBoW2::TemplatedVocabulary<FORB::TDescriptor, FORB> as ORBVocabulary
 * (include/ORBVocabulary.h) for Frame::ComputeBoW / KeyFrame::ComputeBoW (src/Frame.cc:208-214,
 * src/KeyFrame.cc:66-74): loadFromTextFile (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1341-1431)
 * and transform(features, BowVector&, FeatureVector&, levelsup) (:1130-1196, descent :1221-1263).
 * BowVector = std::map<WordId, double> and FeatureVector = std::map<NodeId, vector<unsigned>>
 * (BowVector.h, FeatureVector.h) are returned as ascending arrays / CSR — the FeatureVector CSR is
 * exactly orbm_tri_frame's node_id / node_off / indices.
 * ---------------------------------------------------------------------------------------- */
typedef struct orbv_vocabulary orbv_vocabulary;
#define ORBV_MAX_FEATURES 4096   /* descriptors per transform (2 x nfeatures of the initial extractor) */

/* Text format of saveToTextFile (:1434-1450): "k L scoring weighting", then one line per node
 * 1..N-1 in id order: "parent isLeaf d0 .. d31 weight".  Trailing empty lines are ignored (the
 * reference's eof loop turns a final newline into an extra root child with an uninitialised
 * descriptor and weight 0). */
int orbv_load_text(const char* path, int device, orbv_vocabulary** out);
/* The same content from arrays: node i (1 <= i < n_nodes) has parent[i], is_leaf[i], desc[32 i ..],
 * weight[i]; entries for i = 0 (the root) are ignored. */
int orbv_create(int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent,
                const uint8_t* is_leaf, const uint8_t* desc, const double* weight, int device,
                orbv_vocabulary** out);
int orbv_destroy(orbv_vocabulary* v);
int orbv_info(const orbv_vocabulary* v, int* k, int* L, int* n_nodes, int* n_words, int* scoring,
              int* weighting);

/* transform(features, BowVector&, FeatureVector&, levelsup) for one descriptor set, host memory.
 * bow_word / bow_weight: capacity n each, *n_words entries, word ids ascending.  fv_node: capacity
 * n, fv_off: n + 1, fv_idx: n; *n_nodes node ids ascending, node t owns fv_idx[fv_off[t] ..
 * fv_off[t+1]) (feature indices ascending).  Stopped words (weight 0) are in neither vector.
 * Where the reference's node id is undefined (a leaf shallower than L - levelsup) the leaf's id
 * is used. */
int orbv_transform(orbv_vocabulary* v, const uint8_t* desc, int n, int levelsup, uint32_t* bow_word,
                   double* bow_weight, int* n_words, uint32_t* fv_node, int32_t* fv_off, int32_t* fv_idx,
                   int* n_nodes);
/* Batched device form over n_frames descriptor sets (frame f: d_desc + f*cap*32, d_counts[f] rows,
 * cap <= ORBV_MAX_FEATURES) — e.g. an orbx_extract_batch_device output.  Per frame f the outputs
 * use slot f: d_bow_word / d_bow_weight / d_fv_node / d_fv_idx at f*cap, d_fv_off at f*(cap+1),
 * d_n_words[f], d_n_nodes[f].  Enqueue only on `stream`. */
int orbv_transform_batch_device(orbv_vocabulary* v, const uint8_t* d_desc, const int32_t* d_counts, int cap,
                                int n_frames, int levelsup, uint32_t* d_bow_word, double* d_bow_weight,
                                int32_t* d_n_words, uint32_t* d_fv_node, int32_t* d_fv_off, int32_t* d_fv_idx,
                                int32_t* d_n_nodes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Local bundle adjustment.  Replaces Optimizer::LocalBundleAdjustment (include/Optimizer.h:47,
 * src/Optimizer.cc:491-736) from the vertex/edge setup (:540-631) onwards: the caller
 * gathers local / fixed keyframes and map points and flattens them in reference order.
 * ---------------------------------------------------------------------------------------- */
typedef struct orbba_problem {
    int32_t        n_poses;     /* local KFs then fixed KFs (vertex insertion order) */
    const double*  pose_R;      /* n_poses x 9 row-major world->camera rotation (CameraPose R) */
    const double*  pose_t;      /* n_poses x 3 */
    const uint8_t* pose_fixed;  /* n_poses: KF id 0 or a fixed camera */
    int32_t        n_points;
    const double*  points;      /* n_points x 3 world position */
    int32_t        n_edges;     /* observations, in reference insertion order */
    const int32_t* edge_point;  /* n_edges */
    const int32_t* edge_pose;   /* n_edges */
    const double*  edge_obs;    /* n_edges x 3: u, v, ur (ur < 0 => mono edge, :595) */
    const double*  edge_inv_sigma2; /* n_edges: pyramid.invSigmaSq[octave] */
    const double*  edge_cam;    /* n_edges x 5: fx, fy, cx, cy, bf */
} orbba_problem;

typedef struct orbba_result {
    double*   pose_R;       /* n_poses x 9 (optimised; fixed poses unchanged) */
    double*   pose_t;       /* n_poses x 3 */
    double*   pose_q;       /* n_poses x 4 (x,y,z,w), g2o SE3Quat rotation; may be NULL */
    double*   points;       /* n_points x 3 */
    uint8_t*  edge_outlier; /* n_edges: 1 = chi2 > 5.991/7.815 or depth <= 0 at the end (:686-699) */
    double*   edge_chi2;    /* n_edges: final chi2 (may be NULL) */
    int32_t   iterations[2];/* LM iterations run by optimize(5) and optimize(10) */
    double    chi2[2];      /* active robust chi2 after each optimize */
    int32_t   ran;          /* 0: the stop flag was set on entry, nothing was optimised and the caller
                             * must not write anything back (Optimizer.cc:633-634 returns there) */
} orbba_result;

/* Free keyframes per optimize() (the reduced camera system is 6 x that square).  Up to 21 the system
 * is factored in LDS; above that in HBM by a 1024-thread blocked LDL^T (slower per trial, same
 * algorithm).  ORB_EINVAL beyond this limit. */
#define ORBBA_MAX_FREE_KEYFRAMES 512

/* stop_flag: g2o's force-stop flag (sparse_optimizer.h:188, LocalMapping's abortBA_); may be NULL.
 * Polled where g2o polls terminate(): before the call, between optimize(5) and optimize(10), and after
 * every LM trial (the flag is mirrored into device-visible memory while the call waits, and the
 * device's control kernel ends the loop after the trial in which it saw the flag). */
int orbba_local_ba(const orbba_problem* prob, orbba_result* res, const volatile int32_t* stop_flag,
                   int device);

/* ------------------------------------------------------------------------------------------
 * Optimizer::LocalBundleAdjustment(currKF, stopFlag, map) as a whole (src/Optimizer.cc:491-736), in place on the slot
 * tables of the map-maintenance entries below (orbtl_map's conventions: a slot stands for a pointer, -1 is null; a
 * slot, an offset or an index read from device memory is not trusted: one outside its table is skipped and no store
 * leaves a table).  Three parts, each with an entry of its own (csrc/ba_window.h holds the rules):
 *
 * 1. The window (:493-631), orbba_local_window.  In orbba_problem's order:
 *    local keyframes  cur, then ord_slot[cur][0 .. n_ord[cur]) in row order without those whose kf_bad is set (a bad
 *                     neighbour still counts as marked BALocalForKF: it is never a fixed camera); a neighbour equal to
 *                     cur or met before in the row is skipped.
 *    local points     the local keyframes in list order, kf_mappoint[k][0 .. kf_n[k]) in index order: each point that
 *                     is not null and not bad, at its first occurrence.
 *    fixed cameras    the local points in list order, their observations in CSR order without the erased ones
 *                     (mp_obs_kf == -1): each keyframe neither marked local nor marked fixed, at its first occurrence;
 *                     a bad keyframe is marked but not listed.  Departure, the one UpdateNormalAndDepth and the culls
 *                     make: the reference walks a std::map<KeyFrame*, size_t> in pointer order; here it is CSR order.
 *    edges            point-major in local-point order; a point's observations in CSR order without erased entries and
 *                     bad keyframes (and without an observation whose keypoint index or octave is outside its table).
 *                     Per edge: edge_point, edge_pose (index into local ++ fixed), the (keyframe slot, keypoint index)
 *                     behind it, (u, v, ur) from kf_keypoint[idx] and kf_uright, inv_sigma2[octave], the keyframe's
 *                     fx fy cx cy bf.  pose_fixed = (kf_id == 0) for a local keyframe, 1 for a fixed camera.
 *    counts[0 .. 4)   n_local, n_fixed, n_points, n_edges; counts[4] the status: ORBBA_WINDOW_OK, or
 *                     ORBBA_WINDOW_OVERFLOW when n_local + n_fixed > cap_poses, n_points > cap_points or n_edges >
 *                     cap_edges: the four counts are then the sizes needed and no other array of the window is
 *                     written; the other two parts do nothing on such a window.  counts[5]: every edge's camera is
 *                     cur's, bit for bit.  counts has ORBBA_WINDOW_COUNTS entries.
 *    Integer atomicMin "first position" words per slot, flags, one-workgroup scans and stable compactions: no
 *    floating-point atomics, and the result does not depend on the order anything runs in: two runs are byte-identical.
 *
 * 2. LocalBA on the window, inside orbba_local_ba_map: a kernel fills orbba_local_ba's device problem from the window
 *    (q from the float pose by the host's quat_from_R, everything else by exact float-to-double widening, mono by
 *    ur < 0); pose_fixed, edge_point, edge_pose and the counts come back for the structure build, nothing else of the
 *    window crosses PCIe.  The kernels and the LM control are orbba_local_ba's, and so are its environment knobs.
 *
 * 3. The write-back (:677-735), orbba_local_ba_apply; skipped entirely by orbba_local_ba_map when ran == 0.
 *    For every edge flagged outlier, in edge order, EraseMapPointMatch then EraseObservation: if the point still
 *    observes the keyframe, kf_mappoint[kf][idx] = -1, mp_nobs -= (kf_uright[kf][idx] >= 0 ? 2 : 1), the observation is
 *    erased (mp_obs_kf = -1), mp_ref_kf == kf becomes the first remaining observation in CSR order or -1, and mp_nobs
 *    <= 2 gives SetBadFlag (the culls' rules below); a point that has gone bad observes nothing, so its later outlier
 *    edges do nothing.  Points run in parallel, a point's edges in order.  Then kf_pose of every local keyframe =
 *    FromSE3Quat(estimate) (kf_id == 0 included), mp_xw of every local point = the narrowed estimate, and
 *    UpdateNormalAndDepth over the local points (orbmm_update_normal_depth's).
 * ---------------------------------------------------------------------------------------- */
#define ORBBA_WINDOW_OK 0
#define ORBBA_WINDOW_OVERFLOW 1
#define ORBBA_WINDOW_COUNTS 8

typedef struct orbba_window_map {
    int32_t n_keyframes, n_mappoints, kf_cap, conn_cap, n_obs, n_levels;
    const float*   inv_sigma2;      /* host memory, n_levels: pyramid.invSigmaSq */
    const float*   scale_factors;   /* host memory, n_levels: pyramid.scaleFactors (UpdateNormalAndDepth) */
    const int32_t* kf_id;           /* [K] */
    const int32_t* kf_n;            /* [K] */
    const uint8_t* kf_bad;          /* [K] */
    int32_t*       kf_mappoint;     /* [K][kf_cap], updated */
    const orbx_keypoint* kf_keypoint;   /* [K][kf_cap] keypointsUn, as orblm_batch holds them */
    const int32_t* kf_kp_octave;    /* [K][kf_cap] keypointsUn[i].octave, the table orbmm_points takes; the window alone
                                     * does not read it */
    const float*   kf_uright;       /* [K][kf_cap] */
    const float*   kf_camera;       /* [K][6] fx, fy, cx, cy, bf, baseline (orblm_batch's) */
    float*         kf_pose;         /* [K][12] Rcw row-major, tcw; updated */
    const int32_t* ord_slot;        /* [K][conn_cap] orderedConnectedKeyFrames_ */
    const int32_t* n_ord;           /* [K] */
    uint8_t*       mp_bad;          /* [M] updated */
    float*         mp_xw;           /* [M][3] updated */
    int32_t*       mp_nobs;         /* [M] updated */
    int32_t*       mp_ref_kf;       /* [M] updated */
    const int32_t* mp_obs_off;      /* [M + 1] */
    int32_t*       mp_obs_kf;       /* updated: -1 where erased */
    const int32_t* mp_obs_idx;
    float*         mp_normal;       /* [M][3] updated */
    float*         mp_max_min;      /* [M][2] updated */
} orbba_window_map;

typedef struct orbba_window {
    int32_t  cap_poses, cap_points, cap_edges;
    int32_t* counts;           /* ORBBA_WINDOW_COUNTS */
    int32_t* pose_kf;          /* [cap_poses] keyframe slot of each vertex: local, then fixed */
    uint8_t* pose_fixed;       /* [cap_poses] */
    int32_t* point;            /* [cap_points] map-point slot of each point vertex */
    int32_t* edge_point;       /* [cap_edges] */
    int32_t* edge_pose;        /* [cap_edges] */
    int32_t* edge_kf;          /* [cap_edges] keyframe slot */
    int32_t* edge_idx;         /* [cap_edges] keypoint index */
    float*   edge_obs;         /* [cap_edges][3] u, v, ur */
    float*   edge_inv_sigma2;  /* [cap_edges] */
    float*   edge_cam;         /* [cap_edges][5] fx, fy, cx, cy, bf */
} orbba_window;

typedef struct orbba_map_result {
    int32_t iterations[2];   /* orbba_result's */
    double  chi2[2];
    int32_t ran;             /* 0: the stop flag was set on entry; no table was written */
    int32_t counts[4];       /* n_local, n_fixed, n_points, n_edges */
    int32_t status;          /* ORBBA_WINDOW_* */
} orbba_map_result;

/* Device forms: every array in HBM but inv_sigma2 and scale_factors; enqueue only on `stream`.  ORB_EINVAL for a NULL
 * required array, negative sizes or capacities, kf_cap or conn_cap < 1, n_levels outside [1, 32] and a table (or
 * (conn_cap + 1) * kf_cap) of 2^31 entries or more.  The workspace (per thread, grow-only: 20 bytes per keyframe, 24 per
 * map point) belongs to the calling thread: its calls must be stream-ordered.
 * orbba_local_window_device reads kf_id, kf_n, kf_bad, kf_mappoint, kf_keypoint, kf_uright, kf_camera, ord_slot, n_ord,
 * mp_bad and the CSR; the others may be NULL there.  Nothing is copied back.
 * orbba_local_ba_apply_device: outlier[n_edges], pose_R[n_poses][9], pose_t[n_poses][3], points[n_points][3] in HBM, in
 * the window's order (orbba_result's arrays).
 * orbba_local_ba_map_device: parts 1 to 3 on `stream`, ordered after what it holds at entry.  The LM loop is
 * host-driven, so the call returns once the loop has ended; work enqueued on `stream` afterwards sees the applied
 * tables (the write-back may still be in flight at return).  window: the caller's buffers for the window, kept as the
 * call leaves them.  On ORBBA_WINDOW_OVERFLOW the call returns ORB_OK with result->status set, ran = 0 and no table
 * written.  More than ORBBA_MAX_FREE_KEYFRAMES free keyframes: ORB_EINVAL.  stop_flag as in orbba_local_ba. */
int orbba_local_window_device(const orbba_window_map* map, int32_t cur, const orbba_window* window, void* stream);
int orbba_local_ba_apply_device(const orbba_window_map* map, const orbba_window* window, const uint8_t* outlier,
                                const double* pose_R, const double* pose_t, const double* points, void* stream);
int orbba_local_ba_map_device(const orbba_window_map* map, int32_t cur, const orbba_window* window,
                              orbba_map_result* result, const volatile int32_t* stop_flag, void* stream);
/* Host forms: every pointer is host memory, synchronous; the updated arrays are written back.  Before anything is
 * copied, besides the checks above: cur in [0, n_keyframes), the offsets start at 0, do not decrease and end within
 * n_obs, mp_obs_kf in [-1, n_keyframes), mp_obs_idx in [0, kf_cap) and the octave of that keypoint in [0, n_levels),
 * kf_mappoint in [-1, n_mappoints), mp_ref_kf in [-1, n_keyframes), kf_n in [0, kf_cap], n_ord in [0, conn_cap] and the
 * first n_ord entries of a row in [0, n_keyframes), no point twice in a keyframe's row, no keyframe twice in a point's
 * observations; for the apply the window's counts within its capacities and its indices within the counts.
 * ORB_EINVAL otherwise.  orbba_local_ba_map sizes the window itself (n_keyframes poses, n_mappoints points, n_obs
 * edges). */
int orbba_local_window(const orbba_window_map* map, int32_t cur, const orbba_window* window, int device);
int orbba_local_ba_apply(const orbba_window_map* map, const orbba_window* window, const uint8_t* outlier,
                         const double* pose_R, const double* pose_t, const double* points, int device);
int orbba_local_ba_map(const orbba_window_map* map, int32_t cur, orbba_map_result* result,
                       const volatile int32_t* stop_flag, int device);

/* ------------------------------------------------------------------------------------------
 * void Optimizer::BundleAdjustment(keyframes, mappoints, nIterations, stopFlag, loopKFId, robust)
 * (include/Optimizer.h, src/Optimizer.cc:197-343), which Optimizer::GlobalBundleAdjustemnt (LoopClosing's GlobalBA
 * thread, LoopClosing.cc:366: 10 iterations, not robust) and Tracking::CreateInitialMapMonocular (Tracking.cc:1136:
 * 20 iterations, robust) call.  The problem is orbba_problem as it is: the caller flattens :212-294 in reference
 * order, leaving out bad keyframes and the observations in a keyframe that is bad or has id > maxKFId; pose_fixed
 * is id == 0.
 * Edge typing, stereo_rule: under ORBBA_GBA_RULE_REFERENCE the reference's `if (ur)` (:253) is reproduced as it
 * stands: an observation with ur != 0 (-1 or a real right coordinate alike) is a mono edge, and one with ur == 0.0
 * exactly a stereo edge with measurement (u, v, 0).  ORBBA_GBA_RULE_LOCAL types as LocalBA does (ur < 0 => mono).
 * Schedule: one optimize(n_iterations) over every edge at level 0, Huber on every edge (delta = sqrt(5.991) mono,
 * sqrt(7.815) stereo) or on none, no outlier classification.  The kernels, the lambda / rho / nu / ten-trial / nBad
 * rules and the stop-flag polling are orbba_local_ba's, and so is the calling thread's device context.
 * n_iterations == 0 optimises nothing and still counts as run.  A stop flag set on entry gives ran = 0 (g2o's
 * optimize() returns at once); the reference then still copies the unchanged estimates back, so the outputs are
 * the inputs through SE3Quat and narrowed.
 * Outputs: pose_R / pose_t / pose_q / points as orbba_result's; pose_f and points_f are FromSE3Quat / FromVector3d
 * of the estimates (:157-181), element by element the float of the double outputs: what the caller stores as
 * TcwGBA / posGBA (loopKFId != 0) or passes to SetPose / SetWorldPos.  point_included[p] = 0 for a point without
 * an edge (notIncludedMP, :285-289): it never enters the system and keeps its position.  UpdateNormalAndDepth
 * (:335) is not part of the call.  At most ORBBA_MAX_FREE_KEYFRAMES free keyframes.
 * ---------------------------------------------------------------------------------------- */
#define ORBBA_GBA_RULE_REFERENCE 0
#define ORBBA_GBA_RULE_LOCAL 1

typedef struct orbba_gba_options {
    int32_t n_iterations;   /* optimize(nIterations): 0 .. 1000 */
    int32_t robust;         /* Huber on every edge, or no robust kernel */
    int32_t stereo_rule;    /* ORBBA_GBA_RULE_REFERENCE or ORBBA_GBA_RULE_LOCAL */
} orbba_gba_options;

typedef struct orbba_gba_result {
    double*   pose_R;         /* n_poses x 9 (optimised; fixed poses unchanged) */
    double*   pose_t;         /* n_poses x 3 */
    double*   pose_q;         /* n_poses x 4 (x,y,z,w); may be NULL */
    double*   points;         /* n_points x 3 */
    float*    pose_f;         /* n_poses x 12: Rcw row-major then tcw, narrowed */
    float*    points_f;       /* n_points x 3, narrowed */
    uint8_t*  point_included; /* n_points: 0 = no edge */
    double*   edge_chi2;      /* n_edges: final chi2 (may be NULL) */
    int32_t   iterations;     /* LM iterations run */
    int32_t   trials;         /* LM trials run */
    double    chi2;           /* active robust chi2 at the end */
    int32_t   ran;            /* 0: the stop flag was set on entry */
} orbba_gba_result;

/* ORB_EINVAL for null pointers, n_iterations or stereo_rule out of range and an edge that refers to a missing
 * vertex.  stop_flag as in orbba_local_ba; may be NULL.  The call is orbba_local_ba's, so that entry's environment
 * knobs and test hooks apply to it as well: ORBBA_STRUCT, ORBBA_SOLVE_THREADS, ORBBA_SOLVE_SIMD0,
 * ORBBA_DEBUG_TIMING, ORBBA_DEBUG_SPEC_EARLY and ORBBA_DEBUG_STOP_AFTER_TRIALS, which ends the loop after that many
 * trials (0: nothing is optimised and ran = 0). */
int orbba_bundle_adjustment(const orbba_problem* prob, const orbba_gba_options* opt, orbba_gba_result* res,
                            const volatile int32_t* stop_flag, int device);

/* The reduced camera system of orbba_bundle_adjustment above 21 free keyframes is factored in HBM, by one workgroup
 * (orbba_local_ba's path) or by a blocked LDL^T spread over the grid: per block column of 32 one launch for the
 * diagonal block and the panel and one for the trailing update, then both substitutions.  ORBBA_GBA_SOLVE=grid or
 * =single (environment, read per call) forces a path; the default takes the grid from 64 free keyframes.  Both run
 * every sum in a fixed order.  orbba_debug_ldlt_grid exposes the grid factorisation alone: A x = b for a dense
 * symmetric A (D x D row-major, host memory, the lower triangle is read; 1 <= D <= 6 ORBBA_MAX_FREE_KEYFRAMES),
 * synchronous; *ok = 0 for a zero or non-finite pivot, and x is then not written. */
int orbba_debug_ldlt_grid(const double* A, const double* b, int D, double* x, int32_t* ok, int device);

/* The other two solves alone, for tests: the kernels orbba_local_ba launches, on a fabricated problem without poses or
 * points, so that only the solve of A x = b runs.  A is dense symmetric (D x D row-major, host memory; the lower
 * triangle and the diagonal blocks are read), both calls are synchronous, allocate and free their own buffers and use
 * no state of the thread's BA context.  *ok = 0 for a zero or non-finite pivot (a negative pivot is no failure), and x
 * is then all zero.
 * orbba_debug_ldlt_lds: the LDS kernel (up to 21 free keyframes), D even, 2 <= D <= 128, with `threads` = 1024 or 256
 * (ORBBA_SOLVE_THREADS) and simd0_helpers = 0 or 1 (ORBBA_SOLVE_SIMD0).  That kernel sums the system from the Schur
 * step's part matrices and adds lambda on the diagonal while it stages it; the entry splits A - lambda I into such
 * parts, so the system solved is A for any lambda that can be taken off A's diagonal without rounding (0 always;
 * ORB_EINVAL otherwise).
 * orbba_debug_ldlt_hbm: the single-workgroup HBM kernel, 1 <= D <= 7 (ORBBA_EG_MAX_KEYFRAMES - 1): the factorisation
 * orbba_optimize_essential_graph runs as well. */
int orbba_debug_ldlt_lds(const double* A, const double* b, int D, double lambda, int threads, int simd0_helpers,
                         double* x, int32_t* ok, int device);
int orbba_debug_ldlt_hbm(const double* A, const double* b, int D, double* x, int32_t* ok, int device);

/* ------------------------------------------------------------------------------------------
 * The map update behind the global bundle adjustment (GlobalBA::_Run, LoopClosing.cc:392-446) on slot tables that
 * follow orbtl_map's conventions, so a device-resident map is corrected in place.
 * Keyframes (:393-413): walked from the origins down the spanning tree.  A child whose flag is clear gets
 * TcwGBA = (Tchild * Tparent^-1) * parent.TcwGBA, with both poses the ones from before the update (a keyframe's
 * SetPose comes after its children were handled), and its flag is set.  Every keyframe the walk reaches then gets
 * TcwBefGBA = its old pose and pose = TcwGBA.  One the walk never reaches keeps all three rows, a stale
 * kf_pose_bef included, which the point pass may still read: the reference's behaviour.
 * Points (:416-446): a bad point is skipped; one with mp_in_gba set takes mp_pos_gba; any other is skipped if its
 * reference keyframe's flag is clear after the walk, and else goes into that keyframe's camera by TcwBefGBA and
 * back out by the inverse of its new pose.
 * The arithmetic is CameraPose's, in float (include/CameraPose.h:44-63): Inverse = (R^T, -R^T t), operator* is
 * t = R1 t2 + t1, R = R1 R2, products summed in k = 0, 1, 2 order, no contraction.  A child's value depends on its
 * parent's alone, so the device's level-by-level walk gives the sequential result bit for bit, in two launches
 * whatever the tree's depth.
 * ---------------------------------------------------------------------------------------- */
typedef struct orbba_gba_map {
    int32_t n_keyframes, n_mappoints, n_origins;
    const int32_t* origins;        /* n_origins: map->keyFrameOrigins as slots */
    const int32_t* kf_child_off;   /* n_keyframes + 1: CSR of GetChildren() (orbtl_map's) */
    const int32_t* kf_child_idx;
    uint8_t* kf_in_gba;            /* n_keyframes: BAGlobalForKF == loopKFId; read and updated */
    float*   kf_pose;              /* n_keyframes x 12: Rcw row-major, tcw; read and updated (SetPose) */
    float*   kf_pose_gba;          /* n_keyframes x 12: TcwGBA; read and updated */
    float*   kf_pose_bef;          /* n_keyframes x 12: TcwBefGBA; read and updated */
    const uint8_t* mp_bad;         /* n_mappoints */
    const uint8_t* mp_in_gba;      /* n_mappoints: MapPoint::BAGlobalForKF == loopKFId */
    const float*   mp_pos_gba;     /* n_mappoints x 3: posGBA */
    const int32_t* mp_ref_kf;      /* n_mappoints: GetReferenceKeyFrame() as a slot */
    float*   mp_xw;                /* n_mappoints x 3: read and updated (SetWorldPos) */
} orbba_gba_map;

/* Host entry: every pointer is host memory, synchronous; the five updated arrays are written back.  ORB_EINVAL
 * before any device call for null pointers, negative sizes, a kf_child_off that does not start at 0 or decreases,
 * an origin, child or (for a point that is neither bad nor in the adjustment) reference slot out of range, a slot
 * that is an origin twice, a child of two parents or both an origin and a child, and a non-finite kf_pose row,
 * flagged kf_pose_gba row or used mp_pos_gba row. */
int orbba_gba_update_map(const orbba_gba_map* map, int device);
/* Device entry: every array in HBM; enqueue only on `stream`, nothing is copied back.  Sizes and null pointers are
 * checked.  Whatever the tables hold, the walk ends within n_keyframes levels and nothing is written out of bounds:
 * an index out of range is skipped, a slot is visited once (so a cycle or a repeated child ends there) and a
 * kf_child_off entry is clamped to [its predecessor's clamped value, kf_child_off[n_keyframes]].  kf_child_idx must
 * hold kf_child_off[n_keyframes] entries; it may be NULL, and then no keyframe has a child.
 * The workspace belongs to the calling thread and is reused by its next call: calls from one thread must be
 * stream-ordered; threads are independent of each other. */
int orbba_gba_update_map_device(const orbba_gba_map* map, void* stream);

/* ------------------------------------------------------------------------------------------
 * Motion-only bundle adjustment.  Replaces Optimizer::PoseOptimization (include/Optimizer.h:49,
 * src/Optimizer.cc:345-489) for a batch of frames: one SE3 vertex per frame, one unary
 * EdgeSE3ProjectXYZOnlyPose / EdgeStereoSE3ProjectXYZOnlyPose per matched map point
 * (types_six_dof_expmap.h:143-202), 4 rounds of optimize(10) with chi2 outlier
 * classification (5.991 mono / 7.815 stereo), Huber kernels dropped after round 2, and a
 * single round when a frame has fewer than 10 edges.  The caller flattens, per frame, the
 * keypoints that have a map point in keypoint order (Optimizer.cc:364-410).
 * ---------------------------------------------------------------------------------------- */
#define ORBBA_POSE_MAX_EDGES 16384   /* edges per frame */

typedef struct orbba_pose_batch {
    int32_t        n_frames;
    const int32_t* edge_begin;  /* n_frames + 1: frame f owns edges [edge_begin[f], edge_begin[f+1]) */
    const double*  pose_R;      /* n_frames x 9 row-major Tcw rotation (frame->pose) */
    const double*  pose_t;      /* n_frames x 3 */
    const double*  cam;         /* n_frames x 5: fx, fy, cx, cy, bf (frame->camera) */
    const double*  xw;          /* E x 3: the map point's GetWorldPos() */
    const double*  obs;         /* E x 3: keypointsUn[i].pt.x, .y, uright[i] (ur < 0: monocular, :376) */
    const double*  inv_sigma2;  /* E: pyramid.invSigmaSq[keypointsUn[i].octave] */
} orbba_pose_batch;

typedef struct orbba_pose_result {
    double*  pose_R;     /* n_frames x 9 (frame->SetPose; input pose copied when < 3 edges) */
    double*  pose_t;     /* n_frames x 3 */
    int32_t* n_inliers;  /* n_frames: PoseOptimization's return value (nedges - noutliers, 0 if < 3);
                          * -1 from the device entry when a frame exceeds ORBBA_POSE_MAX_EDGES */
    uint8_t* outlier;    /* E: frame->outlier[i] after the last round */
} orbba_pose_result;

/* Host buffers; synchronous.  ORB_EINVAL if a frame has more than ORBBA_POSE_MAX_EDGES edges. */
int orbba_pose_optimization(const orbba_pose_batch* in, orbba_pose_result* out, int device);
/* Device buffers (every pointer in both structs); enqueue only, on `stream` (NULL = default
 * stream).  One workgroup per frame. */
int orbba_pose_optimization_device(const orbba_pose_batch* in, orbba_pose_result* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * int Optimizer::OptimizeSim3(KeyFrame* keyframe1, KeyFrame* keyframe2, std::vector<MapPoint*>& matches1,
 * Sim3& S12, float maxChi2, bool fixScale) (include/Optimizer.h, src/Optimizer.cc:944-1100;
 * LoopClosing::FindLoopInCandidateKFs, LoopClosing.cc:139, maxChi2 10), batched over (keyframe1,
 * keyframe2, S12) pairs in orbm_sim3_batch's slot layout, so orbm_search_by_sim3_device's match12 feeds
 * straight in.  fp64 throughout, one launch per batch.
 * Vertex: VertexSim3Expmap with the estimate g2o::Sim3(R12, t12, (float)s) widened to double, the rotation
 * through Quaterniond(R) without renormalisation (Optimizer.cc:183-188, sim3.h:64-67), _fix_scale =
 * fix_scale, both keyframes' intrinsics widened from float.
 * Correspondences: slot i of keyframe 1, ascending, is kept iff mp1_valid[i] && match12[i] >= 0 &&
 * mp2_valid[match12[i]] (:993-1001; i2 = match12[i] stands for GetIndexInKeyFrame(keyframe2)).  Its two
 * fixed points are Xc1 = R1w * Xw1 + t1w and Xc2 = R2w * Xw2 + t2w in float, then widened (:1006-1012).
 * Edges (:1016-1038; types_seven_dof_expmap.h:138-145, :160-167; sim3.h:144-146, :233-236):
 *   e12 = kp1_xy[i]  - cam_map1(project(S.map(Xc2))),            Omega = inv_level_sigma2[kp1_octave[i]]  * I
 *   e21 = kp2_xy[i2] - cam_map2(project(S.inverse().map(Xc1))),  Omega = inv_level_sigma2[kp2_octave[i2]] * I
 * both with a Huber kernel of delta = sqrt((double)max_chi2) that is kept for the second round.
 * Jacobian: the edges have no linearizeOplus, so it is g2o's numeric one (base_binary_edge.hpp:143-200):
 * column d = (e(+delta) - e(-delta)) * (1 / (2 delta)), delta = 1e-9, each perturbed estimate being
 * Sim3(update) * estimate (oplusImpl, types_seven_dof_expmap.h:60-69; Sim3(Vector7d), sim3.h:70-142, with
 * its four eps = 1e-5 branches).  With fix_scale update[6] is zeroed, so column 6 is exactly 0.
 * Solver: Levenberg-Marquardt as in orbba_pose_optimization (optimization_algorithm_levenberg.cpp:61-189:
 * lambda0 = 1e-5 max diag, at most 10 trials, rho with the 1e-3 term, the nBad stop), robust weighting of
 * base_binary_edge.hpp:54-120 / robust_kernel_impl.cpp:65-91, and an unpivoted dense LDL^T of the 7 x 7
 * (linear_solver_dense.h:65-115; a negative pivot fails the solve).
 * Schedule (:1046-1099): optimize(5); every correspondence with e12.chi2() > max_chi2 || e21.chi2() >
 * max_chi2 loses its match (match12[i] = -1), its two edges, and counts in nbad, chi2() being e' Omega e of
 * the last computed error (after a rejected last trial that is the rejected trial's error; nothing is
 * recomputed).  If ncorrespondences - nbad < 10 the call returns 0 with S12 unchanged and the matches
 * already removed stay removed.  Otherwise optimize(nbad > 0 ? 10 : 5) on the survivors, the same test
 * removes matches and counts n_inliers, and S12 = FromG2OSim3(estimate). */
#define ORBBA_SIM3_MAX_CORR ORBM_PROJ_MAX_KP   /* correspondences per pair */

typedef struct orbba_sim3_batch {
    int32_t        n_pairs, total_kp1, total_kp2;
    const int32_t* kp1_begin;    /* n_pairs + 1 */
    const int32_t* kp2_begin;    /* n_pairs + 1 */
    const float*   kp1_xy;       /* keyframe 1 keypointsUn pt, total_kp1 x 2 */
    const int32_t* kp1_octave;
    const float*   kp2_xy;       /* keyframe 2, total_kp2 rows */
    const int32_t* kp2_octave;
    const float*   pose1;        /* n_pairs x 12: Rcw (row-major 3x3) then tcw */
    const float*   camera1;      /* n_pairs x 4: fx, fy, cx, cy */
    const float*   pose2;
    const float*   camera2;
    const uint8_t* mp1_valid;    /* total_kp1: mappoints1[i] && !mappoints1[i]->isBad() */
    const float*   mp1_xw;       /* total_kp1 x 3 */
    const uint8_t* mp2_valid;    /* total_kp2: the map point of slot i2 exists and is not bad */
    const float*   mp2_xw;       /* total_kp2 x 3 */
    const float*   s12;          /* n_pairs x 13: R12 (row-major 3x3), t12, s */
    const int32_t* match12;      /* total_kp1: keyframe-2-relative index of matches1[i] or -1 */
    int32_t        n_levels;
    const float*   inv_level_sigma2; /* host, n_levels (pyramid.invSigmaSq) */
    float          max_chi2;
    int32_t        fix_scale;    /* per batch */
} orbba_sim3_batch;

typedef struct orbba_sim3_result {
    float*   s12;        /* n_pairs x 13: S12 on return; the input row when the pair returns 0 */
    double*  s12_g2o;    /* n_pairs x 8: q (x, y, z, w), t, s of the vertex estimate when the call returned;
                          * may be NULL */
    int32_t* match12;    /* total_kp1: the thinned matches; may alias the input */
    int32_t* n_inliers;  /* n_pairs: the return value; -1 from the device entry for a pair with more than
                          * ORBBA_SIM3_MAX_CORR correspondences (its s12 and match12 are the input's) */
    int32_t* iterations; /* n_pairs x 2: LM iterations of the two optimize() calls; may be NULL */
} orbba_sim3_result;

/* Host entry: every pointer is host memory, synchronous; offsets, octaves and the range of match12 are
 * validated; a pair with more than ORBBA_SIM3_MAX_CORR correspondences is refused. */
int orbba_optimize_sim3(const orbba_sim3_batch* in, orbba_sim3_result* out, int device);
/* Device entry: every array in HBM except inv_level_sigma2; enqueue only on `stream`.  One wavefront per
 * pair. */
int orbba_optimize_sim3_device(const orbba_sim3_batch* in, orbba_sim3_result* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * void Optimizer::OptimizeEssentialGraph(Map* map, KeyFrame* loopKF, KeyFrame* currKF, const KeyFrameAndPose&
 * nonCorrectedSim3, const KeyFrameAndPose& correctedSim3, const LoopConnections& loopConnections, bool fixScale)
 * (include/Optimizer.h, src/Optimizer.cc:743-942; LoopClosing::CorrectLoop) on slot tables: slot k is the k-th
 * keyframe that is not bad, in map->GetAllKeyFrames() order.
 * Vertices (:761-796): one VertexSim3Expmap per slot, estimate ToG2OSim3(vertex_sim3[k]) (:183-188: widened, the
 * rotation through Quaterniond(R)), where vertex_sim3[k] is the keyframe's correctedSim3 entry or Sim3(pose) with
 * scale 1 (the reference's nonCorrectedScw table).  fixed_slot (loopKF) is fixed; _fix_scale = fix_scale.
 * Edges (:798-903): EdgeSim3 with information I7, vertex 0 = edge_i, vertex 1 = edge_j, in the reference's
 * insertion order (orbba_essential_graph_edges builds the list).  Measurement Sji = Sjw * Swi in the float Sim3
 * class (include/Sim3.h:40-63), then ToG2OSim3; both ends read vertex_sim3 when edge_table[e] == 0 (loop
 * connections) and edge_sim3 otherwise (edge_sim3[k]: the nonCorrectedSim3 entry, or the vertex_sim3 row).
 * Error log(C * v1 * v2^-1) (types_seven_dof_expmap.h:106-114, sim3.h:148-230 with its four branches, W.lu() as
 * a partially pivoted LU); Jacobians by g2o's central differences at delta = 1e-9
 * (base_binary_edge.hpp:131-205), so under fix_scale every scale column is exactly 0.
 * Solver: BlockSolver_7_3 with nothing marginalised, so each trial solves the dense (H + lambda I) x = b of the
 * active free vertices (a slot with no edge is never activated and keeps its estimate) by an unpivoted blocked
 * LDL^T (a zero or non-finite pivot rejects the trial); Levenberg with lambda0 = 1e-16 (Optimizer.cc:749),
 * optimize(20), no robust kernel, the rho / nu / ten-trial / nBad rules of orbba_local_ba.  chi2, H and b are
 * summed edge by edge in insertion order without atomics: two runs are bit-identical.
 * Recovery (:911-941): pose[k] = (R, (1. / s) * t) of FromG2OSim3(estimate) with the product in double; a point
 * with point_ref[p] = r >= 0 becomes (correctedSwc[r] * vertex_sim3[r]).Map(P) in float; point_ref = -1 (a bad
 * point) copies the point.  point_ref is correctedReference where correctedByKF == currKF->id, else the
 * reference keyframe.  UpdateNormalAndDepth is not part of this call.
 * Size: the system is dense, 7 ORBBA_EG_MAX_KEYFRAMES unknowns at most (103 MB for H, as much for its factor);
 * a larger map is refused. */
#define ORBBA_EG_MAX_KEYFRAMES 512
#define ORBBA_EG_MAX_TRIALS 200   /* 20 iterations x 10 trials */

typedef struct orbba_essential_graph {
    int32_t        n_keyframes;
    const float*   vertex_sim3;  /* n_keyframes x 13: R (row-major 3x3), t, s of the vertex table */
    const float*   edge_sim3;    /* n_keyframes x 13: the edge-side table */
    int32_t        fixed_slot;   /* loopKF */
    int32_t        fix_scale;
    int32_t        n_edges;
    const int32_t* edge_i;       /* n_edges: vertex 0 */
    const int32_t* edge_j;       /* n_edges: vertex 1 */
    const uint8_t* edge_table;   /* n_edges: 0 = both ends from vertex_sim3, 1 = from edge_sim3 */
    int32_t        n_points;
    const float*   points;       /* n_points x 3 */
    const int32_t* point_ref;    /* n_points: reference slot, -1 = skip */
} orbba_essential_graph;

typedef struct orbba_essential_graph_result {
    double*  sim3_g2o;     /* n_keyframes x 8: q (x, y, z, w), t, s of the optimised vertices */
    float*   pose;         /* n_keyframes x 12: Rcw (row-major 3x3) then tcw */
    float*   points;       /* n_points x 3 */
    double*  measurement;  /* n_edges x 8: the edges' measurements as g2o holds them; may be NULL */
    int32_t* iterations;   /* 2: LM iterations run, trials run */
    double*  chi2;         /* 1: the final chi2 */
    uint8_t* accept;       /* ORBBA_EG_MAX_TRIALS: 1 = the trial was accepted, in order; the rest 0 */
} orbba_essential_graph_result;

/* Host entry: every pointer is host memory, synchronous.  ORB_EINVAL before any device call for null pointers,
 * n_keyframes < 1 or > ORBBA_EG_MAX_KEYFRAMES, fixed_slot out of range, edge_i == edge_j, an index out of range
 * (edges, point_ref < -1 or >= n_keyframes), a scale <= 0 and non-finite input. */
int orbba_optimize_essential_graph(const orbba_essential_graph* in, orbba_essential_graph_result* out, int device);
/* Device entry: every array in HBM; enqueue only on `stream`, nothing is copied back.  Sizes, fixed_slot and
 * null pointers are checked; an edge whose indices are out of range or equal is left out of the graph and a
 * point_ref out of range copies its point.  The workspace (the control struct, H, its factor) belongs to the calling
 * thread and is reused by its next call: calls from one thread must be stream-ordered (the same stream, or an
 * event between them); threads are independent of each other. */
int orbba_optimize_essential_graph_device(const orbba_essential_graph* in, orbba_essential_graph_result* out,
                                          void* stream);

/* orbba_optimize_essential_graph with the device time of each kernel, summed over its launches, in kernel_ms
 * (ORBBA_EG_KERNELS floats: setup, measure, linearize, assemble, begin, stage, solve, update, chi, ctl, recover).
 * An event pair and a wait surround every launch, so the call itself is slower; for tools/time_essential_graph.py. */
#define ORBBA_EG_KERNELS 11
int orbba_essential_graph_profile(const orbba_essential_graph* in, orbba_essential_graph_result* out, int device,
                                  float* kernel_ms);

/* The edge list of Optimizer.cc:798-903 from slot tables (host only, no device call).  Loop connections first
 * (:802-828, edge_table 0), in the order given: connection c is keyframe conn_kf[c] with the keyframes
 * conn_slot[conn_begin[c] .. conn_begin[c + 1]); one is kept if it is (curr_slot, loop_slot) or its covisibility
 * weight is >= min_weight, and enters insertedEdges.  Then per slot in order (:831-903, edge_table 1): the
 * spanning-tree edge to parent[k] (-1: none), the loop edges with a smaller kf_id, and the covisibility row
 * (GetCovisiblesByWeight order) with weight >= min_weight, leaving out the parent, a child (a slot whose parent
 * is k), a loop edge, a slot of -1 (bad), a kf_id not smaller than the keyframe's and a pair in insertedEdges.
 * Writes at most `capacity` edges and always the full count to *n_edges. */
typedef struct orbba_eg_tables {
    int32_t        n_keyframes;
    const int32_t* kf_id;        /* n_keyframes: KeyFrame::id */
    const int32_t* parent;       /* n_keyframes: slot or -1 */
    const int32_t* loop_begin;   /* n_keyframes + 1 */
    const int32_t* loop_slot;    /* GetLoopEdges() in iteration order */
    const int32_t* covis_begin;  /* n_keyframes + 1 */
    const int32_t* covis_slot;   /* the ordered connected keyframes; -1 for a bad one */
    const int32_t* covis_weight;
    int32_t        n_connections;
    const int32_t* conn_kf;      /* n_connections */
    const int32_t* conn_begin;   /* n_connections + 1 */
    const int32_t* conn_slot;
    int32_t        curr_slot, loop_kf_slot;
} orbba_eg_tables;
int orbba_essential_graph_edges(const orbba_eg_tables* g, int32_t min_weight, int32_t capacity, int32_t* edge_i,
                                int32_t* edge_j, uint8_t* edge_table, int32_t* n_edges);

/* ------------------------------------------------------------------------------------------
 * Sim3Solver(keyframe1, keyframe2, matches, fixScale), SetRansacParameters(probability, minInliers,
 * maxIterations) and bool Sim3Solver::iterate(int maxk, Sim3& sim3, std::vector<bool>& isInlier)
 * (include/Sim3Solver.h, src/Sim3Solver.cc:206-365; LoopClosing::FindLoopInCandidateKFs, LoopClosing.cc:105-135:
 * 0.99, 20, 300, iterate(5)), batched over (keyframe1, keyframe2) pairs in orbm_sim3_batch's slot layout, so
 * orbm_search_by_bow_kf_batch_device's match12 feeds straight in and the outputs feed orbm_search_by_sim3_device
 * and orbba_optimize_sim3_device.
 * Correspondences (:225-255): slot i1 of keyframe 1, ascending, is kept iff mp1_valid[i1] && match12[i1] >= 0 &&
 * mp2_valid[match12[i1]]; i1 stands for GetIndexInKeyFrame(keyframe1) and match12[i1] for
 * GetIndexInKeyFrame(keyframe2), the convention of orbba_optimize_sim3.  Per kept correspondence, in float:
 * Xc1 = R1w * Xw1 + t1w, Xc2 = R2w * Xw2 + t2w, points{1,2} = FromCameraToImage(Xc{1,2}) (invZ = 1 / z,
 * fx * (x * invZ) + cx; :186-204), and in double maxErrorSq{1,2} = 9.21 * (double)level_sigma2[octave].  The
 * keypoint positions are not read (kp1_xy, kp2_xy and s12 keep orbba_sim3_batch's layout and may be NULL).
 * Iteration cap (:266-287): with nmatches the kept count, epsilon = 1.f * min_inliers / nmatches (float),
 * niterations = 1 when min_inliers == nmatches, else ceil(log(1 - probability) / log(1 - pow(epsilon, 3))) in
 * double, cap = max(1, min(niterations, max_iterations)) (compared in double before narrowing to int).  The
 * host computes cap for every nmatches in 0 .. ORBM_PROJ_MAX_KP with libm and the kernel indexes that table.
 * Sampling (:307-322): DUtils::Random::RandomInt is libc rand(), so the draws are an input: hypothesis k of
 * pair p uses draws[p, k, 0..2], raw rand() values in [0, rand_max]; draw c picks position
 * int(((double)r / ((double)rand_max + 1.0)) * (nmatches - c)) of the available indices, which is then refilled
 * from the back and popped (three draws without replacement).  A result therefore does not depend on how the
 * iterations are split over calls.  The reference interleaves one global rand() stream over the candidates in
 * round-robin order; a table per pair is statistically the same and not a replay of a particular CPU run.
 * Hypothesis (ComputeSim3, :111-163), float unless said: centroids ((P(i,0) + P(i,1)) + P(i,2)) / 3.f;
 * M = Pr2 * Pr1^T with ((a0 b0 + a1 b1) + a2 b2); R12 = U S Vh of svd(M^T) with S(2,2) = -1 when
 * det(U) det(Vh) < 0, computed in fp64 from the float M as Horn's unit quaternion (the same proper rotation,
 * DESIGN.md section 4) and rounded to float; P3 = R12 * Pr2; s12 = (float)(nom / den), nom = Pr1.dot(P3) with
 * products and sum in double, den = the float products P3(i,j) * P3(i,j) added to a double, both row-major; 1
 * exactly with fix_scale; t12 = O1 - (s12 * R12) * O2; S21 = S12.Inverse() (Sim3.h:43-47: R21 = R12^T,
 * t21 = ((-(1 / s)) * R12^T) * t12, s21 = 1 / s).
 * Scoring (:327-344): proj1 = Project(Xc2, S12, camera1), proj2 = Project(Xc1, S21, camera2) with Sim3::Map
 * ((s * R) * x + t), invZ = 1.f / z and no depth test; errorSq = dx * dx + dy * dy in float, widened, and a
 * correspondence is an inlier iff errorSq1 < maxErrorSq1 && errorSq2 < maxErrorSq2 (IEEE: a zero or negative
 * depth gives inf or NaN, never an inlier).  n[k] = the inlier count of hypothesis k.
 * Control (:289-365), per pair, on the state (iterations, max_inliers) that the call reads and writes:
 * nmatches < min_inliers: terminate = 1, found = 0, the state unchanged.  Otherwise k runs over
 * [iterations, min(iterations + maxk, cap)); k updates iff n[k] >= max_inliers (then max_inliers = n[k]) and
 * succeeds iff it updates and n[k] > min_inliers.  At the first success: found = 1, iterations = k + 1, s12 =
 * that hypothesis, inlier[i1] = 1 for the slots of its inliers, match12[i1] = the input's for those slots and
 * -1 elsewhere (LoopClosing.cc:133-135), n_inliers = n[k].  Without one: found = 0, iterations =
 * min(iterations + maxk, cap), terminate = (iterations >= cap), n_inliers = 0, and the pair's inlier is 0,
 * its match12 -1 and its s12 row 0 everywhere (iterate() clears isInlier on entry; nothing is left unwritten). */
typedef struct orb_sim3solver_batch {
    int32_t        n_pairs, total_kp1, total_kp2;
    const int32_t* kp1_begin;    /* n_pairs + 1 */
    const int32_t* kp2_begin;    /* n_pairs + 1 */
    const float*   kp1_xy;       /* not read; may be NULL */
    const int32_t* kp1_octave;   /* total_kp1 */
    const float*   kp2_xy;       /* not read; may be NULL */
    const int32_t* kp2_octave;   /* total_kp2 */
    const float*   pose1;        /* n_pairs x 12: Rcw (row-major 3x3) then tcw */
    const float*   camera1;      /* n_pairs x 4: fx, fy, cx, cy */
    const float*   pose2;
    const float*   camera2;
    const uint8_t* mp1_valid;    /* total_kp1: mappoints1[i] && !mappoints1[i]->isBad() */
    const float*   mp1_xw;       /* total_kp1 x 3 */
    const uint8_t* mp2_valid;    /* total_kp2: the map point of slot i2 exists and is not bad */
    const float*   mp2_xw;       /* total_kp2 x 3 */
    const float*   s12;          /* not read; may be NULL */
    const int32_t* match12;      /* total_kp1: keyframe-2-relative index of matches[i1] or -1 */
    int32_t        n_levels;
    const float*   level_sigma2; /* host, n_levels (pyramid.sigmaSq) */
    int32_t        fix_scale;    /* per batch */
    const int32_t* draws;        /* n_pairs x max_iterations x 3: rand() values in [0, rand_max] */
    int32_t        rand_max;     /* RAND_MAX of the generator that made draws (glibc: 2147483647) */
    double         probability;  /* SetRansacParameters; in (0, 1) */
    int32_t        min_inliers;  /* >= 3 */
    int32_t        max_iterations; /* >= 1 */
    int32_t        maxk;         /* iterate(maxk); >= 1 */
} orb_sim3solver_batch;

typedef struct orb_sim3solver_result {
    float*   s12;          /* n_pairs x 13: R12 (row-major 3x3), t12, s of the successful hypothesis, else 0 */
    uint8_t* inlier;       /* total_kp1: isInlier */
    int32_t* match12;      /* total_kp1: inlier[i1] ? the input's match12[i1] : -1; must not alias the input */
    int32_t* found;        /* n_pairs: iterate()'s return value; -1 from the device entry for a pair either of
                            * whose keyframes has more than ORBM_PROJ_MAX_KP keypoints (its state unchanged,
                            * terminate 1, the other outputs as without a success) */
    int32_t* n_inliers;    /* n_pairs: the successful hypothesis's inlier count, else 0 */
    int32_t* iterations;   /* n_pairs, in / out: iterations_ (0 for a fresh solver) */
    int32_t* max_inliers;  /* n_pairs, in / out: maxInliers_ (0 for a fresh solver) */
    int32_t* terminate;    /* n_pairs: terminate() */
    int32_t* hyp_inliers;  /* n_pairs x max_iterations: n[k] of the hypotheses the reference would have
                            * evaluated in this call, -1 elsewhere; may be NULL */
} orb_sim3solver_result;

/* Host entry: every pointer is host memory, synchronous; offsets, octaves, the range of match12, the state and
 * draws in [0, rand_max] are validated before anything is copied; a keyframe with more than ORBM_PROJ_MAX_KP
 * keypoints is refused. */
int orb_sim3solver_iterate(const orb_sim3solver_batch* in, orb_sim3solver_result* out, int device);
/* Device entry: every array in HBM except level_sigma2; enqueues only on `stream` (the first call with a new
 * (probability, min_inliers, max_iterations) uploads its cap table synchronously, as the first call allocates
 * the workspace).  A draw outside [0, rand_max] is clamped to a valid position.  One lane per hypothesis. */
int orb_sim3solver_iterate_device(const orb_sim3solver_batch* in, orb_sim3solver_result* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * PnPsolver(Frame, matches), SetRansacParameters(probability, minInliers, maxIterations, minSet, epsilon, th2)
 * and cv::Mat PnPsolver::iterate(int nIterations, bool& bNoMore, vector<bool>& vbInliers, int& nInliers)
 * (include/PnPsolver.h, src/PnPsolver.cc; Tracking::Relocalization, Tracking.cc:336-362: 0.99, 10, 300, 4, 0.5f,
 * 5.991f, iterate(5)), batched over candidate keyframes: one solver per frame slot range, in the layout of
 * orbm_reloc_batch / orbba_pose_batch, so orbm_search_by_bow_batch_device's matches feed in (as mp_valid, mp_xw)
 * and tcw / inlier feed orbba_pose_optimization_device.
 * Correspondences (:79-101): the slots i with mp_valid[i], ascending; P2D = kp_xy[i], P3Dw = mp_xw[i],
 * maxError = level_sigma2[octave] * th2, all float.  N is their count.
 * SetRansacParameters (:121-157): minInliers = max(int(N * epsilon), min_inliers, min_set), eps = max(epsilon,
 * (float)minInliers / N), cap = 1 when minInliers == N, else ceil(log(1 - probability) / log(1 - pow(eps, 3)))
 * in double, clamped to [1, max_iterations] (compared in double before narrowing).  The host computes cap for
 * every N in 0 .. ORBM_PROJ_MAX_KP with libm and the kernel indexes that table.
 * Draws (:191-201): hypothesis k of candidate p uses draws[p, k, 0..3], raw rand() values in [0, rand_max]; draw
 * c picks position int(((double)r / ((double)rand_max + 1.0)) * (N - c)) of the available indices, which is then
 * refilled from the back and popped.  A result does not depend on how the iterations are split over calls.
 * Hypothesis: EPnP (compute_pose, :477-526) in fp64 on the four correspondences, then CheckInliers (:308-339)
 * with the reference's mix of float and double and the strict float <.  Where the reference reads an OpenCV SVD
 * whose rounding decides the answer, a rule of the data stands instead (PnPsolver).
 * Control (:165-258), per candidate, on the state (iterations, best_inliers, best_mask, best_tcw) that the call
 * reads and writes.  N < minInliers: terminate = 1, found = 0, the state unchanged.  Otherwise k runs over
 * [iterations, max(cap, iterations + maxk)) -- the reference's loop condition is an OR, so a fresh solver runs
 * its whole cap in one call and an exhausted one maxk more.  A hypothesis with n[k] >= minInliers replaces the
 * best when n[k] > best_inliers, and then Refine() (EPnP over the best inliers, CheckInliers) succeeds when its
 * count is > minInliers: found = 1, tcw / inlier / n_inliers are the refined ones, iterations = k + 1.  Without a
 * success iterations = the end of the range, terminate = (iterations >= cap), and with terminate and
 * best_inliers >= minInliers found = 2 and tcw / inlier / n_inliers are the best (unrefined) ones.  Otherwise
 * found = 0 and tcw, inlier and n_inliers are 0 (nothing is left unwritten). */
typedef struct orb_pnpsolver_batch {
    int32_t        n_frames, total_kp;
    const int32_t* kp_begin;     /* n_frames + 1 */
    const float*   kp_xy;        /* total_kp x 2: keypointsUn */
    const int32_t* kp_octave;    /* total_kp */
    const float*   camera;       /* n_frames x 4: fx, fy, cx, cy */
    const uint8_t* mp_valid;     /* total_kp: vpMapPointMatches[i] && !isBad() */
    const float*   mp_xw;        /* total_kp x 3 */
    int32_t        n_levels;
    const float*   level_sigma2; /* host, n_levels (pyramid.sigmaSq) */
    const int32_t* draws;        /* n_frames x n_draws x 4: rand() values in [0, rand_max] */
    int32_t        n_draws;      /* >= the end of the range of every candidate */
    int32_t        rand_max;     /* RAND_MAX of the generator that made draws (glibc: 2147483647) */
    double         probability;  /* in (0, 1) */
    int32_t        min_inliers;  /* >= 6 (a departure: Refine on five points has a two-dimensional null space) */
    int32_t        max_iterations; /* >= 1 */
    int32_t        min_set;      /* 4 */
    float          epsilon;      /* in [0, 1] */
    float          th2;          /* > 0 */
    int32_t        maxk;         /* iterate(nIterations); >= 1 */
} orb_pnpsolver_batch;

typedef struct orb_pnpsolver_result {
    float*   tcw;          /* n_frames x 12: Rcw (row-major 3x3) then tcw, 0 when nothing is returned */
    uint8_t* inlier;       /* total_kp: vbInliers, in keypoint slots */
    int32_t* found;        /* n_frames: 1 refined, 2 best at termination, 0 none; -1 from the device entry for a
                            * candidate with more than ORBM_PROJ_MAX_KP keypoints or whose range would pass
                            * n_draws (its state unchanged, terminate 1, the other outputs 0) */
    int32_t* n_inliers;    /* n_frames: nInliers */
    int32_t* terminate;    /* n_frames: bNoMore */
    int32_t* iterations;   /* n_frames, in / out: mnIterations (0 for a fresh solver) */
    int32_t* best_inliers; /* n_frames, in / out: mnBestInliers (0 for a fresh solver) */
    uint8_t* best_mask;    /* total_kp, in / out: mvbBestInliers in keypoint slots */
    float*   best_tcw;     /* n_frames x 12, in / out: mBestTcw */
    int32_t* hyp_inliers;  /* n_frames x n_draws: n[k] of the hypotheses the reference would have evaluated in
                            * this call, -1 elsewhere; may be NULL */
} orb_pnpsolver_result;

/* Host entry: every pointer is host memory, synchronous; offsets, octaves, the state, the length of the draw
 * table and draws in [0, rand_max] are validated before anything is copied; a frame with more than
 * ORBM_PROJ_MAX_KP keypoints is refused. */
int orb_pnpsolver_iterate(const orb_pnpsolver_batch* in, orb_pnpsolver_result* out, int device);
/* Device entry: every array in HBM except level_sigma2; enqueues only on `stream` (the first call with a new
 * parameter set uploads its cap table synchronously, as the first call allocates the workspace).  A draw outside
 * [0, rand_max] is clamped to a valid position.  One lane per hypothesis, one wavefront per Refine().
 * The workspace (records, ranges, hypothesis poses) is one per host thread and shared by every stream that
 * thread enqueues on: two calls from one thread on different streams need an event or a synchronise between
 * them, as with orb_sim3solver_iterate_device. */
int orb_pnpsolver_iterate_device(const orb_pnpsolver_batch* in, orb_pnpsolver_result* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Initializer(ReferenceFrame, sigma, iterations) and bool Initializer::Initialize(CurrentFrame, vMatches12, R21,
 * t21, vP3D, vbTriangulated) (include/Initializer.h, src/Initializer.cc:45-122; Tracking::MonocularInitialization,
 * Tracking.cc:1033-1075), batched over (reference frame, current frame) pairs: frame 1 of pair p holds the slots
 * [kp1_begin[p], kp1_begin[p+1]) of kp1_xy (keypointsUn), frame 2 likewise, and matches12 is what
 * orbm_search_for_initialization* writes (the frame-2-relative index of slot i's match, -1 for none).
 * mvMatches12 (:55-64): the slots with matches12[i] >= 0, ascending; N is their count.  Normalize (:750-796) runs
 * over all keypoints of either frame in float (summation order: csrc/orbinit.hip).
 * Draws (:83-98): hypothesis `it` of pair p uses draws[p, it, 0..7], raw rand() values in [0, rand_max]; draw j
 * picks position int(((double)r / ((double)rand_max + 1.0)) * (N - j)) of the available indices, which is then
 * refilled from the back and popped.  The same eight indices serve the homography and the fundamental matrix.
 * Hypotheses: ComputeH21 / ComputeF21 (:227-304) under rules of the data in fp64 (csrc/init_hyp.h, DESIGN.md
 * section 4, Initializer), H21i / H12i / F21i rounded to float; CheckHomography / CheckFundamental (:306-469) in
 * the reference's float expressions and summation order.  The winner of either model is the first maximum of the
 * scores (currentScore > score from 0); a model none of whose scores is positive has best = -1, a zero matrix and
 * an empty mask.  RH = SH / (SH + SF) in float picks ReconstructH (RH > rh_threshold) or ReconstructF (:113-119).
 * ReconstructF (:471-571) tries (R1, t), (R2, t), (R1, -t), (R2, -t) of DecomposeE, ReconstructH (:573-733)
 * Faugeras' eight hypotheses, each through CheckRT (:799-908) with the reference's tests and types; the decision
 * rules are the reference's.  Departures: N < 8 evaluates nothing (found = 0; the reference would draw from an
 * empty vector); parallax is the element of rank min(50, nGood - 1) with ties broken by correspondence index. */
typedef struct orb_initializer_batch {
    int32_t        n_pairs, total_kp1, total_kp2;
    const int32_t* kp1_begin;    /* n_pairs + 1 */
    const int32_t* kp2_begin;    /* n_pairs + 1 */
    const float*   kp1_xy;       /* total_kp1 x 2: the reference frame's keypointsUn */
    const float*   kp2_xy;       /* total_kp2 x 2: the current frame's keypointsUn */
    const int32_t* matches12;    /* total_kp1 */
    const float*   camera;       /* n_pairs x 4: fx, fy, cx, cy */
    const int32_t* draws;        /* n_pairs x max_iterations x 8: rand() values in [0, rand_max] */
    int32_t        rand_max;     /* RAND_MAX of the generator that made draws (glibc: 2147483647) */
    float          sigma;        /* > 0 (1.0) */
    int32_t        max_iterations; /* >= 1 (200) */
    float          min_parallax; /* degrees (1.0) */
    int32_t        min_triangulated; /* (50) */
    double         rh_threshold; /* (0.40) */
} orb_initializer_batch;

typedef struct orb_initializer_result {
    int32_t* found;        /* n_pairs: 1 initialised, 0 not; -1 from the device entry for a pair either of whose
                            * frames has more than ORBM_PROJ_MAX_KP keypoints (every other output of the pair 0) */
    int32_t* model;        /* n_pairs: 0 = ReconstructH, 1 = ReconstructF was tried */
    float*   r21t21;       /* n_pairs x 12: R21 (row-major 3x3) then t21; 0 without a success */
    float*   p3d;          /* total_kp1 x 3: vP3D in reference-frame keypoint slots; 0 without a success */
    uint8_t* triangulated; /* total_kp1: vbTriangulated */
    float*   score_h;      /* n_pairs: SH */
    float*   score_f;      /* n_pairs: SF */
    int32_t* best_h;       /* n_pairs: the winning `it` of FindHomography, -1 for none */
    int32_t* best_f;       /* n_pairs: of FindFundamental */
    float*   h21;          /* n_pairs x 9 */
    float*   f21;          /* n_pairs x 9 */
    uint8_t* inlier_h;     /* total_kp1: vbMatchesInliersH in keypoint slots */
    uint8_t* inlier_f;     /* total_kp1: vbMatchesInliersF */
    float*   hyp_score;    /* n_pairs x 2 x max_iterations: currentScore of every hypothesis, H then F */
    int32_t* n_good;       /* n_pairs x 8: nGood of every motion hypothesis (4..7 are 0 on the F path) */
    float*   parallax;     /* n_pairs x 8: its parallax in degrees */
} orb_initializer_result;

/* Host entry: every pointer is host memory, synchronous; offsets, matches12 in [-1, keypoints of frame 2), draws in
 * [0, rand_max] and the scalars are validated before anything is copied; a frame with more than ORBM_PROJ_MAX_KP
 * keypoints is refused. */
int orb_initializer_initialize(const orb_initializer_batch* in, orb_initializer_result* out, int device);
/* Device entry: every array in HBM; enqueues only on `stream` (the first call allocates the workspace).  A draw
 * outside [0, rand_max] is clamped to a valid position and a match outside frame 2 is ignored.  One lane per
 * hypothesis.  The workspace is one per host thread and shared by every stream that thread enqueues on, as with
 * orb_pnpsolver_iterate_device. */
int orb_initializer_initialize_device(const orb_initializer_batch* in, orb_initializer_result* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:380-578) on extractor slots, batched over
 * (keyframe 1, keyframe 2) pairs.  Three steps, each with a device and a host form:
 *   orblm_prepare_pairs           per pair: Ow1, Ow2, the baseline, ComputeF12 (:55-71), the epipole
 *                                 (src/ORBmatcher.cc:772-773) and the skip rule (:410-422: stereo
 *                                 baseline < camera2.baseline; monocular baseline / ComputeSceneMedianDepth(2)
 *                                 < 0.01f, src/KeyFrame.cc:522-552).  F12 / ep2 are what
 *                                 orbm_search_for_triangulation_batch_device reads, in its layout.
 *   orblm_triangulate             per match of that search's match12 (:437-560): the parallax test, linear
 *                                 triangulation or uvZToWorld of either frame, the depth signs, both
 *                                 reprojection gates, the scale gate; a status per keypoint of keyframe 1,
 *                                 the created points compacted in ascending idx1 (the reference's creation
 *                                 order) with what UpdateNormalAndDepth (src/MapPoint.cc:341-380) gives
 *                                 them, and optionally the MapPoint flags of both keyframes set in place.
 *   orblm_create_new_map_points   the neighbour loop: n_rounds x n_pairs plan entries; prepare once, then
 *                                 per round the search followed by the triangulation with writable flags,
 *                                 so that a point created against neighbour i hides its keypoints from the
 *                                 search against neighbour i + 1, as keyframe1->GetMapPoint(idx1) does.
 * All float arithmetic follows one fixed operation order (csrc/lm_newpoint.h), so F12, ep2, the baseline and
 * the median are reproducible bit for bit.  Departure: a monocular pair whose keyframe 2 has no MapPoint is
 * skipped (the reference indexes an empty vector).
 * ---------------------------------------------------------------------------------------- */
#define ORBLM_MAX_KP 8192          /* cap2 at most, where the median is taken (monocular) */
enum {
    ORBLM_CREATED = 0,             /* :562: the point is created */
    ORBLM_NO_MATCH = 1,            /* match12[idx1] < 0 (or not a keypoint of keyframe 2) */
    ORBLM_PAIR_SKIPPED = 2,        /* :410-422: a match of a skipped pair */
    ORBLM_LOW_PARALLAX = 3,        /* :502 */
    ORBLM_W_ZERO = 4,              /* :485: v(3) == 0 */
    ORBLM_BEHIND1 = 5,             /* :507: Xc1.z <= 0 */
    ORBLM_BEHIND2 = 6,             /* :507: Xc2.z <= 0 */
    ORBLM_REPROJ1 = 7,             /* :514-525 */
    ORBLM_REPROJ2 = 8,             /* :531-542 */
    ORBLM_DIST_ZERO = 9,           /* :551 */
    ORBLM_SCALE = 10               /* :559 */
};
enum { ORBLM_BRANCH_NONE = 0, ORBLM_BRANCH_TRIANGULATED = 1, ORBLM_BRANCH_STEREO1 = 2, ORBLM_BRANCH_STEREO2 = 3 };

typedef struct orblm_batch {
    int32_t n_pairs;                 /* pairs of one call; pairs per round for orblm_create_new_map_points */
    int32_t cap1, cap2;              /* slots per keyframe of set 1 / set 2 (sets may be the same arrays) */
    int32_t n_frames1, n_frames2;    /* keyframes in set 1 / set 2 */
    const orbx_keypoint* kps1; const int32_t* counts1;   /* keypointsUn slots, as orbm_tri_batch */
    const float* uright1; const float* depth1;            /* per slot; NULL: every keypoint monocular */
    const orbx_keypoint* kps2; const int32_t* counts2;
    const float* uright2; const float* depth2;
    const uint8_t* has_mappoint2;    /* per slot of set 2: GetMapPoint(idx) != nullptr; monocular only */
    const float* mp_xw2;             /* per slot of set 2 x 3: that MapPoint's GetWorldPos(); monocular only */
    const float* pose1; const float* pose2;       /* per keyframe 12: Tcw as 3 x 4 row-major */
    const float* camera1; const float* camera2;   /* per keyframe 6: fx, fy, cx, cy, bf, baseline */
    const int32_t* frame1; const int32_t* frame2; /* per pair: keyframe of set 1 / set 2; negative: no pair */
    int32_t n_levels;                /* <= ORBM_TRI_MAX_LEVELS */
    const float* scale_factors1; const float* sigma2_1;   /* host, n_levels: keyframe 1's pyramid */
    const float* scale_factors2; const float* sigma2_2;   /* host, n_levels: keyframe 2's pyramid */
    float scale_factor;              /* keyframe1->pyramid.scaleFactor (ratioFactor = 1.5f x this) */
    int32_t monocular;               /* which skip rule (:410) */
} orblm_batch;

/* What prepare writes and the other steps read, per pair (all required). */
typedef struct orblm_pairs {
    float* F12;            /* x 9 */
    float* ep2;            /* x 2 */
    float* baseline;
    float* median;         /* medianDepthKF2 (0 where it is not taken) */
    int32_t* skip;         /* 0 go on, 1 skipped by the rule, 2 no pair */
    int32_t* frame1;       /* the pair's keyframes, 0 for "no pair": always valid indices for the search */
    int32_t* frame2;
    float* consts;         /* x 64: both keyframes' Tcw, Rwc, Ow and camera */
} orblm_pairs;

/* Per pair p and keypoint idx1 of keyframe 1, at p*cap1 + idx1 (written for idx1 < counts1). */
typedef struct orblm_points {
    int32_t* status;       /* ORBLM_* */
    int32_t* branch;       /* ORBLM_BRANCH_* */
    float* xw;             /* x 3: Xw where a branch was taken */
    float* normal;         /* x 3, of a created point */
    float* min_distance; float* max_distance;
    int32_t* new_idx1;     /* k < n_created[p]: the created points in ascending idx1; -1 after them */
    int32_t* new_idx2;
    int32_t* n_created;    /* per pair */
    uint8_t* has_mappoint1;/* per slot of set 1 / set 2: a created point sets its two flags; NULL: nothing */
    uint8_t* has_mappoint2;/* is written (orblm_create_new_map_points needs both) */
} orblm_points;

/* Device forms: every array in HBM but the pyramid tables; enqueue only on `stream`.  A pair whose frame
 * index is negative or not below n_frames1 / n_frames2 is "no pair": n_created = 0, nothing else written. */
int orblm_prepare_pairs_device(const orblm_batch* b, const orblm_pairs* pairs, void* stream);
/* d_match12[p*cap1 + idx1] as orbm_search_for_triangulation_batch_device leaves it. */
int orblm_triangulate_device(const orblm_batch* b, const orblm_pairs* pairs, const int32_t* d_match12,
                             const orblm_points* out, void* stream);
/* The neighbour loop.  Plan entry (r, j) = (b->frame1[r*n_pairs + j], b->frame2[...]); every per-pair array of
 * `pairs`, `out`, d_match12 and d_nmatches holds n_rounds*n_pairs pairs.  `search` gives what the search needs
 * beyond `b` (desc1, desc2, the FeatureVectors, only_stereo, keyframe 2's tables); its slot arrays must be b's,
 * its pair arrays and flags are replaced per round.  Precondition, not checked here (the plan is device
 * memory): within one round all frame1 are distinct, all frame2 are distinct and, where the two sets are the
 * same arrays, no keyframe is both; otherwise two pairs write one keyframe's flags.  Only enqueues: no
 * synchronisation, no copy.  A caller that wants CheckNewKeyFrames() between neighbours (:401) enqueues round
 * by round with the search and orblm_triangulate_device instead. */
int orblm_create_new_map_points_device(const orblm_batch* b, const orbm_tri_batch* search, int32_t n_rounds,
                                       const orblm_pairs* pairs, const orblm_points* out, int32_t* d_match12,
                                       int32_t* d_nmatches, void* stream);
/* Host forms: every pointer is host memory, synchronous; shapes, counts, octaves and the plan's precondition are
 * validated before anything is copied.  out->has_mappoint1 / 2 are read and updated.
 * orblm_create_new_map_points takes a search without FeatureVectors (one node holding every keypoint). */
int orblm_prepare_pairs(const orblm_batch* b, const orblm_pairs* pairs, int device);
int orblm_triangulate(const orblm_batch* b, const orblm_pairs* pairs, const int32_t* match12, const orblm_points* out,
                      int device);
int orblm_create_new_map_points(const orblm_batch* b, const orbm_tri_batch* search, int32_t n_rounds,
                                const orblm_pairs* pairs, const orblm_points* out, int32_t* match12, int32_t* nmatches,
                                int device);

/* ------------------------------------------------------------------------------------------
 * KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:34-265) resident in HBM: add / erase /
 * clear, DetectLoopCandidates (:68-171) and DetectRelocalizationCandidates (:173-265) batched over query frames,
 * and the minScore loop of LoopDetector::Detect (src/LoopClosing.cc:170-178).  voc_->score is L1Scoring::score
 * (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), the only scoring supported.
 *
 * A keyframe is a slot k in [0, max_keyframes): the host's index for its KeyFrame*.  A slot holds a live flag,
 * its BowVector (word ids ascending, fp64 weights, at most word_cap entries, as orbv_transform* emits them) and
 * one persistent float, reloc_score (KeyFrame::relocScore; the reference never initialises it, add sets 0).
 * There is no inverted file: words[q][k], the number of word ids query q shares with live slot k (loopWords /
 * relocWords after the walk of :78-93 / :181-193), is found by looking every word of the slot up in the query.
 *
 * Query q, with S = the live slots with words > 0 (loop form: and not in the query's connected set):
 *   maxw = max words over S, minw = (int)(0.8f * (float)maxw); the slots of S with words > minw are scored:
 *   score[q][k] = (float)voc.score(query, slot).  Relocalisation also stores it in reloc_score[k].
 *   Every scored k (loop form: with score >= min_score[q]) opens a group: acc = best = score, bestk = k; its
 *   covis[k][0..9] in order, -1 and slots outside S skipped (loop form: and slots this query did not score),
 *   add their score to acc (float) and take bestk where it is > best.  Relocalisation adds reloc_score[nb], which
 *   for a slot of S this query did not score is what the latest earlier query that scored it left (:239-247).
 *   bestAcc = max over the groups' acc, starting from 0 (loop form: min_score[q]); the candidates are the set of
 *   bestk of the groups with acc > 0.75f * bestAcc, ascending slot ids (the reference's std::set<KeyFrame*>).
 * A batch of Q queries gives the result of the Q calls in order q = 0 .. Q-1: loop queries are independent,
 * relocalisation queries are coupled through reloc_score (a last-writer scan over q per slot).
 *
 * Outputs: cand[q*max_keyframes ..] ascending (the rest -1) and n_cand[q]; optional (NULL to skip), each
 * [Q][max_keyframes]: words, scored, score (0 where not scored), acc (0 where no group), bestk (-1 where none).
 * A database's calls share one workspace: enqueue them on one stream at a time.
 * ---------------------------------------------------------------------------------------- */
typedef struct orbdb_database orbdb_database;
#define ORBDB_COVIS 10   /* GetBestCovisibilityKeyFrames(10) */

typedef struct orbdb_query_batch {
    int32_t n_queries;
    int32_t cap;                 /* the query BowVectors in orbv_transform_batch_device's layout: frame f at f*cap */
    int32_t n_frames;            /* frames in the three arrays */
    const uint32_t* bow_word; const double* bow_weight; const int32_t* n_words;
    const int32_t* frame;        /* query q is frame frame[q] (NULL: q); outside [0, n_frames) = an empty query */
    const int32_t* covis;        /* [max_keyframes][ORBDB_COVIS] slots, -1 padded, GetBestCovisibilityKeyFrames(10) order */
    /* loop form only: */
    const int32_t* conn_off;     /* [n_queries + 1] CSR of GetConnectedKeyFrames() as slots (the query's own slot too, */
    const int32_t* conn_idx;     /* if it is live); entries outside [0, max_keyframes) are ignored */
    const float* min_score;      /* [n_queries], e.g. orbdb_min_score_device's output */
} orbdb_query_batch;

typedef struct orbdb_result {
    int32_t* cand; int32_t* n_cand;
    int32_t* words; uint8_t* scored; float* score; float* acc; int32_t* bestk;   /* optional */
} orbdb_result;

/* KeyFrameDatabase(const ORBVocabulary&) (:34-37).  ORB_EINVAL unless the vocabulary's scoring is L1_NORM (0),
 * 1 <= max_keyframes <= 1048576 and 1 <= word_cap <= ORBV_MAX_FEATURES.  All slots start erased. */
int orbdb_create(const orbv_vocabulary* voc, int max_keyframes, int word_cap, int device, orbdb_database** out);
int orbdb_destroy(orbdb_database* db);
int orbdb_info(const orbdb_database* db, int* max_keyframes, int* word_cap);
/* clear() (:62-66): every slot erased.  Enqueue only on `stream`. */
int orbdb_clear(orbdb_database* db, void* stream);
/* add(KeyFrame*) (:39-45) for n keyframes: slot d_slot[i] takes the BowVector of frame d_frame[i] (NULL: i) of an
 * orbv_transform_batch_device output (stride cap, n_frames frames), becomes live and gets reloc_score 0.  The
 * slots of one call are distinct.  An entry whose slot, frame or word count (> word_cap) is out of range is left
 * out (device memory cannot be validated here; orbdb_add refuses it).  Enqueue only on `stream`. */
int orbdb_add_device(orbdb_database* db, int n, const int32_t* d_slot, const int32_t* d_frame,
                     const uint32_t* d_bow_word, const double* d_bow_weight, const int32_t* d_n_words, int cap,
                     int n_frames, void* stream);
/* erase(KeyFrame*) (:47-60): a flag store per slot; out-of-range slots are ignored.  Enqueue only on `stream`. */
int orbdb_erase_device(orbdb_database* db, int n, const int32_t* d_slot, void* stream);
/* LoopDetector::Detect's minScore (LoopClosing.cc:170-178): d_min_score[q] = min(1.f, (float)score(query q, slot k))
 * over the slots k of d_cov_idx[d_cov_off[q] .. d_cov_off[q+1]) (GetVectorCovisibleKeyFrames(); the host leaves out
 * isBad() ones; erased or out-of-range slots are skipped).  b->covis and the loop fields are not read.  Enqueue
 * only on `stream`. */
int orbdb_min_score_device(orbdb_database* db, const orbdb_query_batch* b, const int32_t* d_cov_off,
                           const int32_t* d_cov_idx, float* d_min_score, void* stream);
/* DetectRelocalizationCandidates (:173-265) / DetectLoopCandidates (:68-171) as described above; every array in
 * HBM; enqueue only on `stream`, nothing is read back. */
int orbdb_detect_reloc_device(orbdb_database* db, const orbdb_query_batch* b, const orbdb_result* out, void* stream);
int orbdb_detect_loop_device(orbdb_database* db, const orbdb_query_batch* b, const orbdb_result* out, void* stream);
/* Host-memory forms, synchronous.  Slots, frames, word counts, the covisibility table and the CSR lists are
 * validated before anything is copied: ORB_EINVAL for a slot outside [0, max_keyframes) or named twice, a frame
 * outside [0, n_frames), n_words > word_cap (add) or > cap, Q < 0, a NULL required array. */
int orbdb_add(orbdb_database* db, int n, const int32_t* slot, const int32_t* frame, const uint32_t* bow_word,
              const double* bow_weight, const int32_t* n_words, int cap, int n_frames);
int orbdb_erase(orbdb_database* db, int n, const int32_t* slot);
int orbdb_min_score(orbdb_database* db, const orbdb_query_batch* b, const int32_t* cov_off, const int32_t* cov_idx,
                    float* min_score);
int orbdb_detect_reloc(orbdb_database* db, const orbdb_query_batch* b, const orbdb_result* out);
int orbdb_detect_loop(orbdb_database* db, const orbdb_query_batch* b, const orbdb_result* out);
/* The slots' state, synchronous: live[k] and reloc_score[k], max_keyframes entries each (either may be NULL). */
int orbdb_read_slots(orbdb_database* db, uint8_t* live, float* reloc_score);

/* ------------------------------------------------------------------------------------------
 * Tracking's local map: LocalMap::Update (src/Tracking.cc:59-179: UpdateLocalKeyFrames, UpdateLocalPoints) and
 * SearchLocalPoints up to the matcher call (:607-642, IsInFrustum :554-605), batched over frames.  The outputs are
 * the arrays of an orbm_proj_batch, so orbm_search_by_projection_device is enqueued behind this call on the same
 * stream with nothing copied back; orbba_pose_optimization_device follows it: TrackLocalMap (:651-683).
 *
 * The map is slot tables the caller owns.  Keyframe slot k in [0, n_keyframes), map-point slot m in
 * [0, n_mappoints); -1 is a null pointer.  Per frame f, in this order:
 *  1 votes (:72-88): every frame_mappoint[f][i], i < frame_n[f], that is >= 0 and not bad adds 1 to
 *    votes[f][k] for each k of its observation list; a bad one is set to -1 in frame_mappoint.
 *  2 first part (:90-116): with no vote at all the call leaves local_kf / n_local_kf as they came in and
 *    reference_kf[f] = -1 (unchanged).  Otherwise the list is cleared and every voted, non-bad k appended and
 *    marked; reference_kf[f] = the first with a strictly greater count (-1 when all voted ones are bad).
 *  3 second part (:119-156): for each element of the first part, in order: stop when the list holds more than 80;
 *    append the first non-bad unmarked entry of kf_covis[k]; the first non-bad unmarked child; the parent if it
 *    is unmarked (bad or not), and then stop the whole walk (the break of :152 leaves the outer loop).
 *  4 UpdateLocalPoints (:165-179): the map points of the listed keyframes in list order, then keypoint order
 *    (kf_mappoint[k][0 .. kf_n[k])), each at its first occurrence, null and bad ones left out: local_mp[f][..],
 *    n_local_mp[f].
 *  5 :610-625: every non-null frame_mappoint[f][i] gets mp_visible += 1 and is not projected (lastFrameSeen).
 *  6 :631-642: every other local point runs IsInFrustum with min_view_cos; a passing one gets mp_visible += 1;
 *    n_to_match[f] counts them.
 * Departure from the reference: it walks a std::map<KeyFrame*, int> (the votes) and a std::set<KeyFrame*> (the
 * children) in pointer order, which no two runs share.  Here both are walked in ascending slot order.
 *
 * Outputs for local point j of frame f, at f*mp_cap + j: mp_valid (in frustum = trackInView && !isBad()), mp_proj
 * (u, v, u - bf/z), mp_view_cos, mp_level (all 0 where mp_valid is 0), mp_desc and mp_has_obs (mp_nobs > 0) for
 * every j < n_local_mp[f]; slots from n_local_mp[f] on hold mp_valid 0, local_mp -1 and zeros.  mp_begin[f] =
 * f*mp_cap and kp_begin[f] = f*kp_cap (F + 1 entries each) make them an orbm_proj_batch over keypoint arrays of
 * stride kp_cap without a pass across frames.  kp_claimed[f*kp_cap + i] = frame_mappoint >= 0 && mp_nobs > 0
 * (after step 1), and 1 for the padding i >= frame_n[f], which the search therefore never matches (give the
 * padding any finite kp_xy).
 *
 * status[f]: ORBTL_OK, or ORBTL_KF_OVERFLOW (steps 2-3 built more than kf_list_cap keyframes; local_kf keeps the
 * first kf_list_cap, n_local_kf[f] = kf_list_cap), or ORBTL_MP_OVERFLOW (step 4 found more than mp_cap points).
 * Such a frame gets n_to_match[f] = -1, n_local_mp[f] = 0, no local point and no mp_visible increment; nothing is
 * written out of bounds and the other frames are unaffected.
 * Frames of a batch are independent except that their mp_visible increments add up (integer atomics: a batch
 * equals its frames run one at a time, in any order).  Two frames of one batch must not share a local_kf row.
 *
 * Workspace (per thread, grow-only, as the projection searches'): per (frame, map point) a uint32 first-occurrence
 * key (list position * kf_cap + index, by atomicMin) and a seen byte, per (frame, keyframe) a mark byte and, when
 * votes is NULL, the int32 votes: n_frames * (5 * n_mappoints + 5 * n_keyframes + 4 * kf_list_cap) bytes.
 * ---------------------------------------------------------------------------------------- */
#define ORBTL_OK 0
#define ORBTL_KF_OVERFLOW 1
#define ORBTL_MP_OVERFLOW 2
#define ORBTL_MAX_KEYFRAMES 80   /* the walk of step 3 stops once the list holds more (:122) */

typedef struct orbtl_map {
    int32_t n_keyframes, n_mappoints, kf_cap;
    const uint8_t* kf_bad;        /* [K] isBad() */
    const int32_t* kf_covis;      /* [K][ORBDB_COVIS] GetBestCovisibilityKeyFrames(10) order, -1 padded (orbdb_query_batch.covis) */
    const int32_t* kf_parent;     /* [K] GetParent(), -1 for none */
    const int32_t* kf_child_off;  /* [K + 1] CSR of GetChildren(), each list ascending */
    const int32_t* kf_child_idx;
    const int32_t* kf_n;          /* [K] N */
    const int32_t* kf_mappoint;   /* [K][kf_cap] GetMapPointMatches() */
    const uint8_t* mp_bad;        /* [M] */
    const float* mp_xw;           /* [M][3] GetWorldPos() */
    const float* mp_normal;       /* [M][3] GetNormal() */
    const float* mp_max_min;      /* [M][2] maxDistance_, minDistance_ (raw, as orbm_reloc_batch takes them) */
    const uint8_t* mp_desc;       /* [M][32] GetDescriptor() */
    const int32_t* mp_nobs;       /* [M] Observations() */
    const int32_t* mp_obs_off;    /* [M + 1] CSR of GetObservations() keys as keyframe slots */
    const int32_t* mp_obs_kf;
    int32_t* mp_visible;          /* [M] read and updated: IncreaseVisible() */
} orbtl_map;

typedef struct orbtl_frames {
    int32_t n_frames, kp_cap, kf_list_cap, mp_cap;
    int32_t n_levels;             /* frame.pyramid.nlevels, 1 .. 32 */
    float log_scale_factor;       /* frame.pyramid.logScaleFactor */
    float min_view_cos;           /* 0.5f at the call site (:637) */
    const int32_t* frame_n;       /* [F] N */
    int32_t* frame_mappoint;      /* [F][kp_cap] read and updated (step 1) */
    const float* pose;            /* [F][12] Rcw row-major, tcw */
    const float* camera;          /* [F][5] fx, fy, cx, cy, bf */
    const float* bounds;          /* [F][4] imageBounds minx, maxx, miny, maxy */
    int32_t* local_kf;            /* [F][kf_list_cap] read and updated: LocalMap::keyframes of frame f's tracker */
    int32_t* n_local_kf;          /* [F] */
} orbtl_frames;

typedef struct orbtl_result {
    int32_t* reference_kf;        /* [F] */
    int32_t* local_mp;            /* [F][mp_cap] */
    int32_t* n_local_mp;          /* [F] */
    int32_t* n_to_match;          /* [F] */
    int32_t* status;              /* [F] */
    int32_t* kp_begin;            /* [F + 1] f*kp_cap */
    int32_t* mp_begin;            /* [F + 1] f*mp_cap */
    uint8_t* kp_claimed;          /* [F][kp_cap] */
    uint8_t* mp_valid;            /* [F][mp_cap] */
    float* mp_proj;               /* [F][mp_cap][3] */
    float* mp_view_cos;           /* [F][mp_cap] */
    int32_t* mp_level;            /* [F][mp_cap] */
    uint8_t* mp_desc;             /* [F][mp_cap][32] */
    uint8_t* mp_has_obs;          /* [F][mp_cap] */
    int32_t* votes;               /* optional (NULL to skip): [F][K] */
} orbtl_result;

/* Every array in HBM; enqueue only on `stream`: no synchronisation, no copy.  Slots read from device memory are
 * not trusted: one outside its table is treated as null.  ORB_EINVAL for a NULL required array, negative sizes,
 * kf_cap / kp_cap / kf_list_cap / mp_cap < 1, n_levels outside [1, 32], kf_list_cap * kf_cap >= 2^31 or a table of
 * 2^31 entries or more. */
int orbtl_track_local_map_device(const orbtl_map* map, const orbtl_frames* frames, const orbtl_result* out,
                                 void* stream);
/* Host memory, synchronous.  Before anything is copied: the checks above, every slot of every table in range
 * (kf_covis, kf_parent, frame_mappoint, kf_mappoint in [-1, size); kf_child_idx, mp_obs_kf, local_kf in [0, size)),
 * kf_n in [0, kf_cap], frame_n in [0, kp_cap], n_local_kf in [0, kf_list_cap], both CSR offset arrays starting at 0
 * and not decreasing, log_scale_factor finite and > 0.  ORB_EINVAL otherwise. */
int orbtl_track_local_map(const orbtl_map* map, const orbtl_frames* frames, const orbtl_result* out, int device);

/* ------------------------------------------------------------------------------------------
 * Map maintenance: the tables the other batches read, kept up to date in HBM.
 *   orbmm_update_normal_depth   MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:341-380) batched over map points:
 *                               mp_normal and mp_max_min, the arrays orbtl_map and the Fuse / relocalisation / Sim3
 *                               batches take, from the poses orbba_gba_update_map_device leaves.
 *   orbmm_update_connections    KeyFrame::UpdateConnections with AddConnection / UpdateBestCovisibles
 *                               (src/KeyFrame.cc:94-119, 235-309) batched over keyframes: the connection rows, the
 *                               ordered rows, kf_parent, kf_first_connection and kf_covis.
 *   orbmm_children              the GetChildren() CSR as the inverse of kf_parent.
 *   orbmm_covis_csr             the rows packed into the CSR forms orbba_eg_tables and orbdb_query_batch take.
 * Slots follow orbtl_map: keyframe slot k in [0, n_keyframes), map-point slot in [0, n_mappoints), -1 is null.  A
 * slot, an offset or an index read from device memory is not trusted: one outside its table is skipped.
 *
 * UpdateNormalAndDepth, per point (csrc/mm_normal.h, float as the reference): a bad point, one with no observation
 * in the table and one whose reference slot (or the keypoint index / octave read for it) is outside its table are
 * left as they are.  Ow = (-R^T) t per keyframe, each sum ascending from 0; normal = (1. / n) * sum over the
 * observations, in CSR order, of Normalized(Xw - Ow) (cv::norm in double, 1. / norm in double, each component narrowed
 * after the product); dist = (float)cv::norm(Xw - Ow_ref); maxDistance = scaleFactors[octave] * dist and minDistance
 * = maxDistance / scaleFactors[n_levels - 1], the octave that of the reference keyframe's keypoint mp_obs_idx of its
 * observation (keypoint 0 when the reference keyframe does not observe the point: observations[referenceKF] inserts 0).
 * Departure: the observations are summed in the caller's CSR order; the reference walks a std::map<KeyFrame*, size_t>
 * in pointer order, which no two runs share.
 *
 * UpdateConnections, per batch item[0 .. n_items) of keyframe slots: the result is that of the reference's calls one
 * after another in batch order, slots standing in for pointers.  The counter of keyframe k: for every
 * kf_mappoint[k][i], i < kf_n[k], that is not null and not bad, +1 for every observer o with kf_id[o] != kf_id[k].
 * An empty counter changes nothing.  A count >= ORBMM_THRESHOLD gives a pair and AddConnection(k, count) on that
 * neighbour; with no such count the only pair is the largest count, the lowest slot among equals.  k's connection row
 * becomes the whole counter (ascending slots), its ordered row the pairs sorted descending by (weight, slot); with
 * kf_first_connection[k] set and kf_id[k] != 0 the parent becomes the ordered row's front and the flag clears.
 * AddConnection on X takes effect if X has no entry for k or another weight; X's ordered row is then rebuilt from its
 * whole connection row (UpdateBestCovisibles), entries below the threshold included.  kf_covis[X] = the first
 * ORBDB_COVIS of the ordered row, -1 padded, rewritten with it.  A rewritten row is padded with slot -1 / weight 0 up
 * to conn_cap.  An item outside [0, n_keyframes) is skipped.
 * status[k] (written for every keyframe): ORBMM_OK, or ORBMM_CONN_OVERFLOW when k's connection row would at any
 * point of the batch hold more than conn_cap entries: every array of k is then left as it came in; the other
 * keyframes are unaffected (a keyframe's final state depends only on the events that reach it).  Capacity is checked
 * before anything is written.  No floating point and no atomics on HBM: two runs are byte-identical.
 *
 * Workspace (per thread, grow-only): n_items * n_keyframes int32 counts, 20 bytes per item, 8 * n_keyframes *
 * conn_cap bytes of working rows; 12 bytes per keyframe for orbmm_update_normal_depth.  ORBMM_WINDOW (read per
 * call, default and at most 8192, at least 64) is the number of keyframe slots one pass of the LDS histogram covers.
 * ---------------------------------------------------------------------------------------- */
#define ORBMM_OK 0
#define ORBMM_CONN_OVERFLOW 1
#define ORBMM_THRESHOLD 15

typedef struct orbmm_points {
    int32_t n_keyframes, n_mappoints, kf_cap;
    int32_t n_obs;                 /* entries of mp_obs_kf / mp_obs_idx (>= mp_obs_off[n_mappoints]) */
    int32_t n_levels;              /* 1 .. 32 */
    const float*   scale_factors;  /* host memory, n_levels: pyramid.scaleFactors */
    const uint8_t* mp_bad;         /* [M] */
    const float*   mp_xw;          /* [M][3] */
    const int32_t* mp_ref_kf;      /* [M] GetReferenceKeyFrame() as a slot */
    const int32_t* mp_obs_off;     /* [M + 1] CSR of GetObservations(): orbtl_map's */
    const int32_t* mp_obs_kf;      /* keyframe slot of each observation */
    const int32_t* mp_obs_idx;     /* keypoint index of each observation */
    const float*   kf_pose;        /* [K][12] Rcw row-major, tcw (orbba_gba_map.kf_pose) */
    const int32_t* kf_n;           /* [K] */
    const int32_t* kf_kp_octave;   /* [K][kf_cap] keypointsUn[i].octave */
    int32_t        n_points;       /* entries of point; ignored when point is NULL */
    const int32_t* point;          /* optional: the point slots to update (NULL: every point) */
    float* mp_normal;              /* [M][3] updated in place */
    float* mp_max_min;             /* [M][2] maxDistance_, minDistance_; updated in place */
} orbmm_points;

typedef struct orbmm_graph {
    int32_t n_keyframes, n_mappoints, kf_cap;
    int32_t conn_cap;              /* row capacity of the four row arrays */
    int32_t n_obs;                 /* entries of mp_obs_kf */
    const int32_t* kf_id;          /* [K] KeyFrame::id */
    const int32_t* kf_n;           /* [K] */
    const int32_t* kf_mappoint;    /* [K][kf_cap] */
    const uint8_t* mp_bad;         /* [M] */
    const int32_t* mp_obs_off;     /* [M + 1] */
    const int32_t* mp_obs_kf;
    int32_t* conn_slot;            /* [K][conn_cap] connectionTo_, ascending slots */
    int32_t* conn_weight;          /* [K][conn_cap] */
    int32_t* n_conn;               /* [K] */
    int32_t* ord_slot;             /* [K][conn_cap] orderedConnectedKeyFrames_ */
    int32_t* ord_weight;           /* [K][conn_cap] orderedWeights_ */
    int32_t* n_ord;                /* [K] */
    uint8_t* kf_first_connection;  /* [K] firstConnection_ */
    int32_t* kf_parent;            /* [K] */
    int32_t* kf_covis;             /* [K][ORBDB_COVIS] */
    int32_t* status;               /* [K] ORBMM_*; output only (orbmm_covis_csr does not read it: may be NULL there) */
} orbmm_graph;

/* The packed forms.  covis_*: orbba_eg_tables' ordered rows of every keyframe (covis_begin K + 1 entries; covis_slot
 * and covis_weight must hold n_keyframes * conn_cap entries; a slot whose kf_bad is set, or outside the table, becomes
 * -1).  conn_*: orbdb_query_batch's connected sets (the connection row, ascending) of the keyframes query[0 ..
 * n_queries), conn_off n_queries + 1 entries, conn_idx n_queries * (conn_cap + 1); append_self adds the query's own
 * slot at the end of its list.  Either group may be left out (all of its pointers NULL). */
typedef struct orbmm_csr {
    const uint8_t* kf_bad;         /* [K]; NULL: none is bad */
    int32_t* covis_begin; int32_t* covis_slot; int32_t* covis_weight;
    int32_t n_queries; const int32_t* query; int32_t append_self;
    int32_t* conn_off; int32_t* conn_idx;
} orbmm_csr;

/* Device forms: every array in HBM but scale_factors; enqueue only on `stream`, nothing is copied back.  ORB_EINVAL
 * for a NULL required array, negative sizes, kf_cap or conn_cap < 1, n_levels outside [1, 32] and a table of 2^31
 * entries or more.  The workspace belongs to the calling thread: its calls must be stream-ordered. */
int orbmm_update_normal_depth_device(const orbmm_points* p, void* stream);
int orbmm_update_connections_device(const orbmm_graph* g, int32_t n_items, const int32_t* item, void* stream);
/* kf_child_off (n_keyframes + 1) and kf_child_idx (n_keyframes entries), each list ascending; a parent outside
 * [0, n_keyframes) is no parent.  One workgroup: count, scan, fill. */
int orbmm_children_device(int32_t n_keyframes, const int32_t* kf_parent, int32_t* kf_child_off, int32_t* kf_child_idx,
                          void* stream);
int orbmm_covis_csr_device(const orbmm_graph* g, const orbmm_csr* out, void* stream);
/* Host forms: every pointer is host memory, synchronous; the updated arrays are written back.  Before anything is
 * copied, besides the checks above: both CSR offset arrays start at 0 and do not decrease and end within n_obs, every
 * slot is in range (mp_obs_kf, item, point, query in [0, size); kf_mappoint, kf_parent, kf_covis, mp_ref_kf in
 * [-1, size); the first n_conn / n_ord entries of a row in [0, n_keyframes)), mp_obs_idx in [0, kf_cap), kf_n in
 * [0, kf_cap], the octaves of kf_n's keypoints in [0, n_levels), n_conn and n_ord in [0, conn_cap].  ORB_EINVAL
 * otherwise. */
int orbmm_update_normal_depth(const orbmm_points* p, int device);
int orbmm_update_connections(const orbmm_graph* g, int32_t n_items, const int32_t* item, int device);
int orbmm_children(int32_t n_keyframes, const int32_t* kf_parent, int32_t* kf_child_off, int32_t* kf_child_idx,
                   int device);
int orbmm_covis_csr(const orbmm_graph* g, const orbmm_csr* out, int device);

/* ------------------------------------------------------------------------------------------
 * The culls of LocalMapping (src/LocalMapping.cc:335-369, 641-701), in place on the tables above, with the
 * bookkeeping they rest on: MapPoint::SetBadFlag and EraseObservation (src/MapPoint.cc:124-182), KeyFrame::SetBadFlag
 * and EraseConnection (src/KeyFrame.cc:379-489).  Slots as above; a slot, an offset or an index read from device
 * memory is not trusted: one outside its table is skipped, and no store leaves a table.
 *
 * An erased observation stays in the CSR as mp_obs_kf = -1 (every device entry of this header skips it);
 * orbmm_compact_observations writes the CSR without those.
 *
 * MapPoint::SetBadFlag(p): mp_bad[p] = 1; for every observation (o, idx) of p in range kf_mappoint[o][idx] = -1,
 * whatever it held (EraseMapPointMatch(idx)); every observation of p is erased; mp_nobs[p] stays, as nobservations_
 * does.
 *
 * orbmm_cull_map_points, per entry of recent[0 .. n_recent) (recentAddedMapPoints_), in the reference's branch order,
 * minObservation = monocular ? 2 : 3: a bad point is dropped; (float)mp_found / (float)mp_visible < 0.25f (IEEE
 * division: x / 0 is no reason to drop) -> SetBadFlag and dropped; cur_kf_id - mp_first_kf_id >= 2 && mp_nobs <=
 * minObservation -> SetBadFlag and dropped; cur_kf_id - mp_first_kf_id >= 3 -> dropped; otherwise kept.  A slot
 * outside [0, n_mappoints) is dropped.  recent is rewritten in place, its order kept; *n_recent_out = what is left.
 * A grid kernel (the points are independent) and a one-workgroup stable compaction.
 *
 * orbmm_cull_keyframes: the targets are ord_slot[cur][0 .. n_ord[cur]) as they are at entry, in that order, one after
 * another (a culled target changes what later ones see).  Target t is skipped if kf_id[t] == 0 or kf_bad[t] (the
 * second is a departure; it cannot occur on consistent tables).  Over i1 < kf_n[t] with p = kf_mappoint[t][i1] not
 * null and not bad: unless monocular, i1 is skipped where kf_depth[t][i1] > th_depth || kf_depth[t][i1] < 0;
 * npoints++; if mp_nobs[p] > 3 and at least three observations (o, i2) of p have o != t and kf_kp_octave[o][i2] <=
 * kf_kp_octave[t][i1] + 1, nredundant++.  t is culled if nredundant > 0.9 * npoints (double).  Culling t with
 * kf_not_erase[t] set: kf_to_be_erased[t] = 1, nothing else.  Otherwise, in this order:
 *   1. EraseConnection: every v of t's connection row loses its entry for t, if it has one; v's ordered row is then
 *      rebuilt from its whole connection row, descending by (weight, slot), with kf_covis[v] (UpdateBestCovisibles).
 *   2. EraseObservation: for every kf_mappoint[t][i] not null, i < kf_n[t], whose point p observes t at idx:
 *      mp_nobs[p] -= kf_uright[t][idx] >= 0 ? 2 : 1; that observation is erased; if mp_ref_kf[p] == t it becomes the
 *      first remaining observation in CSR order, or -1 (departure: the reference takes the first in pointer order);
 *      if mp_nobs[p] <= 2, SetBadFlag(p).  kf_mappoint[t] itself is left, as mappoints_ is.
 *   3. t's rows are cleared: n_conn = n_ord = 0, slot -1 / weight 0 up to conn_cap, kf_covis[t] = -1.
 *   4. The spanning tree: the candidates start as {kf_parent[t]}; repeatedly, over the not-bad children of t in
 *      ascending slot order (departure: pointer order) and the entries of each child's ordered row in order, an entry
 *      whose kf_id equals a candidate's competes with its weight in the child's connection row (0 if absent); a
 *      strictly larger weight wins, so the first met among equals stays; the winning child gets that entry as parent,
 *      joins the candidates and leaves the children.  When no pair is found the remaining children get kf_parent[t].
 *      kf_parent[t] stays.  kf_tcp[t] = kf_pose[t] * Inverse(kf_pose[kf_parent[t]]) in float (CameraPose.h:44-56, one
 *      rounding per operation), left alone when the parent is outside the table.  kf_bad[t] = 1.
 * culled[0 .. conn_cap): the culled slots in order, -1 padded: orbdb_erase_device(db, conn_cap, culled, stream) is
 * keyFrameDB_->erase without a count crossing PCIe.  *n_culled: their number.  *status: ORBMM_OK.
 * One launch of one workgroup of four wavefronts: all lanes over the target's row for the count and for
 * EraseObservation, one wavefront per neighbour for EraseConnection, one for the tree, barriers between the phases.
 * No floating-point and no HBM atomics (each point and each row has one writer per phase): two runs are
 * byte-identical.  Tables where a point is twice in one keyframe's row (below kf_n) or a keyframe twice in one
 * point's observations: the host entries refuse them; on the device entries the result is unspecified, but every
 * store stays inside its table.
 *
 * Workspace (per thread, grow-only): n_recent bytes; 4 * (9 * conn_cap + 2 * n_keyframes + 1) bytes.
 * ---------------------------------------------------------------------------------------- */
typedef struct orbmm_cull {
    int32_t n_keyframes, n_mappoints, kf_cap;
    int32_t conn_cap;                 /* row capacity of the four row arrays; orbmm_cull_map_points ignores it */
    int32_t n_obs;                    /* entries of mp_obs_kf / mp_obs_idx (>= mp_obs_off[n_mappoints]) */
    /* orbmm_cull_map_points reads only the arrays marked P; the others may be NULL there */
    const int32_t* kf_id;             /* [K] */
    const int32_t* kf_n;              /* [K] */
    int32_t*       kf_mappoint;       /* [K][kf_cap] P, updated */
    const int32_t* kf_kp_octave;      /* [K][kf_cap] */
    const float*   kf_uright;         /* [K][kf_cap] */
    const float*   kf_depth;          /* [K][kf_cap] */
    const float*   kf_pose;           /* [K][12] Rcw row-major, tcw */
    uint8_t*       kf_bad;            /* [K] updated */
    const uint8_t* kf_not_erase;      /* [K] notErase_ */
    uint8_t*       kf_to_be_erased;   /* [K] toBeErased_, updated */
    float*         kf_tcp;            /* [K][12] Tcp, written for the culled */
    uint8_t*       mp_bad;            /* [M] P, updated */
    int32_t*       mp_nobs;           /* [M] P nobservations_ (a stereo observation counts 2), updated by the keyframe cull */
    const int32_t* mp_found;          /* [M] P */
    const int32_t* mp_visible;        /* [M] P */
    const int32_t* mp_first_kf_id;    /* [M] P firstKFid */
    int32_t*       mp_ref_kf;         /* [M] updated */
    const int32_t* mp_obs_off;        /* [M + 1] P */
    int32_t*       mp_obs_kf;         /* P, updated: -1 where erased */
    const int32_t* mp_obs_idx;        /* P */
    int32_t* conn_slot; int32_t* conn_weight; int32_t* n_conn;   /* orbmm_graph's, updated */
    int32_t* ord_slot; int32_t* ord_weight; int32_t* n_ord;
    int32_t* kf_parent;               /* [K] updated */
    int32_t* kf_covis;                /* [K][ORBDB_COVIS] updated */
} orbmm_cull;

/* Device forms: every array in HBM; enqueue only on `stream`, nothing is copied back.  ORB_EINVAL for a NULL required
 * array, negative sizes, kf_cap or conn_cap < 1 and a table of 2^31 entries or more.  The workspace belongs to the
 * calling thread: its calls must be stream-ordered. */
int orbmm_cull_map_points_device(const orbmm_cull* c, int32_t n_recent, int32_t* recent, int32_t cur_kf_id,
                                 int32_t monocular, int32_t* n_recent_out, void* stream);
int orbmm_cull_keyframes_device(const orbmm_cull* c, int32_t cur, int32_t monocular, float th_depth, int32_t* culled,
                                int32_t* n_culled, int32_t* status, void* stream);
/* The CSR without the entries whose mp_obs_kf is -1, the order within a point kept, into out_off (n_mappoints + 1) and
 * out_kf / out_idx (n_obs entries each, distinct from the inputs; the caller swaps the arrays).  Count per point, one
 * scan by one workgroup, fill. */
int orbmm_compact_observations_device(int32_t n_mappoints, int32_t n_obs, const int32_t* mp_obs_off,
                                      const int32_t* mp_obs_kf, const int32_t* mp_obs_idx, int32_t* out_off,
                                      int32_t* out_kf, int32_t* out_idx, void* stream);
/* orbmm_children with the keyframes whose kf_bad is set left out as children: GetChildren() after EraseChild.
 * (orbmm_children lists a culled keyframe under its parent, because kf_parent of a culled keyframe stays.) */
int orbmm_children_live_device(int32_t n_keyframes, const int32_t* kf_parent, const uint8_t* kf_bad,
                               int32_t* kf_child_off, int32_t* kf_child_idx, void* stream);
/* Host forms: every pointer is host memory, synchronous; the updated arrays are written back.  Before anything is
 * copied, besides the checks above: the offsets start at 0, do not decrease and end within n_obs; mp_obs_kf in
 * [0, n_keyframes) (an erased entry is refused: compact first), mp_obs_idx in [0, kf_cap), kf_mappoint in
 * [-1, n_mappoints), recent in [0, n_mappoints), no keyframe twice in a point's observations; for the keyframe cull
 * also cur in [0, n_keyframes), kf_n in [0, kf_cap], mp_ref_kf and kf_parent in [-1, n_keyframes), n_conn and n_ord in
 * [0, conn_cap], the first n_conn / n_ord entries of a row in [0, n_keyframes), no point twice in a keyframe's row.
 * ORB_EINVAL otherwise. */
int orbmm_cull_map_points(const orbmm_cull* c, int32_t n_recent, int32_t* recent, int32_t cur_kf_id, int32_t monocular,
                          int32_t* n_recent_out, int device);
int orbmm_cull_keyframes(const orbmm_cull* c, int32_t cur, int32_t monocular, float th_depth, int32_t* culled,
                         int32_t* n_culled, int32_t* status, int device);
int orbmm_compact_observations(int32_t n_mappoints, int32_t n_obs, const int32_t* mp_obs_off, const int32_t* mp_obs_kf,
                               const int32_t* mp_obs_idx, int32_t* out_off, int32_t* out_kf, int32_t* out_idx, int device);
int orbmm_children_live(int32_t n_keyframes, const int32_t* kf_parent, const uint8_t* kf_bad, int32_t* kf_child_off,
                        int32_t* kf_child_idx, int device);

/* ------------------------------------------------------------------------------------------
 * Observation edits: the insert half of the observation graph, in place on the tables above.  MapPoint::AddObservation
 * and MapPoint::Replace (src/MapPoint.cc:109-122, 191-230) and the three loops that use them: ProcessNewKeyFrame's
 * (src/LocalMapping.cc:309-326), Fuse's apply loops (src/ORBmatcher.cc:957-976; :1070-1084 with
 * src/LoopClosing.cc:652-657) and CorrectLoop's matched points (src/LoopClosing.cc:617-634).  Slots as above; a slot, an
 * offset or an index read from device memory is not trusted: one outside its table is skipped, and no store leaves a
 * table.
 *
 * Row slack.  A point's row is [mp_obs_off[p], mp_obs_off[p + 1]); an entry whose mp_obs_kf is outside [0, K) is free
 * (-1 is what the culls leave).  mp_obs_off is never rewritten by an edit; orbmm_grow_observations makes room.
 *
 * AddObservation(p, k, idx): nothing if k is a live entry of p's row.  Otherwise the new entry goes before the first
 * live entry whose keyframe slot is greater than k (last if there is none), the row's live entries are packed to its
 * front in that order, the rest of the row is -1 in mp_obs_kf and mp_obs_idx, and mp_nobs[p] += kf_uright[k][idx] >= 0
 * ? 2 : 1.  Departure: the rows are kept ascending in keyframe slot, which stands in for the pointer order of
 * std::map<KeyFrame*, size_t>, as slot order does for the children and the votes elsewhere.  A row without a free
 * entry: nothing is written and the step reports ORBMM_OBS_OVERFLOW.
 *
 * Replace(loser -> survivor): nothing if they are one slot (the id test).  The survivor's bad flag is not tested.  Per
 * live entry (o, idx) of the loser: if the survivor does not observe o, kf_mappoint[o][idx] = survivor and
 * AddObservation(survivor, o, idx); otherwise kf_mappoint[o][idx] = -1.  Then mp_found and mp_visible of the loser are
 * added to the survivor's, the loser's row is all -1 (mp_obs_idx stays), mp_bad[loser] = 1, mp_replaced[loser] =
 * survivor; mp_nobs[loser] stays.  A survivor that gains nothing keeps its row as it is.  On ascending rows the new
 * row is the sorted union of the two, and it is built that way: every entry is placed at its rank.  If the union
 * does not fit the survivor's row, nothing of this Replace is written: ORBMM_OBS_OVERFLOW.
 * Departure: the reference recomputes the survivor's descriptor inside each Replace; here the caller recomputes once,
 * after the walk, on the final observations (the `touched` list).  The two differ only where a survivor gains a
 * further observation later in the same walk.
 *
 * The live entries of every row must ascend in keyframe slot on entry.  The host entries refuse a row that does not,
 * a keyframe twice in a row and a point twice in a keyframe's row (below kf_n); on the device entries the result is
 * then unspecified, but every store stays inside its table.
 *
 * orbmm_add_keyframe_observations(cur): for i < kf_n[cur] with p = kf_mappoint[cur][i] not null and not bad: if p does
 * not observe cur, AddObservation(p, cur, i) and p joins `added`; otherwise p joins `recent_out` (the stereo points
 * Tracking inserted: append them to recentAddedMapPoints_).  Both lists ascend in i, hold kf_cap entries, -1 padded;
 * counts[0] / counts[1] are their lengths.  status[i] (kf_cap entries): ORBMM_OK, or ORBMM_OBS_OVERFLOW when p's row
 * was full: that point is in neither list, the others still apply.  A grid kernel (the points of a row are distinct)
 * and a one-workgroup stable compaction.  `added` is what UpdateNormalAndDepth and the distinctive descriptors follow
 * over.
 *
 * orbmm_fuse_apply walks an orbm_fuse_batch-shaped list: item i is keyframe item_kf[i] with the entries
 * [mp_begin[i], mp_begin[i + 1]); point[m] is a map point slot or -1, best_idx[m] what orbm_fuse_device left.  The
 * items in order, the entries of an item in order:
 *   ORBMM_APPLY_FUSE: skipped if best_idx < 0, mp_bad[point] or the point observes the keyframe (the test of
 *     ORBmatcher.cc:876 evaluated again at the entry's turn).  in_kf = kf_mappoint[kf][best_idx].  If there is one and
 *     it is not bad: Replace(point -> in_kf) when mp_nobs[in_kf] > mp_nobs[point], else Replace(in_kf -> point).  If
 *     there is none: AddObservation(point, kf, best_idx) and kf_mappoint[kf][best_idx] = point.
 *   ORBMM_APPLY_FUSE_SIM3: phase 0 skips on best_idx < 0 or mp_bad[point] only; replace_point[m] = in_kf when in_kf is
 *     there and not bad, AddObservation / AddMapPoint when there is none.  Phase 1, after the item's whole list: for
 *     every replace_point[m] >= 0 in order, Replace(replace_point[m] -> point[m]).  replace_point: -1 on entry.
 *   ORBMM_APPLY_LOOP_MATCHED: best_idx[m] is the keypoint index, point[m] the matched loop point (-1: none).
 *     Replace(kf_mappoint[kf][best_idx] -> point) when the keyframe holds a point there, bad or not; otherwise
 *     kf_mappoint[kf][best_idx] = point and AddObservation(point, kf, best_idx).
 * n_fused[i]: the reference's nFused of item i (the entries past the skips; the matched entries in the third mode).
 * touched[0 .. *n_touched): ascending, the points the reference calls ComputeDistinctiveDescriptors on during the walk
 * that are not bad at its end: every Replace survivor, and the added points of the third mode.  The rest of touched, up
 * to n_mappoints entries, is -1: orbmm_update_normal_depth_device with point = touched and n_points = n_mappoints skips
 * the padding, so the count need not cross PCIe.  progress[4] = {item,
 * phase, entry within the item, the point whose row was full}: input and output, zero on the first call.  A walk that
 * ends: *status = ORBMM_OK, progress = {n_items, 0, 0, -1}.  A step that does not fit: the walk stops before it, the
 * tables hold exactly the steps before it, *status = ORBMM_OBS_OVERFLOW and progress names the step.  Grow the rows
 * and call again with the same progress, replace_point, n_fused, touched and n_touched: the result equals an
 * uninterrupted walk on rows that were large enough.
 * One launch of one workgroup of four wavefronts: the lanes scan the list in chunks and compact the hits into LDS in
 * order; the hits are taken one after another, every state-dependent test on uniformly loaded values; IsInKeyFrame,
 * the union and the kf_mappoint stores are spread over all lanes, barriers between the phases; a last scan turns the
 * touched flags into the list.  No HBM atomics and no floating-point arithmetic: two runs are byte-identical.
 *
 * orbmm_grow_observations: the CSR with every row its live entries (not -1) in order followed by `slack` free entries
 * (extra[p] instead where extra is given; a negative extra counts as 0), into out_off (n_mappoints + 1) and out_kf /
 * out_idx (n_obs_out entries each, distinct from the inputs).  *status = ORBMM_OBS_OVERFLOW when the total exceeds
 * n_obs_out: nothing is written at or past n_obs_out, and offsets past it read n_obs_out + 1.  With slack 0 this is
 * orbmm_compact_observations.  Count per point, one scan by one workgroup (64-bit sums), fill.
 *
 * Workspace (per thread, grow-only): kf_cap bytes; 4 * (3 * n_obs + n_mappoints) bytes for the walk.
 * ---------------------------------------------------------------------------------------- */
#define ORBMM_OBS_OVERFLOW 2
#define ORBMM_APPLY_FUSE 0
#define ORBMM_APPLY_FUSE_SIM3 1
#define ORBMM_APPLY_LOOP_MATCHED 2

typedef struct orbmm_observe {
    int32_t n_keyframes, n_mappoints, kf_cap;
    int32_t n_obs;                    /* entries of mp_obs_kf / mp_obs_idx (>= mp_obs_off[n_mappoints]) */
    /* orbmm_add_keyframe_observations does not read the arrays marked R; they may be NULL there */
    const int32_t* kf_n;              /* [K] */
    int32_t*       kf_mappoint;       /* [K][kf_cap] updated */
    const float*   kf_uright;         /* [K][kf_cap] */
    uint8_t*       mp_bad;            /* [M] updated */
    int32_t*       mp_nobs;           /* [M] updated */
    int32_t*       mp_found;          /* [M] R, updated */
    int32_t*       mp_visible;        /* [M] R, updated */
    int32_t*       mp_replaced;       /* [M] R replaced_ as a slot, -1 for none; updated */
    const int32_t* mp_obs_off;        /* [M + 1] */
    int32_t*       mp_obs_kf;         /* updated */
    int32_t*       mp_obs_idx;        /* updated */
} orbmm_observe;

typedef struct orbmm_apply {
    int32_t mode;                     /* ORBMM_APPLY_* */
    int32_t n_items, n_entries;       /* n_entries: entries of point / best_idx / replace_point (>= mp_begin[n_items]) */
    const int32_t* item_kf;           /* [n_items] keyframe slots */
    const int32_t* mp_begin;          /* [n_items + 1] */
    const int32_t* point;             /* [n_entries] */
    const int32_t* best_idx;          /* [n_entries] */
    int32_t* replace_point;           /* [n_entries] ORBMM_APPLY_FUSE_SIM3 only: -1 on the first call, updated */
    int32_t* n_fused;                 /* [n_items] written from the item the walk starts at */
    int32_t* touched;                 /* [M] */
    int32_t* n_touched;               /* [1] read when progress is not zero */
    int32_t* progress;                /* [4] input and output */
    int32_t* status;                  /* [1] ORBMM_OK or ORBMM_OBS_OVERFLOW */
} orbmm_apply;

/* Device forms: every array in HBM (the structs themselves are host memory); enqueue only on `stream`, nothing is copied
 * back.  ORB_EINVAL for a NULL required array, negative sizes, kf_cap < 1, an unknown mode and a table of 2^31 entries or
 * more.  The workspace belongs to the calling thread: its calls must be stream-ordered. */
int orbmm_add_keyframe_observations_device(const orbmm_observe* t, int32_t cur, int32_t* added, int32_t* recent_out,
                                           int32_t* counts, int32_t* status, void* stream);
int orbmm_fuse_apply_device(const orbmm_observe* t, const orbmm_apply* a, void* stream);
int orbmm_grow_observations_device(int32_t n_mappoints, int32_t n_obs, const int32_t* mp_obs_off, const int32_t* mp_obs_kf,
                                   const int32_t* mp_obs_idx, int32_t slack, const int32_t* extra, int32_t n_obs_out,
                                   int32_t* out_off, int32_t* out_kf, int32_t* out_idx, int32_t* status, void* stream);
/* Host forms: every pointer is host memory, synchronous; the updated arrays are written back.  Before anything is
 * copied, besides the checks above: the offsets start at 0, do not decrease and end within n_obs; mp_obs_kf in
 * [-1, n_keyframes) (-1 is the slack) and mp_obs_idx of a live entry in [0, kf_cap); the live entries of a row strictly
 * ascending (a keyframe twice in a row included); kf_n in [0, kf_cap], kf_mappoint in [-1, n_mappoints), no point twice
 * in a keyframe's row, mp_replaced in [-1, n_mappoints); cur and item_kf in [0, n_keyframes), mp_begin a CSR within
 * n_entries, point and replace_point in [-1, n_mappoints), best_idx in [-1, kf_cap), progress inside the list, the
 * touched list of a resumed walk in [0, n_mappoints), extra not negative.  ORB_EINVAL otherwise. */
int orbmm_add_keyframe_observations(const orbmm_observe* t, int32_t cur, int32_t* added, int32_t* recent_out,
                                    int32_t* counts, int32_t* status, int device);
int orbmm_fuse_apply(const orbmm_observe* t, const orbmm_apply* a, int device);
int orbmm_grow_observations(int32_t n_mappoints, int32_t n_obs, const int32_t* mp_obs_off, const int32_t* mp_obs_kf,
                            const int32_t* mp_obs_idx, int32_t slack, const int32_t* extra, int32_t n_obs_out,
                            int32_t* out_off, int32_t* out_kf, int32_t* out_idx, int32_t* status, int device);

/* ------------------------------------------------------------------------------------------
 * LoopCorrector::Correct (src/LoopClosing.cc:546-676), in place on the tables of orbmm_points / orbmm_graph: the
 * connected list, the propagation of Scw to the current keyframe's neighbours with the correction of their map
 * points and poses, and the LoopConnections sets; with orbba_essential_graph_edges_device the whole of CorrectLoop is
 * stream-ordered: orbmm_update_connections_device(cur), orblc_connected_device, orblc_propagate_device,
 * orbmm_update_connections_device(items), orbmm_fuse_apply_device (matched points), orbm_fuse_device /
 * orbmm_fuse_apply_device per neighbour, orblc_loop_connections_device, orbmm_covis_csr_device,
 * orbba_essential_graph_edges_device, orbba_optimize_essential_graph_device, orbmm_update_normal_depth_device.
 * orblc_map carries the pointers of both structs and two tables of its own: mp_corrected_by (MapPoint::correctedByKF,
 * a KeyFrame::id, initially 0) and mp_corrected_ref (correctedReference, as a slot).
 * Departure: where the reference iterates a std::map<KeyFrame*, ...> (CorrectedSim3, LoopConnections) in pointer
 * order, which no two runs share, the order here is ascending slot.
 *
 * orblc_connected (:550-552): connected[conn_cap + 1] = the ordered row of cur (ord_slot[cur][0 .. n_ord[cur])), a slot
 * outside [0, n_keyframes) dropped, then cur itself, then -1; n_connected[0] = the count.  Every later entry takes
 * `connected` in HBM and a host max_connected <= conn_cap + 1 (the entries it reads; -1 and a slot outside the table
 * are skipped): n_connected read back, or conn_cap + 1, with identical results.
 *
 * orblc_propagate (:554-613 without UpdateConnections; csrc/lc_propagate.h): scw[13] = R row-major, t, s.
 *   vertex_sim3 / edge_sim3 [K][13], the tables orbba_essential_graph takes: for a connected keyframe i the rows are
 *   CorrectedSiw = Sim3(Tiw * Twc) * Scw (Scw for cur; Twc = kf_pose[cur].Inverse()) and NonCorrectedSiw = Sim3(Tiw);
 *   for every other keyframe both are Sim3(kf_pose[k]), scale 1.  All rows from the poses as they are on entry, in
 *   the reference's float CameraPose / Sim3 classes.
 *   Claims: connected keyframes in ascending slot order, kf_mappoint[k][i] for i < kf_n[k] ascending; a point that is
 *   null, outside its table, bad or has mp_corrected_by == kf_id[cur] is skipped, so each point is corrected once, by
 *   the lowest connected slot that lists it, and a point that carries kf_id[cur] on entry by nobody.
 *   A claimed point: mp_xw = (CorrectedSwi * Siw).Map(P) in float, mp_corrected_by = kf_id[cur], mp_corrected_ref = k,
 *   then UpdateNormalAndDepth (orbmm_update_normal_depth's order and arithmetic) as the reference runs it inside the
 *   walk: observer o, and the reference keyframe, contributes the camera centre of its corrected pose if it is
 *   connected and o < k, of its entry pose otherwise.
 *   kf_pose[k] of a connected keyframe becomes (R, (1. / s) * t) of CorrectedSiw, 1. / s and the product in double.
 *   point_ref[M], the array orbba_essential_graph takes: -1 for a bad point, mp_corrected_ref where mp_corrected_by ==
 *   kf_id[cur], else mp_ref_kf.
 *   items (may be NULL) [max_connected]: the connected slots ascending, then -1: the batch the caller hands to
 *   orbmm_update_connections_device behind this call (:612).
 *   The claim is an integer atomicMin on a workspace array; no floating-point atomics: two runs are byte-identical.
 *
 * orblc_loop_connections (:661-676): for each connected[j] in list order, prev = its ordered row as it stands then,
 * UpdateConnections on it, the set = its whole connection row minus prev minus every connected keyframe.  Output in
 * the form orbba_eg_tables takes, rows in ascending slot order of conn_kf: conn_kf[max_connected] (an empty set keeps
 * its row; the rows of skipped items come last with conn_kf = -1), conn_begin[max_connected + 1],
 * conn_slot[max_connected * conn_cap] each list ascending (a stable compaction of the connection row, which is
 * ascending), n_connections[0] = the rows that are not skipped.
 * status[k] (written for every keyframe) is ORBMM_CONN_OVERFLOW if any of the updates reported it for k; such a
 * keyframe keeps its rows, and its set comes from the unchanged row.  Three enqueues per item: a call made once
 * per loop.
 *
 * Workspace per thread, grow-only: 76 bytes per keyframe and 4 per map point (propagate); 4 * (max_connected + 1) *
 * (conn_cap + 3) + 4 * n_keyframes bytes (loop connections) besides orbmm_update_connections_device's own.
 * ---------------------------------------------------------------------------------------- */
typedef struct orblc_map {
    int32_t n_keyframes, n_mappoints, kf_cap;
    int32_t conn_cap;
    int32_t n_obs;
    int32_t n_levels;              /* 1 .. 32 */
    const float*   scale_factors;  /* host memory, n_levels */
    /* orbmm_graph's */
    const int32_t* kf_id;          /* [K] */
    const int32_t* kf_n;           /* [K] */
    const int32_t* kf_mappoint;    /* [K][kf_cap] */
    const uint8_t* mp_bad;         /* [M] */
    const int32_t* mp_obs_off;     /* [M + 1] */
    const int32_t* mp_obs_kf;
    int32_t* conn_slot; int32_t* conn_weight; int32_t* n_conn;
    int32_t* ord_slot;  int32_t* ord_weight;  int32_t* n_ord;
    uint8_t* kf_first_connection;
    int32_t* kf_parent;
    int32_t* kf_covis;
    int32_t* status;               /* [K] output of orblc_loop_connections */
    /* orbmm_points' */
    const int32_t* mp_obs_idx;
    const int32_t* mp_ref_kf;      /* [M] */
    const int32_t* kf_kp_octave;   /* [K][kf_cap] */
    float* mp_xw;                  /* [M][3] updated in place */
    float* kf_pose;                /* [K][12] updated in place */
    float* mp_normal;              /* [M][3] updated in place */
    float* mp_max_min;             /* [M][2] updated in place */
    /* its own */
    int32_t* mp_corrected_by;      /* [M] KeyFrame::id, initially 0 */
    int32_t* mp_corrected_ref;     /* [M] slot */
} orblc_map;

/* The orbmm_graph that shares an orblc_map's arrays: what orbmm_update_connections[_device] takes for the same map. */
static inline orbmm_graph orblc_graph(const orblc_map* m) {
    orbmm_graph g;
    g.n_keyframes = m->n_keyframes; g.n_mappoints = m->n_mappoints; g.kf_cap = m->kf_cap; g.conn_cap = m->conn_cap;
    g.n_obs = m->n_obs; g.kf_id = m->kf_id; g.kf_n = m->kf_n; g.kf_mappoint = m->kf_mappoint; g.mp_bad = m->mp_bad;
    g.mp_obs_off = m->mp_obs_off; g.mp_obs_kf = m->mp_obs_kf; g.conn_slot = m->conn_slot; g.conn_weight = m->conn_weight;
    g.n_conn = m->n_conn; g.ord_slot = m->ord_slot; g.ord_weight = m->ord_weight; g.n_ord = m->n_ord;
    g.kf_first_connection = m->kf_first_connection; g.kf_parent = m->kf_parent; g.kf_covis = m->kf_covis; g.status = m->status;
    return g;
}

/* Device forms: every array in HBM but scale_factors; enqueue only on `stream`, nothing is copied back.  ORB_EINVAL
 * for a NULL array the entry uses, negative sizes, kf_cap or conn_cap < 1, n_levels outside [1, 32], a table of 2^31
 * entries or more, cur outside [0, n_keyframes), max_connected outside [0, conn_cap + 1].  orblc_connected reads the
 * rows only; orblc_loop_connections what orbmm_update_connections reads and writes.  The workspace belongs to the
 * calling thread: its calls must be stream-ordered. */
int orblc_connected_device(const orblc_map* m, int32_t cur, int32_t* connected, int32_t* n_connected, void* stream);
int orblc_propagate_device(const orblc_map* m, int32_t cur, const float* scw, const int32_t* connected,
                           int32_t max_connected, float* vertex_sim3, float* edge_sim3, int32_t* point_ref,
                           int32_t* items, void* stream);
int orblc_loop_connections_device(const orblc_map* m, const int32_t* connected, int32_t max_connected, int32_t* conn_kf,
                                  int32_t* conn_begin, int32_t* conn_slot, int32_t* n_connections, void* stream);
/* Host forms: every pointer is host memory, synchronous; the updated arrays are written back.  Before anything is
 * copied, besides the checks above, those of orbmm_update_connections / orbmm_update_normal_depth on the tables the
 * entry uses, `connected` entries in [-1, n_keyframes), and for orblc_propagate a scale <= 0 and a non-finite scw. */
int orblc_connected(const orblc_map* m, int32_t cur, int32_t* connected, int32_t* n_connected, int device);
int orblc_propagate(const orblc_map* m, int32_t cur, const float* scw, const int32_t* connected, int32_t max_connected,
                    float* vertex_sim3, float* edge_sim3, int32_t* point_ref, int32_t* items, int device);
int orblc_loop_connections(const orblc_map* m, const int32_t* connected, int32_t max_connected, int32_t* conn_kf,
                           int32_t* conn_begin, int32_t* conn_slot, int32_t* n_connections, int device);

/* orbba_essential_graph_edges on the device: every array of g, edge_i, edge_j, edge_table and n_edges in HBM; the
 * counts are host integers: n_loop_slots, n_covis_slots and n_conn_slots are the entries of loop_slot, covis_slot /
 * covis_weight and conn_slot (an offset read from the device is clamped to them).  g->n_connections may be the row
 * capacity: a row with conn_kf = -1 is skipped.  The loop connections are listed by one workgroup (a scan per row);
 * then per keyframe count, scan, fill, the insertedEdges test a search of the kept loop-connection pairs in either
 * direction.  edge_i / edge_j / edge_table are written up to `capacity`, the entries from the count up to capacity
 * as (-1, -1, 0), which orbba_optimize_essential_graph_device leaves out of the graph (so it can be called with
 * n_edges = capacity and nothing read back); n_edges[0] = the full count.  An index read from device memory outside
 * its table is skipped.  ORB_EINVAL for null pointers, n_keyframes < 1, negative sizes, curr_slot / loop_kf_slot out
 * of range. */
int orbba_essential_graph_edges_device(const orbba_eg_tables* g, int32_t n_loop_slots, int32_t n_covis_slots,
                                       int32_t n_conn_slots, int32_t min_weight, int32_t capacity, int32_t* edge_i,
                                       int32_t* edge_j, uint8_t* edge_table, int32_t* n_edges, void* stream);

/* ------------------------------------------------------------------------------------------
 * Tracking's per-frame state (src/Tracking.cc): frame.mappoints, frame.outlier and the pose kept in HBM between the
 * searches, orbtl_track_local_map_device and orbba_pose_optimization_device, batched over frames.  Seven small
 * entries; none searches or optimises.  Per-element arithmetic: csrc/tf_frame.h.
 *
 * Frame tables, stride kp_cap per frame (the layout of orbtl_frames and the projection batches); an entry reads only
 * the arrays its description names, the others may be NULL.  Map tables are those of orbtl_map / orbmm_observe.
 * A slot read from device memory is not trusted: a map point outside [0, n_mappoints), a match outside its row, a
 * keyframe outside [0, n_keyframes) counts as null; frame_n is clamped to [0, kp_cap]; orbtf_pose_edges, the
 * one entry that indexes a table by an octave, clamps it into the table (orbtf_motion_project passes kp_octave through as
 * mp_octave unchanged: the search behind it rejects an octave outside its own table).  Rows from frame_n[f] up are
 * padding and are left as they are unless said otherwise.
 * Frames of a batch are independent except that their mp_found increments add up (integer atomics): a batch equals
 * its frames run one at a time.  No floating-point atomics: two runs are byte-identical.
 *
 * 1 orbtf_apply_matches: frame_mappoint[f][i] = src[row][kp_match[f][i]] for i < frame_n[f], where src is a table of
 *   n_rows rows of src_cap slots and row = src_row[f] (NULL: row f): orbtl_result.local_mp (rows = frames), the last
 *   frames' frame_mappoint, or kf_mappoint through the reference keyframe's slot.  ORBTF_MERGE writes only where
 *   kp_match >= 0 (src/ORBmatcher.cc:376, the local-map search); ORBTF_REPLACE writes -1 where there is no match
 *   (the std::fill + search of src/Tracking.cc:232-239, currFrame.mappoints = mappoints of :273).  The value written
 *   is the source slot, -1 when that is outside [0, n_mappoints).
 * 2 orbtf_pose_edges: the gather of src/Optimizer.cc:355-411.  Per frame the keypoints i < frame_n[f] with a map
 *   point, in keypoint order, become the edges [edge_begin[f], edge_begin[f + 1]) of an orbba_pose_batch:
 *   frame_outlier[f][i] = 0 for exactly those, xw = mp_xw widened, obs = (kp_xy, kp_uright), inv_sigma2 =
 *   inv_sigma2_table[kp_octave] (float, n_levels entries, pyramid.invSigmaSq), edge_kp = i; pose_R / pose_t / cam are
 *   pose / camera widened.  The edge arrays hold n_frames * kp_cap rows.  Mono / stereo typing stays with the
 *   optimiser (ur < 0).  Two launches: count, then offsets and a stable compaction.
 * 3 orbtf_finish_pose: frame_outlier[f][edge_kp[e]] = outlier[e] and pose = the double pose narrowed with one
 *   rounding per element (FromSE3Quat, src/Optimizer.cc:157-162) for a frame with 3 edges or more (:413-415: a
 *   frame with fewer keeps its pose and its zero flags).  Then over the keypoints with a map point, in order:
 *   ORBTF_DISCARD (DiscardOutliers, src/Tracking.cc:187-211): an outlier's map point becomes -1 and its flag 0, and
 *     its slot is appended to discarded[f][..] (n_discarded[f]; keypoint order; the points whose lastFrameSeen the
 *     reference sets); n_inliers[f] counts the others that have mp_nobs > 0.
 *   ORBTF_LOCAL_MAP (:664-680): a non-outlier gets mp_found += 1 and counts into n_inliers[f] when localization or
 *     mp_nobs > 0; an outlier's map point becomes -1 only when stereo.
 * 4 orbtf_motion_project (TrackWithMotionModel's setup): on the last frames' rows frame_mappoint[i] = mp_replaced[p]
 *   where that is in [0, n_mappoints) (one step, :808-814); cur.pose[f] = velocity[f] * last.pose[f] in CameraPose's
 *   float arithmetic (:225); motion[f] from tlc (src/ORBmatcher.cc:1286-1288; baseline[f] = camera.baseline); per last
 *   keypoint the tests of :1295-1311 give mp_valid, mp_proj, mp_octave, mp_desc, mp_has_obs, mp_angle of an
 *   orbm_motion_batch with mp_begin[f] = f * last.kp_cap and kp_begin[f] = f * cur.kp_cap (rows from last.frame_n[f] up:
 *   mp_valid 0); kp_claimed = 1 on the current frame's padding, 0 elsewhere; the current frame's frame_mappoint[i],
 *   i < frame_n[f], = -1.  It takes no th: the wider search of :238-239 reuses the outputs.
 * 5 orbtf_end_frame (src/Tracking.cc:1259-1281, :490-511): n_observations[f][i] = mp_nobs, or -1 for no map point, an
 *   outlier and the padding; then a map point with mp_nobs < 1 becomes -1, its flag 0; then counts[f] = (close and
 *   tracked, close and not tracked, KeyFrame::TrackedMapPoints(min_obs[f]) of reference_kf[f]).  Close: 0 < kp_depth <
 *   th_depth (kp_depth NULL, monocular: both counts 0).  TrackedMapPoints: src/KeyFrame.cc:198-220 (min_obs <= 0 counts every point that is not bad);
 *   reference_kf[f] = -1 gives 0.  NeedNewKeyFrame's decision stays on the host.
 * 6 orbtf_drop_outliers (:1309-1313): frame_mappoint = -1 where frame_outlier is set.
 * 7 orbtf_stereo_points (CreateMapPoints :685-743, CreateMapPointsVO :745-786, StereoInitialization :980-997): the
 *   pairs (Z, i) with Z = kp_depth > 0 (NaN out, +inf in) in ascending (Z, i) order; ranks 0 .. q are processed, q the
 *   first rank with Z > th_depth and rank + 1 > 100, or the last.  A processed keypoint whose map point is null or has
 *   mp_nobs < 1 is created; ORBTF_KEYFRAME sets frame_mappoint to -1 in the second case, ORBTF_VO leaves it and
 *   unprojects as Frame::UnprojectStereo does; ORBTF_INIT creates every Z > 0 in keypoint order.  created_kp[f][..]
 *   in creation order, created_xw[f][..][3] = uvZToWorld with the frame's pose, n_created[f], n_processed[f];
 *   orbmk_create_points (Map creation, below) reads the lists in place and allocates the slots.  One workgroup per frame, the depth bits and a flag byte per keypoint in LDS (5 * kp_cap bytes; a
 *   keypoint's index is its position), a rank sort.
 * ---------------------------------------------------------------------------------------- */
#define ORBTF_MERGE 0
#define ORBTF_REPLACE 1
#define ORBTF_DISCARD 0
#define ORBTF_LOCAL_MAP 1
#define ORBTF_KEYFRAME 0
#define ORBTF_VO 1
#define ORBTF_INIT 2
#define ORBTF_MAX_LEVELS 32

typedef struct orbtf_frames {
    int32_t n_frames, kp_cap;      /* kp_cap in [1, ORBM_PROJ_MAX_KP] */
    const int32_t* frame_n;        /* [F] N */
    int32_t* frame_mappoint;       /* [F][kp_cap] slots, -1 is null */
    uint8_t* frame_outlier;        /* [F][kp_cap] */
    float* pose;                   /* [F][12] Rcw row-major, tcw */
    const float* camera;           /* [F][5] fx, fy, cx, cy, bf */
    const float* bounds;           /* [F][4] minx, maxx, miny, maxy */
    const float* kp_xy;            /* [F][kp_cap][2] keypointsUn pt */
    const int32_t* kp_octave;      /* [F][kp_cap] */
    const float* kp_uright;        /* [F][kp_cap] */
    const float* kp_depth;         /* [F][kp_cap] */
    const float* kp_angle;         /* [F][kp_cap] */
    const uint8_t* kp_desc;        /* [F][kp_cap][32] */
} orbtf_frames;

typedef struct orbtf_map {
    int32_t n_keyframes, n_mappoints, kf_cap;
    const float* mp_xw;            /* [M][3] */
    const uint8_t* mp_bad;         /* [M] */
    const int32_t* mp_nobs;        /* [M] */
    int32_t* mp_found;             /* [M] updated by orbtf_finish_pose(ORBTF_LOCAL_MAP): IncreaseFound() */
    const int32_t* mp_replaced;    /* [M] GetReplaced(), -1 for none */
    const uint8_t* mp_desc;        /* [M][32] */
    const int32_t* kf_n;           /* [K] */
    const int32_t* kf_mappoint;    /* [K][kf_cap] */
} orbtf_map;

/* The arrays of an orbba_pose_batch plus edge_kp; n_frames * kp_cap rows in the per-edge arrays. */
typedef struct orbtf_edges {
    int32_t* edge_begin;           /* [F + 1] */
    double* pose_R;                /* [F][9] */
    double* pose_t;                /* [F][3] */
    double* cam;                   /* [F][5] */
    double* xw;                    /* [E][3] */
    double* obs;                   /* [E][3] */
    double* inv_sigma2;            /* [E] */
    int32_t* edge_kp;              /* [E] */
} orbtf_edges;

/* The map-point side of an orbm_motion_batch, stride last.kp_cap, and what the current frames add. */
typedef struct orbtf_motion {
    int32_t* motion;               /* [F] */
    int32_t* kp_begin;             /* [F + 1] f * cur.kp_cap */
    int32_t* mp_begin;             /* [F + 1] f * last.kp_cap */
    uint8_t* kp_claimed;           /* [F][cur.kp_cap] */
    uint8_t* mp_valid;             /* [F][last.kp_cap] */
    float* mp_proj;                /* [F][last.kp_cap][3] */
    int32_t* mp_octave;
    uint8_t* mp_desc;              /* [F][last.kp_cap][32], 16-byte aligned as orbtf_map.mp_desc */
    uint8_t* mp_has_obs;
    float* mp_angle;
} orbtf_motion;

typedef struct orbtf_created {
    int32_t* created_kp;           /* [F][kp_cap] */
    float* created_xw;             /* [F][kp_cap][3] */
    int32_t* n_created;            /* [F] */
    int32_t* n_processed;          /* [F] */
} orbtf_created;

/* Device entries: every array in HBM; enqueue only on `stream`, nothing is copied back.  ORB_EINVAL for a NULL array
 * the entry uses, negative sizes, kp_cap outside [1, ORBM_PROJ_MAX_KP] (so no frame exceeds ORBBA_POSE_MAX_EDGES),
 * kf_cap or src_cap < 1 where used, n_levels outside [1, ORBTF_MAX_LEVELS], 65536 frames or more, an unknown mode,
 * last->n_frames != cur->n_frames.  orbtf_pose_edges keeps n_frames counts in a per-thread workspace: its calls must
 * be stream-ordered. */
int orbtf_apply_matches_device(const orbtf_frames* fr, int32_t mode, const int32_t* kp_match, const int32_t* src,
                               int32_t n_rows, int32_t src_cap, const int32_t* src_row, int32_t n_mappoints, void* stream);
int orbtf_pose_edges_device(const orbtf_frames* fr, const orbtf_map* map, const float* inv_sigma2_table, int32_t n_levels,
                            const orbtf_edges* out, void* stream);
int orbtf_finish_pose_device(const orbtf_frames* fr, const orbtf_map* map, int32_t mode, const orbtf_edges* edges,
                             const orbba_pose_result* result, int32_t localization, int32_t stereo, int32_t* n_inliers,
                             int32_t* discarded, int32_t* n_discarded, void* stream);
int orbtf_motion_project_device(const orbtf_frames* cur, const orbtf_frames* last, const orbtf_map* map,
                                const float* velocity, const float* baseline, int32_t monocular, const orbtf_motion* out,
                                void* stream);
int orbtf_end_frame_device(const orbtf_frames* fr, const orbtf_map* map, float th_depth, const int32_t* reference_kf,
                           const int32_t* min_obs, int32_t* n_observations, int32_t* counts, void* stream);
int orbtf_drop_outliers_device(const orbtf_frames* fr, void* stream);
int orbtf_stereo_points_device(const orbtf_frames* fr, const orbtf_map* map, int32_t mode, float th_depth,
                               const orbtf_created* out, void* stream);
/* Host entries: every pointer is host memory, synchronous; the updated arrays are written back.  Before anything is
 * copied, besides the checks above: frame_n in [0, kp_cap]; frame_mappoint, src, mp_replaced, kf_mappoint in
 * [-1, n_mappoints); kp_match in [-1, src_cap); src_row in [0, n_rows); reference_kf in [-1, n_keyframes); kf_n in
 * [0, kf_cap]; kp_octave of a keypoint below frame_n in [0, n_levels); edge_begin a CSR within n_frames * kp_cap and
 * edge_kp in [0, kp_cap).  ORB_EINVAL otherwise. */
int orbtf_apply_matches(const orbtf_frames* fr, int32_t mode, const int32_t* kp_match, const int32_t* src, int32_t n_rows,
                        int32_t src_cap, const int32_t* src_row, int32_t n_mappoints, int device);
int orbtf_pose_edges(const orbtf_frames* fr, const orbtf_map* map, const float* inv_sigma2_table, int32_t n_levels,
                     const orbtf_edges* out, int device);
int orbtf_finish_pose(const orbtf_frames* fr, const orbtf_map* map, int32_t mode, const orbtf_edges* edges,
                      const orbba_pose_result* result, int32_t localization, int32_t stereo, int32_t* n_inliers,
                      int32_t* discarded, int32_t* n_discarded, int device);
int orbtf_motion_project(const orbtf_frames* cur, const orbtf_frames* last, const orbtf_map* map, const float* velocity,
                         const float* baseline, int32_t monocular, const orbtf_motion* out, int device);
int orbtf_end_frame(const orbtf_frames* fr, const orbtf_map* map, float th_depth, const int32_t* reference_kf,
                    const int32_t* min_obs, int32_t* n_observations, int32_t* counts, int device);
int orbtf_drop_outliers(const orbtf_frames* fr, int device);
int orbtf_stereo_points(const orbtf_frames* fr, const orbtf_map* map, int32_t mode, float th_depth,
                        const orbtf_created* out, int device);

/* ------------------------------------------------------------------------------------------
 * Frame construction (src/System.cc): what the reference does between Extract and the Frame constructor, on the
 * extractor's HBM-resident output, batched over frames.  UndistortKeyPoints (:153-174, called at :455, :512, :570),
 * depth.convertTo + ComputeStereoFromRGBD (:515-516, :197-219), ComputeImageBounds (:177-194) and the split of cv::KeyPoint
 * into the arrays orbtf_frames, orbtl_frames and the projection batches take.  Per-element arithmetic: csrc/fr_undistort.h.
 *
 * Input: kps [F][kp_cap] and counts [F] exactly as orbx_extract_batch_device writes them with cap == kp_cap; camera [F][5]
 * = fx, fy, cx, cy, bf (orbtf_frames.camera); dist [F][5] = k1, k2, p1, p2, k3 (four coefficients: k3 = 0).  A device-side
 * count is clamped to [0, kp_cap].
 *   undistortion   cv::undistortPoints(points, points, K, distCoeffs, cv::Mat(), K) restated [ext, recalled]: double
 *                  arithmetic, exactly 5 fixed-point iterations, one rounding to float per coordinate.  icdist < 0 leaves
 *                  the loop with the first guess, as newer OpenCV does (parity unpinned).  k1 == 0.f copies the keypoints
 *                  bit for bit and gives the bounds (0, cols, 0, rows) (:155, :182).
 *   ORBFR_RGBD     v = (int)pt.y, u = (int)pt.x of the distorted keypoint, d = depth(v, u) * depth_factor in float (the
 *                  convertTo folded into the lookup: uint16 or float elements, frame f at depth + f * depth_frame_stride
 *                  bytes, rows depth_step bytes apart); d > 0: kp_depth = d, kp_uright = xUn - bf / d; else both -1 (NaN,
 *                  zeros, negatives; +inf is positive).  A coordinate that is NaN or outside the image gives -1 / -1 (a
 *                  departure: the reference reads outside the depth map; extractor output never does).
 *   ORBFR_MONO     kp_uright = kp_depth = -1.
 *   ORBFR_STEREO   kp_uright / kp_depth are not touched: the caller points them at orbx_stereo_matches_batch_device's
 *                  outputs (src/System.cc:455-461).
 * Output, stride kp_cap, each pointer optional (NULL: not written): frame_n = the clamped count, kp_xy / kp_octave /
 * kp_angle, kp_un = the full undistorted records (keypointsUn, the kf_keypoint form of orblm_batch and orbba_window_map;
 * it may be kps itself), kp_uright / kp_depth, bounds [F][4] = minx, maxx, miny, maxy, frame_mappoint = -1,
 * frame_outlier = 0, kp_begin [F + 1] = f * kp_cap.  Rows from frame_n[f] up are padding and stay as they were.
 * Descriptors are not touched: the extractor's d_desc already is kp_desc.  Frames are independent; no atomics: two runs
 * are byte-identical.  Reference quirk: TrackMonocular never computes imageBounds_; a caller reproducing
 * that passes bounds = NULL and its own array to the searches.
 * ---------------------------------------------------------------------------------------- */
#define ORBFR_MONO 0
#define ORBFR_STEREO 1
#define ORBFR_RGBD 2
#define ORBFR_DEPTH_U16 0
#define ORBFR_DEPTH_F32 1

typedef struct orbfr_input {
    int32_t n_frames, kp_cap;      /* kp_cap in [1, ORBM_PROJ_MAX_KP] */
    int32_t rows, cols;            /* the image, at least 1 x 1 */
    int32_t mode;                  /* ORBFR_MONO, ORBFR_STEREO, ORBFR_RGBD */
    int32_t depth_type;            /* ORBFR_DEPTH_U16, ORBFR_DEPTH_F32 (ORBFR_RGBD only, as the four fields below) */
    const orbx_keypoint* kps;      /* [F][kp_cap] */
    const int32_t* counts;         /* [F] */
    const float* camera;           /* [F][5] fx, fy, cx, cy, bf */
    const float* dist;             /* [F][5] k1, k2, p1, p2, k3 */
    const void* depth;             /* F depth images of rows x cols elements */
    size_t depth_frame_stride;     /* bytes between frames */
    size_t depth_step;             /* bytes between rows: at least cols elements, a multiple of the element size */
    float depth_factor;            /* depthFactor_ (1 / DepthMapFactor) */
} orbfr_input;

typedef struct orbfr_frames {
    int32_t* frame_n;              /* [F] */
    float* kp_xy;                  /* [F][kp_cap][2] keypointsUn pt */
    int32_t* kp_octave;            /* [F][kp_cap] */
    float* kp_angle;               /* [F][kp_cap] */
    orbx_keypoint* kp_un;          /* [F][kp_cap] keypointsUn */
    float* kp_uright;              /* [F][kp_cap] */
    float* kp_depth;               /* [F][kp_cap] */
    float* bounds;                 /* [F][4] */
    int32_t* frame_mappoint;       /* [F][kp_cap] */
    uint8_t* frame_outlier;        /* [F][kp_cap] */
    int32_t* kp_begin;             /* [F + 1] */
} orbfr_frames;

/* Device entry: every array in HBM; one launch enqueued on `stream`, nothing is copied back.  ORB_EINVAL for a NULL struct,
 * a NULL kps, counts, camera or dist (depth in ORBFR_RGBD), negative n_frames or 65536 frames or more, kp_cap outside
 * [1, ORBM_PROJ_MAX_KP], rows or cols below 1, an unknown mode or depth type, a depth_step below cols elements or not a
 * multiple of the element size, a depth_frame_stride that is not such a multiple or (more than one frame) shorter than a
 * frame, a depth pointer not aligned to its element. */
int orbfr_build_frames_device(const orbfr_input* in, const orbfr_frames* out, void* stream);
/* Host entry: every pointer is host memory, synchronous; the requested outputs are written back.  Before anything is
 * copied, besides the checks above: counts in [0, kp_cap].  ORB_EINVAL otherwise. */
int orbfr_build_frames(const orbfr_input* in, const orbfr_frames* out, int device);
/* Plain CPU functions of the same arithmetic, for the reference's own once-per-run shape (imageBounds_ is computed for
 * the first frame only, src/System.cc:464-465, :519-520).  camera: fx, fy, cx, cy; dist: k1, k2, p1, p2, k3; bounds: minx,
 * maxx, miny, maxy.  orbfr_undistort_points is UndistortKeyPoints on n points (x, y) (out may be xy). */
int orbfr_image_bounds(int32_t rows, int32_t cols, const float* camera, const float* dist, float* bounds);
int orbfr_undistort_points(const float* camera, const float* dist, const float* xy, int32_t n, float* out);

/* ------------------------------------------------------------------------------------------
 * Map creation: the two places where the map grows, in place on the tables above.  KeyFrame::KeyFrame(const Frame&, ...)
 * (src/KeyFrame.cc:51-64) and MapPoint::MapPoint(Xw, referenceKF, map) (src/MapPoint.cc:44-56) with the calls that follow
 * a construction: AddObservation, ComputeDistinctiveDescriptors, KeyFrame::AddMapPoint, Map::AddMapPoint and the frame's
 * own pointer (src/Tracking.cc:724-736, :981-997, :1104-1126; src/LocalMapping.cc:562-575).  Per-element rules:
 * csrc/mk_create.h.  Integers and copied float bits only; no atomics: two runs are byte-identical.  The KeyFrame* <->
 * slot table, NeedNewKeyFrame's decision and the choice of a keyframe's slot stay on the host.  A slot or an index read
 * from device memory is not trusted: one outside its table is skipped, and no store leaves a table.
 *
 * orbmk_insert_keyframes: item i = (item_frame[i], item_kf[i], item_id[i], item_baseline[i]) fills keyframe row k =
 * item_kf[i] from frame f = item_frame[i] of an orbtf_frames / orbfr_frames batch.  For j < frame_n[f] (clamped to
 * [0, kp_cap]): kf_mappoint = frame_mappoint (outliers included, as mappoints_(frame.mappoints) copies them), kf_keypoint
 * = kp_un, kf_kp_octave, kf_uright, kf_depth, kf_desc = kp_desc.  Rows from frame_n[f] up to kf_cap: kf_mappoint = -1,
 * the other per-keypoint arrays are left as they are.  kf_n = the clamped count, kf_pose = pose (SetPose), kf_camera =
 * camera[5] and the item's baseline, kf_id = the item's id, kf_bad = kf_not_erase = kf_to_be_erased = 0, kf_parent = -1,
 * kf_first_connection = 1, n_conn = n_ord = 0, the four connection rows slot -1 / weight 0 up to conn_cap, kf_covis = -1.
 * Every pointer of orbmk_keyframes is optional (NULL: not written); the frame array behind a table that is written is
 * required, as are item_id with kf_id and item_baseline with kf_camera.  kp_cap <= kf_cap.  An item whose frame or slot
 * is outside its table is skipped.  Two items with one slot: the host form refuses them; on the device form the result
 * is unspecified, but every store stays inside its table.  One launch, a grid over (item, keypoint).
 *
 * orbmk_create_points: a list batch.  Item i has the keyframes kf1[i] and kf2[i] (kf2 NULL or kf2[i] = -1: one
 * observation) and the entries j < n_list[i] (clamped to [0, list_cap]) idx1[i][j], idx2[i][j], rows list_cap apart.
 * The values xw [..][3] and the optional normal [..][3], max_distance, min_distance of entry (i, j) are at row i *
 * list_cap + j, or at row i * list_cap + idx1[i][j] with values_by_keypoint.  This reads both producers in place:
 *   orbtf_created     kf1 = the new keyframe's slot, idx1 = created_kp, xw = created_xw, n_list = n_created, list_cap =
 *                     kp_cap, one observation; item_frame = the frame, so that frame_mappoint gets the slot (:735, :996);
 *   orblm_points      one item per plan entry, rounds in order: idx1 = new_idx1, idx2 = new_idx2, n_list = n_created, xw,
 *                     normal, max_distance, min_distance by keypoint, list_cap = cap1;
 *   the monocular initial map (:1104-1126): kf1 = the current keyframe (the points' reference keyframe), kf2 = the
 *                     initial one, list position i = keypoint i of the initial keyframe: idx2[i] = i, idx1[i] =
 *                     initMatches[i] or -1 where nothing was triangulated, xw = the initializer's p3d by position.
 * An entry is valid when its keyframe slot(s) are inside the table, 0 <= idx1 < kf_n[kf1], 0 <= idx2 < kf_n[kf2] where
 * there is a second keyframe, kf1 != kf2, and with values_by_keypoint idx1 < list_cap.  An invalid entry is dropped:
 * created[i][j] = -1, and it takes no slot.
 * Allocation.  alloc[0] (HBM, clamped to [0, n_mappoints]) is the number of map-point slots in use.  The caller keeps
 * the slots [alloc[0], n_mappoints) free: mp_bad = 1, mp_nobs = 0, rows that hold only -1; a free slot's row
 * [mp_obs_off[p], mp_obs_off[p + 1]) is what the caller provisioned (orbmm_grow_observations' extra); mp_obs_off is
 * never rewritten.  The valid entries are numbered in creation order, items ascending and list positions ascending, and
 * number r takes slot alloc[0] + r: the reference's nextId order.  A count per 256 list positions, one scan, the fill.
 * Everything is checked before anything is written.  The call fails whole when the total does not fit n_mappoints, when
 * a slot it would take has a row shorter than its observations, or when the batch does not fit recent: status[0] =
 * ORBMK_OVERFLOW, needed[0] = the slot count required (alloc[0] + the valid entries), needed[1] = the first slot whose
 * row is too short, or -1 (also when the total does not fit); no table changes, alloc[0] and n_recent[0] stay, created
 * is -1 and n_created 0.  Otherwise status[0] = ORBMK_OK, needed = (the new alloc[0], -1) and alloc[0] advances.
 * Per created point p: mp_xw = the given point; mp_normal and mp_max_min = the given values (max, min), zeros where not
 * given: the constructor's state, to be followed by orbmm_update_normal_depth_device over `created`; mp_bad = 0,
 * mp_replaced = -1, mp_found = mp_visible = 1, mp_first_kf_id = kf_id[kf1], mp_ref_kf = kf1; the row's live entries are
 * the one or two observations in ascending keyframe slot (the rule of the observation edits above), the rest of the row
 * -1; mp_nobs = the sum over them of kf_uright >= 0 ? 2 : 1; kf_mappoint[kf1][idx1] = kf_mappoint[kf2][idx2] = p;
 * mp_desc[p] = the kf_desc row of the first live entry whose keyframe is not bad (ComputeDistinctiveDescriptors for
 * N <= 2, src/MapPoint.cc:300-314: both medians are 0), not written when there is none.  kf_bad NULL: none is bad.
 * kf_desc / mp_desc, mp_normal and mp_max_min may be NULL (not written).
 * Optional outputs: frame_mappoint[item_frame[i]][idx1] = p (an item_frame outside [0, n_frames) or idx1 >= kp_cap: not
 * written); created [n_items][list_cap], -1 where no point was created, and n_created[i]; recent[n_recent[0] ..] gets the
 * created slots in creation order and n_recent[0] advances (recentAddedMapPoints_.push_back, LocalMapping.cc:575).
 * The same keypoint of one keyframe twice in a call: the host form refuses it; on the device form the result is
 * unspecified, but every store stays inside its table.
 * Intended range: a keyframe's batch (tens of items, hundreds to a few thousand points); the decision is one workgroup,
 * serial in n_items * ceil(list_cap / 256) and in the slots taken.
 * Workspace (per thread, grow-only): 4 * (n_items * ceil(list_cap / 256) + 5) bytes.
 * ---------------------------------------------------------------------------------------- */
#define ORBMK_OK 0
#define ORBMK_OVERFLOW 1

typedef struct orbmk_frames {
    int32_t n_frames, kp_cap;
    const int32_t* frame_n;           /* [F] */
    const int32_t* frame_mappoint;    /* [F][kp_cap] */
    const orbx_keypoint* kp_un;       /* [F][kp_cap] keypointsUn (orbfr_frames.kp_un) */
    const int32_t* kp_octave;         /* [F][kp_cap] */
    const float* kp_uright;           /* [F][kp_cap] */
    const float* kp_depth;            /* [F][kp_cap] */
    const uint8_t* kp_desc;           /* [F][kp_cap][32], 16-byte aligned */
    const float* pose;                /* [F][12] */
    const float* camera;              /* [F][5] fx, fy, cx, cy, bf */
} orbmk_frames;

typedef struct orbmk_keyframes {      /* every pointer optional */
    int32_t n_keyframes, kf_cap, conn_cap;
    int32_t* kf_id;                   /* [K] */
    int32_t* kf_n;                    /* [K] */
    int32_t* kf_mappoint;             /* [K][kf_cap] */
    orbx_keypoint* kf_keypoint;       /* [K][kf_cap] */
    int32_t* kf_kp_octave;            /* [K][kf_cap] */
    float* kf_uright;                 /* [K][kf_cap] */
    float* kf_depth;                  /* [K][kf_cap] */
    uint8_t* kf_desc;                 /* [K][kf_cap][32], 16-byte aligned */
    float* kf_pose;                   /* [K][12] */
    float* kf_camera;                 /* [K][6] fx, fy, cx, cy, bf, baseline */
    uint8_t* kf_bad; uint8_t* kf_not_erase; uint8_t* kf_to_be_erased;   /* [K] */
    int32_t* kf_parent;               /* [K] */
    uint8_t* kf_first_connection;     /* [K] */
    int32_t* conn_slot; int32_t* conn_weight; int32_t* n_conn;          /* orbmm_graph's */
    int32_t* ord_slot; int32_t* ord_weight; int32_t* n_ord;
    int32_t* kf_covis;                /* [K][ORBDB_COVIS] */
} orbmk_keyframes;

typedef struct orbmk_map {
    int32_t n_keyframes, n_mappoints, kf_cap;
    int32_t n_obs;                    /* entries of mp_obs_kf / mp_obs_idx (>= mp_obs_off[n_mappoints]) */
    const int32_t* kf_id;             /* [K] */
    const int32_t* kf_n;              /* [K] */
    int32_t*       kf_mappoint;       /* [K][kf_cap] updated */
    const float*   kf_uright;         /* [K][kf_cap] */
    const uint8_t* kf_bad;            /* [K] optional */
    const uint8_t* kf_desc;           /* [K][kf_cap][32] optional, with mp_desc */
    uint8_t*       mp_bad;            /* [M] */
    float*         mp_xw;             /* [M][3] */
    float*         mp_normal;         /* [M][3] optional */
    float*         mp_max_min;        /* [M][2] optional */
    int32_t*       mp_nobs;           /* [M] */
    int32_t*       mp_found;          /* [M] */
    int32_t*       mp_visible;        /* [M] */
    int32_t*       mp_replaced;       /* [M] */
    int32_t*       mp_first_kf_id;    /* [M] */
    int32_t*       mp_ref_kf;         /* [M] */
    uint8_t*       mp_desc;           /* [M][32] optional, 16-byte aligned */
    const int32_t* mp_obs_off;        /* [M + 1] */
    int32_t*       mp_obs_kf;
    int32_t*       mp_obs_idx;
} orbmk_map;

typedef struct orbmk_lists {
    int32_t n_items, list_cap;
    int32_t values_by_keypoint;       /* 0: the values of entry (i, j) at row i * list_cap + j; 1: at i * list_cap + idx1 */
    const int32_t* kf1;               /* [n_items] */
    const int32_t* kf2;               /* [n_items] or NULL */
    const int32_t* n_list;            /* [n_items] */
    const int32_t* idx1;              /* [n_items][list_cap] */
    const int32_t* idx2;              /* [n_items][list_cap]; required with kf2 */
    const float* xw;                  /* [n_items][list_cap][3] */
    const float* normal;              /* [n_items][list_cap][3] or NULL */
    const float* max_distance;        /* [n_items][list_cap] or NULL */
    const float* min_distance;        /* [n_items][list_cap] or NULL */
    int32_t n_frames, kp_cap;         /* of frame_mappoint; ignored when that is NULL */
    const int32_t* item_frame;        /* [n_items]; required with frame_mappoint */
    int32_t* frame_mappoint;          /* [n_frames][kp_cap] or NULL; updated */
} orbmk_lists;

typedef struct orbmk_created {
    int32_t* alloc;                   /* [1] input and output */
    int32_t* status;                  /* [1] ORBMK_* */
    int32_t* needed;                  /* [2] */
    int32_t* created;                 /* [n_items][list_cap] or NULL */
    int32_t* n_created;               /* [n_items] or NULL */
    int32_t* recent;                  /* [recent_cap] or NULL */
    int32_t* n_recent;                /* [1] input and output; required with recent */
    int32_t recent_cap;
} orbmk_created;

/* Device forms: every array in HBM (the structs themselves are host memory); enqueue only on `stream`, nothing is copied
 * back.  ORB_EINVAL for a NULL struct or required array, negative sizes, kp_cap, kf_cap or list_cap < 1, kp_cap > kf_cap,
 * conn_cap < 1 with a connection row given, 65536 items or more, a table of 2^31 entries or more, descriptors not 16-byte
 * aligned (device forms), kf_desc without mp_desc or the reverse, values_by_keypoint not 0 or 1.  The workspace belongs to the calling
 * thread: its calls must be stream-ordered. */
int orbmk_insert_keyframes_device(const orbmk_frames* frames, const orbmk_keyframes* keyframes, int32_t n_items,
                                  const int32_t* item_frame, const int32_t* item_kf, const int32_t* item_id,
                                  const float* item_baseline, void* stream);
int orbmk_create_points_device(const orbmk_map* map, const orbmk_lists* lists, const orbmk_created* out, void* stream);
/* Host forms: every pointer is host memory, synchronous; the updated arrays are written back.  Before anything is
 * copied, besides the checks above: item_frame in [0, n_frames), item_kf in [0, n_keyframes) and no slot twice, frame_n
 * in [0, kp_cap]; the offsets start at 0, do not decrease and end within n_obs, kf_n in [0, kf_cap], kf1 in
 * [0, n_keyframes), kf2 in [-1, n_keyframes), n_list in [0, list_cap], idx1 and idx2 in [-1, kf_cap) (-1: no entry),
 * the lists' item_frame in [-1, n_frames), alloc[0] in [0, n_mappoints], n_recent[0] in [0, recent_cap], no keypoint of
 * a keyframe twice among the valid entries.  ORB_EINVAL otherwise. */
int orbmk_insert_keyframes(const orbmk_frames* frames, const orbmk_keyframes* keyframes, int32_t n_items,
                           const int32_t* item_frame, const int32_t* item_kf, const int32_t* item_id,
                           const float* item_baseline, int device);
int orbmk_create_points(const orbmk_map* map, const orbmk_lists* lists, const orbmk_created* out, int device);

const char* orb_last_error(void);
int orb_device_count(void);

/* Compact descriptor block for the multi-GPU exchange (BASELINE configs[4]: frame i matched to i-1
 * across shard boundaries; no reference counterpart, the reference runs one camera stream): frame f's
 * first counts[f] descriptor rows of desc (n_frames x cap x 32 bytes, the orbx_extract_batch_device
 * layout) go to out rows [incl[f] - counts[f], incl[f]), with incl the inclusive prefix sum of counts.
 * out holds out_rows rows: rows outside [0, out_rows) are not written, and a count outside [0, cap]
 * copies min(max(counts[f], 0), cap) rows (the device-side counts are never trusted to stay inside the
 * buffers).  counts / incl / desc / out are device memory; enqueue only on `stream`.  One launch,
 * 32-byte rows as two 16-byte vector copies. */
int orbx_pack_descriptors(const uint8_t* desc, int32_t cap, const int32_t* counts, const int32_t* incl,
                          int32_t n_frames, uint8_t* out, int32_t out_rows, void* stream);

/* Stage timing with HIP events recorded as part of each kernel's dispatch (hipExtLaunchKernel start /
 * stop events: the kernel's own duration) for the stages 0 pyramid, 1 FAST cells, 2 quadtree,
 * 3 describe.  enable > 0 times every stage, enable < 0 only the stages in the bitmask -enable
 * (e.g. -2: FAST cells only), 0 stops; read synchronises, returns the summed milliseconds and
 * launch count per stage, and resets. */
#define ORBX_NSTAGES 4
int orbx_profile_enable(orbx_extractor* h, int enable);
int orbx_profile_read(orbx_extractor* h, double* ms, int32_t* launches);

/* ------------------------------------------------------------------------------------------
 * Diagnostics (used by the per-stage parity tests; synchronous, host memory).
 * ---------------------------------------------------------------------------------------- */
/* FAST candidates of (frame, level) of the last batch, in DetectFAST's push order (cell raster,
 * row-major inside a cell): packed x | y << 12 | score << 24.  *n = count (cap-limited copy). */
int orbx_debug_level_candidates(const orbx_extractor* h, int frame, int level, uint32_t* out, int cap, int* n);
/* Runs the quadtree's on-device std::sort emulation (one wavefront) on `sizes`: perm[k] = index of
 * the element that std::sort(size-descending, src/ORBextractor.cc:642-643) puts at position k. */
int orbx_debug_qt_sort(const int32_t* sizes, int n, int32_t* perm);
/* PoseOptimization's cross-lane sums on one wavefront: in = 64 lanes x 32 doubles (lane-major);
 * scatter[l] = wave total of value l >> 1 (reduce-scatter butterfly), sum[l] = wave total of
 * in[*][0] (all-reduce).  Checks the permlane / DPP lane mapping against a host sum. */
int orbba_debug_po_wave(const double* in, double* scatter, double* sum);
/* Quadtree output of (frame, level) of the last batch (list order, packed as above). */
int orbx_debug_level_selected(const orbx_extractor* h, int frame, int level, uint32_t* out, int cap, int* n);
/* describe alone, on planted keypoints.  imgs: n_frames host frames of rows x cols, rows `step` bytes apart,
 * frame f at imgs + f * rows * step.  points: n planted keypoints as int32 (level, x, y, score), x / y in
 * level coordinates; every frame gets the same points.  The pyramid is built as Extract builds it (same
 * kernels, same handle switches), the points are written as the quadtree's selection words and per-level
 * counts (in the given order within a level), and describe_prefix_kernel plus the describe launch the handle
 * is configured for run on them (slot table, ORBX_DESC_DENSE, ORBX_DESC_C with the overflow kernel; the
 * trig mode of orbx_set_opencv_compat).  kps / desc receive n_frames x n records / 32-byte descriptors:
 * per frame level-major, then plant order.  ORB_EINVAL, before anything is launched, for a level outside
 * [0, nlevels) or one that takes no keypoints, x outside [19, w - 19) or y outside [19, h - 19) of the
 * level (FAST's range: a planted point reads nothing Extract could not reach), a score outside 0..255, or
 * more points on a level than its selection capacity (the level's share of orbx_max_keypoints). */
int orbx_debug_describe(orbx_extractor* h, const uint8_t* imgs, int n_frames, int rows, int cols, size_t step,
                        const int32_t* points, int n, orbx_keypoint* kps, uint8_t* desc);

#ifdef __cplusplus
}
#endif
#endif /* ORBSLAM2_AMD_H */
