// orbslam2_amd.hpp — C++ drop-in classes over the C-ABI (include/orbslam2_amd.h).
//
// They keep the reference's class / method shapes so Tracking and LocalMapping call them
// unchanged:
//   ORB_SLAM2_AMD::ORBextractor   <- ORB_SLAM2::ORBextractor   (include/ORBextractor.h:35-81)
//   ORB_SLAM2_AMD::ORBmatcher     <- ORB_SLAM2::ORBmatcher Hamming kernels (include/ORBmatcher.h)
//   ORB_SLAM2_AMD::LocalBundleAdjustment <- Optimizer::LocalBundleAdjustment (include/Optimizer.h:47)
//   ORB_SLAM2_AMD::BundleAdjustment, GlobalBAUpdateMap <- Optimizer::BundleAdjustment (src/Optimizer.cc:197-343) and
//                                            the GlobalBA thread's map update (src/LoopClosing.cc:392-446)
//   ORB_SLAM2_AMD::PoseOptimization      <- Optimizer::PoseOptimization (include/Optimizer.h:49)
//   ORB_SLAM2_AMD::Optimizer::OptimizeSim3 <- Optimizer::OptimizeSim3 (src/Optimizer.cc:944-1100)
//   ORB_SLAM2_AMD::Optimizer::OptimizeEssentialGraph <- Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:743-942)
//   ORB_SLAM2_AMD::SearchByProjection    <- ORBmatcher::SearchByProjection(Frame&, vector<MapPoint*>, th)
//   ORB_SLAM2_AMD::ORBVocabulary         <- DBoW2 ORBVocabulary (include/ORBVocabulary.h) transform
// Plain-type overloads are always available; when OpenCV is on the include path the
// cv::Mat / cv::KeyPoint overloads with the reference's exact signatures are added.
// A non-zero C status is turned into an exception, as the reference's CV_Assert does.
#ifndef ORBSLAM2_AMD_HPP
#define ORBSLAM2_AMD_HPP

#include <algorithm>
#include <cstdint>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "orbslam2_amd.h"

#if defined(__has_include)
#if __has_include(<opencv2/core.hpp>)
#include <opencv2/core.hpp>
#define ORBSLAM2_AMD_HAVE_OPENCV 1
#endif
#endif

namespace ORB_SLAM2_AMD {

inline void check(int rc, const char* what) {
    if (rc != ORB_OK) throw std::runtime_error(std::string(what) + ": " + orb_last_error());
}

class ORBextractor {
public:
    struct Parameters {   // include/ORBextractor.h:39-47
        int nfeatures;
        float scaleFactor;
        int nlevels;
        int iniThFAST;
        int minThFAST;
        Parameters(int nfeatures = 2000, float scaleFactor = 1.2f, int nlevels = 8, int iniThFAST = 20,
                   int minThFAST = 7)
            : nfeatures(nfeatures), scaleFactor(scaleFactor), nlevels(nlevels), iniThFAST(iniThFAST),
              minThFAST(minThFAST) {}
    };

    explicit ORBextractor(const Parameters& p, int device = 0) : param_(p) {
        orbx_params c{p.nfeatures, p.scaleFactor, p.nlevels, p.iniThFAST, p.minThFAST};
        check(orbx_create(&c, device, &h_), "orbx_create");
        const int L = p.nlevels;
        scale_.resize(L); inv_.resize(L); s2_.resize(L); is2_.resize(L);
        check(orbx_scale_tables(h_, scale_.data(), inv_.data(), s2_.data(), is2_.data(), nullptr), "orbx_scale_tables");
    }
    ~ORBextractor() { orbx_destroy(h_); }
    ORBextractor(const ORBextractor&) = delete;
    ORBextractor& operator=(const ORBextractor&) = delete;

    // The OpenCV-build switches (orbslam2_amd.h orbx_set_opencv_compat): trig_mode 0
    // ::cos(double) / 1 cosf for src/ORBextractor.cc:107, resize_simd = the cv::resize SIMD width V.
    // -1 keeps a switch.
    void SetOpenCVCompat(int trig_mode, int resize_simd) {
        check(orbx_set_opencv_compat(h_, trig_mode, resize_simd), "orbx_set_opencv_compat");
    }

    // Extract on a raw CV_8U image.  Returns false (outputs untouched) when no keypoint exists —
    // the reference's early return (src/ORBextractor.cc:778-782).
    bool Extract(const uint8_t* img, int rows, int cols, size_t step, std::vector<orbx_keypoint>& keypoints,
                 std::vector<uint8_t>& descriptors) {
        int32_t cap = 0;
        check(orbx_max_keypoints(h_, rows, cols, &cap), "orbx_max_keypoints");
        kbuf_.resize(cap);
        dbuf_.resize((size_t)cap * 32);
        int n = 0;
        check(orbx_extract(h_, img, rows, cols, step, kbuf_.data(), dbuf_.data(), cap, &n), "orbx_extract");
        if (n == 0) {
            descriptors.clear();
            return false;
        }
        keypoints.assign(kbuf_.begin(), kbuf_.begin() + n);
        descriptors.assign(dbuf_.begin(), dbuf_.begin() + (size_t)n * 32);
        return true;
    }

#ifdef ORBSLAM2_AMD_HAVE_OPENCV
    // void Extract(const cv::Mat& image, KeyPoints& keypoints, cv::Mat& descriptors)
    void Extract(const cv::Mat& image, std::vector<cv::KeyPoint>& keypoints, cv::Mat& descriptors) {
        CV_Assert(image.type() == CV_8U);
        std::vector<orbx_keypoint> k;
        std::vector<uint8_t> d;
        if (!Extract(image.data, image.rows, image.cols, image.step, k, d)) {
            descriptors.release();   // keypoints left untouched, as the reference
            return;
        }
        keypoints.resize(k.size());
        for (size_t i = 0; i < k.size(); i++)
            keypoints[i] = cv::KeyPoint(k[i].x, k[i].y, k[i].size, k[i].angle, k[i].response, k[i].octave,
                                        k[i].class_id);
        descriptors.create((int)k.size(), 32, CV_8U);
        std::copy(d.begin(), d.end(), descriptors.data);
    }
#endif

    int GetLevels() const { return param_.nlevels; }
    float GetScaleFactor() const { return param_.scaleFactor; }
    const std::vector<float>& GetScaleFactors() const { return scale_; }
    const std::vector<float>& GetInverseScaleFactors() const { return inv_; }
    const std::vector<float>& GetScaleSigmaSquares() const { return s2_; }
    const std::vector<float>& GetInverseScaleSigmaSquares() const { return is2_; }

    // GetImagePyramid(): level s of the last image, copied to host memory.
    std::vector<uint8_t> GetImagePyramidLevel(int s, int* rows, int* cols) const {
        check(orbx_pyramid_level(h_, s, nullptr, 0, rows, cols), "orbx_pyramid_level");
        std::vector<uint8_t> out((size_t)(*rows) * (*cols));
        check(orbx_pyramid_level(h_, s, out.data(), (size_t)(*cols), rows, cols), "orbx_pyramid_level");
        return out;
    }

    orbx_extractor* handle() const { return h_; }

private:
    Parameters param_;
    orbx_extractor* h_ = nullptr;
    std::vector<float> scale_, inv_, s2_, is2_;
    std::vector<orbx_keypoint> kbuf_;
    std::vector<uint8_t> dbuf_;
};

class ORBmatcher {
public:
    explicit ORBmatcher(float nnratio = 0.6f, bool checkOri = true) : nnratio_(nnratio), checkOri_(checkOri) {}

    // static int DescriptorDistance(const cv::Mat& a, const cv::Mat& b) on 32-byte rows
    static int DescriptorDistance(const uint8_t* a, const uint8_t* b) { return orbm_descriptor_distance(a, b); }

    // Brute-force best / second-best + ratio test over all rows (reference loop semantics).  With
    // checkOri (the default, as the reference's ORBmatcher(nnratio, checkOri=true)) CheckOrientation
    // (ORBmatcher.cc:249-309) filters `match` as SearchForInitialization applies it (:676-686); the
    // keypoint angles are then required.  Returns the match count.
    int MatchBruteForce(const uint8_t* A, int nA, const uint8_t* B, int nB, std::vector<int>& match, int th_low = 50,
                        const float* angleA = nullptr, const float* angleB = nullptr) const {
        if (checkOri_ && (!angleA || !angleB))
            throw std::invalid_argument("ORBmatcher(checkOri=true)::MatchBruteForce needs the keypoint angles");
        std::vector<int32_t> bi(nA), bd(nA), sd(nA), m(nA);
        check(orbm_bf_match(A, nA, B, nB, nnratio_, th_low, bi.data(), bd.data(), sd.data(), m.data()), "orbm_bf_match");
        int32_t n = 0;
        for (int i = 0; i < nA; i++) n += m[i] >= 0;
        if (checkOri_) check(orbm_check_orientation(angleA, nA, angleB, nB, m.data(), &n), "orbm_check_orientation");
        match.assign(m.begin(), m.end());
        return n;
    }

    // int SearchForTriangulation(kf1, kf2, F12, matchIds, onlyStereo) on flattened keyframes.
    int SearchForTriangulation(const orbm_tri_frame& kf1, const orbm_tri_frame& kf2, const float F12[9],
                               const float ep2[2], const std::vector<float>& scale2, const std::vector<float>& sigma2,
                               std::vector<std::pair<size_t, size_t>>& matchIds, bool onlyStereo) const {
        std::vector<int32_t> m12(kf1.n);
        int32_t n = 0;
        check(orbm_search_for_triangulation(&kf1, &kf2, F12, ep2, scale2.data(), sigma2.data(), (int)scale2.size(),
                                            onlyStereo ? 1 : 0, m12.data(), &n),
              "orbm_search_for_triangulation");
        matchIds.clear();
        matchIds.reserve(n);
        for (int i = 0; i < kf1.n; i++)
            if (m12[i] >= 0) matchIds.emplace_back((size_t)i, (size_t)m12[i]);
        return n;
    }

    // int SearchByBoW(KeyFrame* keyframe, Frame& frame, std::vector<MapPoint*>& matches)
    // (src/ORBmatcher.cc:452-516), batched on HBM-resident slots: the batch's nnratio and
    // check_orientation are taken from this matcher.  Enqueue only; d_match[p*cap2 + idx2] = idx1 or -1
    // (the caller maps idx1 to keyframe->GetMapPointMatches()[idx1]), d_nmatches[p] = the return value.
    void SearchByBoWBatch(orbm_bow_batch b, int32_t* d_match, int32_t* d_nmatches, void* stream = nullptr) const {
        b.nnratio = nnratio_;
        b.check_orientation = checkOri_ ? 1 : 0;
        check(orbm_search_by_bow_batch_device(&b, d_match, d_nmatches, stream), "orbm_search_by_bow_batch_device");
    }

    // int SearchByBoW(KeyFrame* keyframe1, KeyFrame* keyframe2, std::vector<MapPoint*>& matches12)
    // (src/ORBmatcher.cc:696-766), batched: d_match12[p*cap1 + idx1] = idx2 or -1.
    void SearchByBoWKeyFramesBatch(orbm_bow_batch b, int32_t* d_match12, int32_t* d_nmatches,
                                   void* stream = nullptr) const {
        b.nnratio = nnratio_;
        b.check_orientation = checkOri_ ? 1 : 0;
        check(orbm_search_by_bow_kf_batch_device(&b, d_match12, d_nmatches, stream), "orbm_search_by_bow_kf_batch_device");
    }

    // int SearchForInitialization(Frame& F1, Frame& F2, std::vector<cv::Point2f>& prevMatched,
    //                             std::vector<int>& matches12, int windowSize = 10)
    // (include/ORBmatcher.h:81, src/ORBmatcher.cc:614-694) on the frames' keypointsUn (cv::KeyPoint
    // layout), 32-byte descriptors and F2's image bounds; prevMatched as (x, y) pairs, updated in place.
    // nnratio / checkOri are this matcher's (Tracking.cc:1051 builds ORBmatcher(0.9f, true)).
    int SearchForInitialization(const std::vector<orbx_keypoint>& keypointsUn1, const uint8_t* descriptors1,
                                const std::vector<orbx_keypoint>& keypointsUn2, const uint8_t* descriptors2,
                                const float bounds2[4], std::vector<float>& prevMatched, std::vector<int>& matches12,
                                int windowSize = 10, int device = 0) const {
        const int n1 = (int)keypointsUn1.size(), n2 = (int)keypointsUn2.size();
        if ((int)prevMatched.size() != 2 * n1)
            throw std::invalid_argument("SearchForInitialization: prevMatched must hold 2 floats per F1 keypoint");
        std::vector<float> xy2(2 * (size_t)n2), ang2(n2), ang1(n1);
        std::vector<int32_t> oct2(n2), oct1(n1);
        for (int i = 0; i < n2; i++) {
            xy2[2 * i] = keypointsUn2[i].x; xy2[2 * i + 1] = keypointsUn2[i].y;
            oct2[i] = keypointsUn2[i].octave; ang2[i] = keypointsUn2[i].angle;
        }
        for (int i = 0; i < n1; i++) { oct1[i] = keypointsUn1[i].octave; ang1[i] = keypointsUn1[i].angle; }
        const int32_t kb[2] = {0, n2}, qb[2] = {0, n1};
        orbm_init_batch b;
        b.n_pairs = 1; b.total_kp = n2; b.total_q = n1;
        b.kp_begin = kb; b.kp_xy = xy2.data(); b.kp_octave = oct2.data(); b.kp_desc = descriptors2; b.kp_angle = ang2.data();
        b.bounds = bounds2; b.q_begin = qb; b.q_octave = oct1.data(); b.q_desc = descriptors1; b.q_angle = ang1.data();
        b.prev_matched = prevMatched.data(); b.window = windowSize; b.nnratio = nnratio_;
        b.check_orientation = checkOri_ ? 1 : 0;
        std::vector<int32_t> m(std::max(n1, 1));
        int32_t nm = 0;
        check(orbm_search_for_initialization(&b, m.data(), &nm, device), "orbm_search_for_initialization");
        matches12.assign(m.begin(), m.begin() + n1);
        return nm;
    }

    // The same batched over initialisation pairs on HBM arrays (orbm_init_batch; nnratio / checkOri from
    // this matcher).  Enqueue only.
    void SearchForInitializationBatch(orbm_init_batch b, int32_t* d_matches12, int32_t* d_n_matches,
                                      void* stream = nullptr) const {
        b.nnratio = nnratio_;
        b.check_orientation = checkOri_ ? 1 : 0;
        check(orbm_search_for_initialization_device(&b, d_matches12, d_n_matches, stream),
              "orbm_search_for_initialization_device");
    }

    float nnratio() const { return nnratio_; }
    bool checkOrientation() const { return checkOri_; }

private:
    float nnratio_;
    bool checkOri_;
};

// void ComputeStereoMatches(keypointsL, descriptorsL, pyramidL, keypointsR, descriptorsR, pyramidR,
//                           scaleFactors, invScaleFactors, camera, uright, depth)  (src/ORBmatcher.cc:72-247)
// on raw arrays: keypoints in cv::KeyPoint layout, 32-byte descriptors, pyramid level pointers.
struct PyramidView {
    std::vector<const uint8_t*> level;
    std::vector<int32_t> rows, cols, step;
};

inline void ComputeStereoMatches(const std::vector<orbx_keypoint>& keypointsL, const uint8_t* descriptorsL,
                                 const PyramidView& pyramidL, const std::vector<orbx_keypoint>& keypointsR,
                                 const uint8_t* descriptorsR, const PyramidView& pyramidR,
                                 const std::vector<float>& scaleFactors, const std::vector<float>& invScaleFactors,
                                 float bf, float baseline, std::vector<float>& uright, std::vector<float>& depth) {
    auto view = [](const std::vector<orbx_keypoint>& k, const uint8_t* d, const PyramidView& p) {
        orbm_stereo_view v;
        v.n = (int32_t)k.size();
        v.kps = k.data();
        v.desc = d;
        v.n_levels = (int32_t)p.level.size();
        v.level = p.level.data();
        v.level_rows = p.rows.data();
        v.level_cols = p.cols.data();
        v.level_step = p.step.data();
        return v;
    };
    const orbm_stereo_view l = view(keypointsL, descriptorsL, pyramidL), r = view(keypointsR, descriptorsR, pyramidR);
    uright.assign(keypointsL.size(), -1.f);
    depth.assign(keypointsL.size(), -1.f);
    check(orbm_compute_stereo_matches(&l, &r, scaleFactors.data(), invScaleFactors.data(), bf, baseline, uright.data(),
                                      depth.data()),
          "orbm_compute_stereo_matches");
}

// The same on the two extractors' last Extract (System.cc:449-461): keypoints, descriptors and pyramids stay
// on the device; only uright / depth come back.  nLeft = keypointsLeft.size() of that Extract.
inline void ComputeStereoMatches(ORBextractor& left, ORBextractor& right, size_t nLeft, float bf, float baseline,
                                 std::vector<float>& uright, std::vector<float>& depth) {
    uright.assign(nLeft, -1.f);
    depth.assign(nLeft, -1.f);
    check(orbx_stereo_matches_last(left.handle(), right.handle(), bf, baseline, uright.data(), depth.data(),
                                   (int)nLeft),
          "orbx_stereo_matches_last");
}

// Optimizer::LocalBundleAdjustment from the flattened graph (Optimizer.cc:540-631): the caller
// gathers local / fixed keyframes and local map points exactly as :493-537, calls this, then
// erases the outlier observations and writes poses / points back under the map mutex (:677-735).
// Returns false when the stop flag was already set on entry (the reference returns at
// Optimizer.cc:633-634): nothing was optimised and nothing must be written back.
inline bool LocalBundleAdjustment(const orbba_problem& problem, orbba_result& result, const volatile int32_t* stopFlag,
                                  int device = 0) {
    check(orbba_local_ba(&problem, &result, stopFlag, device), "orbba_local_ba");
    return result.ran != 0;
}

// Optimizer::LocalBundleAdjustment(currKF, stopFlag, map) as a whole (Optimizer.cc:491-736), in place on the slot tables
// in HBM (orbba_window_map): the window gather, LocalBA staged from it on the device and the write-back, enqueued on one
// stream.  The *Host members take host arrays and are synchronous.
class LocalBA {
public:
    explicit LocalBA(const orbba_window_map& map) : map_(map) {}

    // :493-631: local keyframes, local points, fixed cameras and edges into window, in orbba_problem's order
    void Window(int32_t cur, const orbba_window& window, void* stream = nullptr) const {
        check(orbba_local_window_device(&map_, cur, &window, stream), "orbba_local_window_device");
    }
    // :677-735 on given flags and estimates (HBM, the window's order): erasures, poses, points, UpdateNormalAndDepth
    void Apply(const orbba_window& window, const uint8_t* d_outlier, const double* d_pose_R, const double* d_pose_t,
               const double* d_points, void* stream = nullptr) const {
        check(orbba_local_ba_apply_device(&map_, &window, d_outlier, d_pose_R, d_pose_t, d_points, stream),
              "orbba_local_ba_apply_device");
    }
    // The whole call.  Returns false when nothing was optimised or written: the stop flag was set on entry, or
    // result.status == ORBBA_WINDOW_OVERFLOW (result.counts are then the sizes the window needs).
    bool Run(int32_t cur, const orbba_window& window, orbba_map_result& result, const volatile int32_t* stopFlag = nullptr,
             void* stream = nullptr) const {
        check(orbba_local_ba_map_device(&map_, cur, &window, &result, stopFlag, stream), "orbba_local_ba_map_device");
        return result.ran != 0;
    }
    void WindowHost(int32_t cur, const orbba_window& window, int device = 0) const {
        check(orbba_local_window(&map_, cur, &window, device), "orbba_local_window");
    }
    void ApplyHost(const orbba_window& window, const uint8_t* outlier, const double* pose_R, const double* pose_t,
                   const double* points, int device = 0) const {
        check(orbba_local_ba_apply(&map_, &window, outlier, pose_R, pose_t, points, device), "orbba_local_ba_apply");
    }
    bool RunHost(int32_t cur, orbba_map_result& result, const volatile int32_t* stopFlag = nullptr, int device = 0) const {
        check(orbba_local_ba_map(&map_, cur, &result, stopFlag, device), "orbba_local_ba_map");
        return result.ran != 0;
    }

private:
    orbba_window_map map_;
};

// void Optimizer::BundleAdjustment(keyframes, mappoints, nIterations, stopFlag, loopKFId, robust)
// (Optimizer.cc:197-343) from the flattened graph (:212-294, pose_fixed = (id == 0)), with the reference's edge
// typing (`if (ur)`).  The caller writes result.pose_f / points_f to TcwGBA / posGBA and sets BAGlobalForKF
// (loopKFId != 0) or calls SetPose / SetWorldPos (:296-342), leaving out the points with point_included == 0.
// Returns false when the stop flag was set on entry.
inline bool BundleAdjustment(const orbba_problem& problem, orbba_gba_result& result, int nIterations = 5,
                             const volatile int32_t* stopFlag = nullptr, bool robust = true, int device = 0) {
    const orbba_gba_options opt{nIterations, robust ? 1 : 0, ORBBA_GBA_RULE_REFERENCE};
    check(orbba_bundle_adjustment(&problem, &opt, &result, stopFlag, device), "orbba_bundle_adjustment");
    return result.ran != 0;
}

// The map update of the GlobalBA thread (LoopClosing.cc:392-446) on host tables, synchronous; the ...Device form
// takes tables in HBM and only enqueues on `stream`.
inline void GlobalBAUpdateMap(const orbba_gba_map& map, int device = 0) {
    check(orbba_gba_update_map(&map, device), "orbba_gba_update_map");
}
inline void GlobalBAUpdateMapDevice(const orbba_gba_map& map, void* stream) {
    check(orbba_gba_update_map_device(&map, stream), "orbba_gba_update_map_device");
}

// int Optimizer::PoseOptimization(Frame*) (include/Optimizer.h:49, src/Optimizer.cc:345-489) over a
// batch of frames.  One PoseFrame per frame holds the keypoints that have a map point, in keypoint
// order (:364-410); R / t are frame->pose on entry and the SetPose argument on return, `outlier`
// receives frame->outlier for those keypoints.  Returns each frame's inlier count.
struct PoseFrame {
    double R[9], t[3];
    double fx, fy, cx, cy, bf;
    std::vector<double> xw;         // 3 per edge: MapPoint::GetWorldPos()
    std::vector<double> obs;        // 3 per edge: keypointsUn[i].pt.x, .y, uright[i] (< 0: monocular)
    std::vector<double> invSigma2;  // 1 per edge: pyramid.invSigmaSq[keypointsUn[i].octave]
    std::vector<uint8_t> outlier;   // out
};

inline std::vector<int> PoseOptimization(std::vector<PoseFrame>& frames, int device = 0) {
    const size_t F = frames.size();
    std::vector<int32_t> eb(F + 1, 0);
    for (size_t f = 0; f < F; f++) eb[f + 1] = eb[f] + (int32_t)frames[f].invSigma2.size();
    const size_t E = (size_t)eb[F];
    std::vector<double> R(9 * F), t(3 * F), cam(5 * F), xw(3 * E), obs(3 * E), is2(E);
    for (size_t f = 0; f < F; f++) {
        const PoseFrame& p = frames[f];
        std::copy(p.R, p.R + 9, R.begin() + 9 * f);
        std::copy(p.t, p.t + 3, t.begin() + 3 * f);
        const double c[5] = {p.fx, p.fy, p.cx, p.cy, p.bf};
        std::copy(c, c + 5, cam.begin() + 5 * f);
        std::copy(p.xw.begin(), p.xw.end(), xw.begin() + 3 * (size_t)eb[f]);
        std::copy(p.obs.begin(), p.obs.end(), obs.begin() + 3 * (size_t)eb[f]);
        std::copy(p.invSigma2.begin(), p.invSigma2.end(), is2.begin() + eb[f]);
    }
    std::vector<double> oR(9 * F), ot(3 * F);
    std::vector<int32_t> ninl(F);
    std::vector<uint8_t> outl(E);
    const orbba_pose_batch in{(int32_t)F, eb.data(), R.data(), t.data(), cam.data(), xw.data(), obs.data(), is2.data()};
    orbba_pose_result out{oR.data(), ot.data(), ninl.data(), outl.data()};
    check(orbba_pose_optimization(&in, &out, device), "orbba_pose_optimization");
    std::vector<int> result(F);
    for (size_t f = 0; f < F; f++) {
        PoseFrame& p = frames[f];
        std::copy(oR.begin() + 9 * f, oR.begin() + 9 * f + 9, p.R);
        std::copy(ot.begin() + 3 * f, ot.begin() + 3 * f + 3, p.t);
        p.outlier.assign(outl.begin() + eb[f], outl.begin() + eb[f + 1]);
        result[f] = ninl[f];
    }
    return result;
}

// int ORBmatcher::SearchByProjection(Frame&, const std::vector<MapPoint*>&, float th)
// (include/ORBmatcher.h:58, src/ORBmatcher.cc:315-382) with the frame's FeaturesGrid, for one
// frame.  `keypointsUn` / `descriptors` / `uright` are the frame's, `claimed[i]` is
// frame.mappoints[i] && ->Observations() > 0; per local map point the IsInFrustum fields
// (Tracking.cc:554-605).  Returns the match count; kpMatch[i] = index into the map point arrays
// assigned to keypoint i (frame.mappoints[i] = mappoints[kpMatch[i]]) or -1.
struct ProjectionPoints {
    std::vector<uint8_t> valid;      // trackInView && !isBad()
    std::vector<float> proj;         // 3 per point: trackProjX, trackProjY, trackProjXR
    std::vector<float> viewCos;      // trackViewCos
    std::vector<int32_t> level;      // trackScaleLevel
    std::vector<uint8_t> desc;       // 32 per point: GetDescriptor()
    std::vector<uint8_t> hasObs;     // Observations() > 0
};

inline int SearchByProjection(const std::vector<orbx_keypoint>& keypointsUn, const uint8_t* descriptors,
                              const std::vector<float>& uright, const std::vector<uint8_t>& claimed,
                              const float bounds[4], const std::vector<float>& scaleFactors,
                              const ProjectionPoints& mps, float th, float nnratio, std::vector<int32_t>& kpMatch,
                              int device = 0) {
    const int n = (int)keypointsUn.size(), m = (int)mps.valid.size();
    std::vector<float> xy(2 * (size_t)n);
    std::vector<int32_t> oct(n);
    for (int i = 0; i < n; i++) { xy[2 * i] = keypointsUn[i].x; xy[2 * i + 1] = keypointsUn[i].y; oct[i] = keypointsUn[i].octave; }
    const int32_t kb[2] = {0, n}, mb[2] = {0, m};
    orbm_proj_batch b;
    b.n_frames = 1; b.total_kp = n; b.total_mp = m;
    b.kp_begin = kb; b.kp_xy = xy.data(); b.kp_octave = oct.data(); b.kp_uright = uright.data();
    b.kp_desc = descriptors; b.kp_claimed = claimed.empty() ? nullptr : claimed.data(); b.bounds = bounds;
    b.mp_begin = mb; b.mp_valid = mps.valid.data(); b.mp_proj = mps.proj.data(); b.mp_view_cos = mps.viewCos.data();
    b.mp_level = mps.level.data(); b.mp_desc = mps.desc.data(); b.mp_has_obs = mps.hasObs.data();
    b.n_levels = (int32_t)scaleFactors.size(); b.scale_factors = scaleFactors.data(); b.th = th; b.nnratio = nnratio;
    kpMatch.assign(n, -1);
    int32_t nm = 0;
    check(orbm_search_by_projection(&b, kpMatch.data(), &nm, device), "orbm_search_by_projection");
    return nm;
}

// int ORBmatcher::SearchByProjection(Frame& currFrame, const Frame& lastFrame, float th, bool monocular)
// (src/ORBmatcher.cc:1279-1362), batched on HBM arrays (orbm_motion_batch: the caller projects the
// last frame's points with the motion-model pose and sets motion[f] from tlc / baseline, :1286-1288).
// Enqueue only; kp_match[k] = idx1 assigned to currFrame keypoint k or -1.
inline void SearchByProjectionMotionBatch(const orbm_motion_batch& b, int32_t* d_kp_match, int32_t* d_n_matches,
                                          void* stream = nullptr) {
    check(orbm_search_by_projection_motion_device(&b, d_kp_match, d_n_matches, stream),
          "orbm_search_by_projection_motion_device");
}

// int ORBmatcher::SearchByProjection(Frame& frame, KeyFrame* keyframe, const std::set<MapPoint*>& alreadyFound,
// float th, int ORBdist) (include/ORBmatcher.h:66, src/ORBmatcher.cc:1364-1445), batched over (frame,
// candidate keyframe) pairs on HBM arrays (orbm_reloc_batch: the caller marks mp_valid = mappoint &&
// !isBad() && !alreadyFound.count(mappoint) and kp_claimed = frame.mappoints[i] != nullptr).  Enqueue
// only; kp_match[k] = keyframe idx1 assigned to frame keypoint k (frame.mappoints[k] =
// keyframe->GetMapPointMatches()[idx1]) or -1.
inline void SearchByProjectionRelocBatch(const orbm_reloc_batch& b, int32_t* d_kp_match, int32_t* d_n_matches,
                                         void* stream = nullptr) {
    check(orbm_search_by_projection_reloc_device(&b, d_kp_match, d_n_matches, stream),
          "orbm_search_by_projection_reloc_device");
}
// The same for one (frame, keyframe) pair on host arrays.
inline int SearchByProjectionReloc(const orbm_reloc_batch& b, std::vector<int32_t>& kpMatch, int device = 0) {
    if (b.n_frames != 1) throw std::invalid_argument("SearchByProjectionReloc: one frame per call (use the batch form)");
    kpMatch.assign(std::max(b.total_kp, 1), -1);
    int32_t nm = 0;
    check(orbm_search_by_projection_reloc(&b, kpMatch.data(), &nm, device), "orbm_search_by_projection_reloc");
    kpMatch.resize(b.total_kp);
    return nm;
}

// int ORBmatcher::Fuse(KeyFrame*, const std::vector<MapPoint*>&, float th) (src/ORBmatcher.cc:868-980,
// chi2_gate = 1) and Fuse(KeyFrame*, const Sim3& Scw, points, th, replacePoints) (:982-1088, chi2_gate = 0,
// pose = Scw.R(), Scw.t() / s), batched over (keyframe, point list) items on HBM arrays (orbm_fuse_batch:
// the caller marks mp_valid = mappoint && !isBad() && !IsInKeyFrame(keyframe), or !alreadyFound.count(
// mappoint), on entry over distinct points).  Enqueue only; best_idx[m] = bestIdx when bestDist <= TH_LOW,
// else -1.  The caller then walks the list in order and applies Replace / AddObservation / AddMapPoint
// (:957-976) or replacePoints[i] (:1070-1084) from best_idx.
inline void FuseBatch(const orbm_fuse_batch& b, int32_t* d_best_idx, int32_t* d_best_dist, int32_t* d_n_fused,
                      void* stream = nullptr) {
    check(orbm_fuse_device(&b, d_best_idx, d_best_dist, d_n_fused, stream), "orbm_fuse_device");
}
// The same for one keyframe on host arrays; returns nfused.
inline int Fuse(const orbm_fuse_batch& b, std::vector<int32_t>& bestIdx, std::vector<int32_t>& bestDist, int device = 0) {
    if (b.n_items != 1) throw std::invalid_argument("Fuse: one keyframe per call (use the batch form)");
    bestIdx.assign(std::max(b.total_mp, 1), -1);
    bestDist.assign(std::max(b.total_mp, 1), 256);
    int32_t nf = 0;
    check(orbm_fuse(&b, bestIdx.data(), bestDist.data(), &nf, device), "orbm_fuse");
    bestIdx.resize(b.total_mp);
    bestDist.resize(b.total_mp);
    return nf;
}

// int ORBmatcher::SearchByProjection(const KeyFrame*, const Sim3& Scw, const std::vector<MapPoint*>&,
// std::vector<MapPoint*>& matched, int th) (src/ORBmatcher.cc:518-612), batched on HBM arrays: the
// orbm_fuse_batch plus d_kp_claimed[k] = matched[k] != nullptr on entry (nullptr: none).  Enqueue only;
// kp_match[k] = item-relative index of the point assigned to keypoint k (matched[k] = mappoints[idx]) or -1.
inline void SearchByProjectionSim3Batch(const orbm_fuse_batch& b, const uint8_t* d_kp_claimed, int32_t* d_kp_match,
                                        int32_t* d_n_matches, void* stream = nullptr) {
    check(orbm_search_by_projection_sim3_device(&b, d_kp_claimed, d_kp_match, d_n_matches, stream),
          "orbm_search_by_projection_sim3_device");
}

// int ORBmatcher::SearchBySim3(KeyFrame*, KeyFrame*, std::vector<MapPoint*>& matches12, const Sim3& S12, float th)
// (src/ORBmatcher.cc:1090-1277), batched over (keyframe1, keyframe2, S12) pairs on HBM arrays
// (orbm_sim3_batch: the caller marks mp1_valid = mappoints1[i1] && !matches12[i1] && !isBad() and mp2_valid =
// mappoints2[i2] && !alreadyMatched2[i2] && !isBad() on entry).  Enqueue only; match12[i1] = the agreed
// keyframe-2 index or -1 (d_match1 / d_match2, the one-way results, may be nullptr).  The caller then writes
// matches12[i1] = mappoints2[match12[i1]] (:1270).
inline void SearchBySim3Batch(const orbm_sim3_batch& b, int32_t* d_match12, int32_t* d_match1, int32_t* d_match2,
                              int32_t* d_n_found, void* stream = nullptr) {
    check(orbm_search_by_sim3_device(&b, d_match12, d_match1, d_match2, d_n_found, stream), "orbm_search_by_sim3_device");
}
// The same for one pair on host arrays; returns nfound.
inline int SearchBySim3(const orbm_sim3_batch& b, std::vector<int32_t>& match12, int device = 0) {
    if (b.n_pairs != 1) throw std::invalid_argument("SearchBySim3: one pair per call (use the batch form)");
    match12.assign(std::max(b.total_kp1, 1), -1);
    int32_t nf = 0;
    check(orbm_search_by_sim3(&b, match12.data(), nullptr, nullptr, &nf, device), "orbm_search_by_sim3");
    match12.resize(b.total_kp1);
    return nf;
}

// int Optimizer::OptimizeSim3(KeyFrame*, KeyFrame*, std::vector<MapPoint*>& matches1, Sim3& S12, float maxChi2,
// bool fixScale) (src/Optimizer.cc:944-1100; LoopClosing.cc:139), batched over (keyframe1, keyframe2, S12)
// pairs on HBM arrays in SearchBySim3's slot layout (orbba_sim3_batch: match12 is SearchBySim3Batch's output,
// mp1_valid / mp2_valid = the slot has a map point that is not bad).  Enqueue only, one launch: r.s12 = S12 on
// return, r.match12 (may alias b.match12) = the thinned matches, r.n_inliers = the return values.
struct Optimizer {
    static void OptimizeSim3Batch(const orbba_sim3_batch& b, orbba_sim3_result& r, void* stream = nullptr) {
        check(orbba_optimize_sim3_device(&b, &r, stream), "orbba_optimize_sim3_device");
    }
    // The same for one pair on host arrays: match12 (total_kp1, in / out) and s12 (13 floats R, t, s, in / out);
    // returns the inlier count.
    static int OptimizeSim3(orbba_sim3_batch b, std::vector<int32_t>& match12, float* s12, int device = 0) {
        if (b.n_pairs != 1) throw std::invalid_argument("OptimizeSim3: one pair per call (use the batch form)");
        if (match12.size() < static_cast<size_t>(b.total_kp1)) throw std::invalid_argument("OptimizeSim3: match12 is short");
        b.match12 = match12.data();
        b.s12 = s12;
        float out_s12[13];
        int32_t n = 0;
        std::vector<int32_t> thinned(std::max(b.total_kp1, 1), -1);
        orbba_sim3_result r = {out_s12, nullptr, thinned.data(), &n, nullptr};
        check(orbba_optimize_sim3(&b, &r, device), "orbba_optimize_sim3");
        std::copy(thinned.begin(), thinned.begin() + b.total_kp1, match12.begin());
        std::copy(out_s12, out_s12 + 13, s12);
        return n;
    }
    // void Optimizer::OptimizeEssentialGraph(Map*, KeyFrame* loopKF, KeyFrame* currKF, nonCorrectedSim3,
    // correctedSim3, loopConnections, bool fixScale) (src/Optimizer.cc:743-942; LoopClosing::CorrectLoop) on the slot
    // tables of orbba_essential_graph in HBM.  Enqueue only: r.sim3_g2o, r.pose and r.points are what :911-941 write
    // back, r.iterations / r.chi2 / r.accept the Levenberg trace.
    static void OptimizeEssentialGraphDevice(const orbba_essential_graph& g, orbba_essential_graph_result& r,
                                             void* stream = nullptr) {
        check(orbba_optimize_essential_graph_device(&g, &r, stream), "orbba_optimize_essential_graph_device");
    }
    // The same on host arrays: pose (n_keyframes x 12) and points (n_points x 3, in / out) as SetPose and SetWorldPos
    // receive them; returns the iterations run.
    static int OptimizeEssentialGraph(orbba_essential_graph g, std::vector<float>& pose, std::vector<float>& points,
                                      int device = 0) {
        if (points.size() < 3 * static_cast<size_t>(std::max(g.n_points, 0)))
            throw std::invalid_argument("OptimizeEssentialGraph: points is short");
        pose.assign(12 * static_cast<size_t>(std::max(g.n_keyframes, 0)), 0.f);
        std::vector<double> g2o(8 * static_cast<size_t>(std::max(g.n_keyframes, 0)));
        std::vector<float> moved(std::max<size_t>(points.size(), 1));
        std::vector<uint8_t> accept(ORBBA_EG_MAX_TRIALS);
        int32_t it[2] = {0, 0};
        double chi2 = 0;
        g.points = points.data();
        orbba_essential_graph_result r = {g2o.data(), pose.data(), moved.data(), nullptr, it, &chi2, accept.data()};
        check(orbba_optimize_essential_graph(&g, &r, device), "orbba_optimize_essential_graph");
        std::copy(moved.begin(), moved.begin() + 3 * static_cast<size_t>(g.n_points), points.begin());
        return it[0];
    }
    // The edge list of :798-903 from slot tables (host only): edge_i, edge_j and edge_table in insertion order.
    static void EssentialGraphEdges(const orbba_eg_tables& t, std::vector<int32_t>& edge_i, std::vector<int32_t>& edge_j,
                                    std::vector<uint8_t>& edge_table, int32_t min_weight = 100) {
        int32_t n = 0;
        check(orbba_essential_graph_edges(&t, min_weight, 0, nullptr, nullptr, nullptr, &n), "orbba_essential_graph_edges");
        edge_i.assign(std::max(n, 1), 0);
        edge_j.assign(std::max(n, 1), 0);
        edge_table.assign(std::max(n, 1), 0);
        check(orbba_essential_graph_edges(&t, min_weight, n, edge_i.data(), edge_j.data(), edge_table.data(), &n),
              "orbba_essential_graph_edges");
        edge_i.resize(n);
        edge_j.resize(n);
        edge_table.resize(n);
    }
};

// Sim3Solver (include/Sim3Solver.h, src/Sim3Solver.cc:206-365): the 3-point RANSAC between SearchByBoW and
// SearchBySim3 in LoopClosing::FindLoopInCandidateKFs, a solver per (keyframe1, keyframe2) pair in SearchBySim3's
// slot layout (orb_sim3solver_batch: match12 is SearchByBoW's output, draws the rand() values of every hypothesis,
// r.iterations / r.max_inliers the solvers' state, read and written).
struct Sim3Solver {
    // bool iterate(maxk, sim3, isInlier) of every pair's solver on HBM arrays.  Enqueue only: r.found = the return
    // values, r.s12 the Sim3, r.inlier isInlier, r.match12 the input's matches thinned to the inliers.
    static void IterateBatch(const orb_sim3solver_batch& b, orb_sim3solver_result& r, void* stream = nullptr) {
        check(orb_sim3solver_iterate_device(&b, &r, stream), "orb_sim3solver_iterate_device");
    }
    // The same for one pair on host arrays.  iterations / max_inliers: the solver's state (0, 0 for a fresh one),
    // in / out; s12: 13 floats R, t, s; returns iterate()'s value and sets terminate.
    static bool Iterate(const orb_sim3solver_batch& b, int32_t& iterations, int32_t& max_inliers, float* s12,
                        std::vector<uint8_t>& inlier, std::vector<int32_t>& match12, bool& terminate, int device = 0) {
        if (b.n_pairs != 1) throw std::invalid_argument("Sim3Solver::Iterate: one pair per call (use the batch form)");
        inlier.assign(std::max(b.total_kp1, 1), 0);
        match12.assign(std::max(b.total_kp1, 1), -1);
        int32_t found = 0, n_inliers = 0, term = 0;
        orb_sim3solver_result r = {s12, inlier.data(), match12.data(), &found, &n_inliers, &iterations, &max_inliers, &term, nullptr};
        check(orb_sim3solver_iterate(&b, &r, device), "orb_sim3solver_iterate");
        inlier.resize(b.total_kp1);
        match12.resize(b.total_kp1);
        terminate = term != 0;
        return found == 1;
    }
};

// PnPsolver (include/PnPsolver.h, src/PnPsolver.cc): the EPnP RANSAC of Tracking::Relocalization between SearchByBoW
// and PoseOptimization, a solver per candidate keyframe in the slot layout of orb_pnpsolver_batch (mp_valid / mp_xw
// are SearchByBoW's matches, draws the rand() values of every hypothesis, r.iterations / r.best_inliers / r.best_mask /
// r.best_tcw the solvers' state, read and written).  The constructor takes the arrays, SetRansacParameters the
// reference's six parameters (Tracking.cc:352: 0.99, 10, 300, 4, 0.5f, 5.991f), iterate / find run the batch.
class PnPsolver {
public:
    PnPsolver(int32_t n_frames, int32_t total_kp, const int32_t* kp_begin, const float* kp_xy, const int32_t* kp_octave,
              const float* camera, const uint8_t* mp_valid, const float* mp_xw, int32_t n_levels, const float* level_sigma2,
              const int32_t* draws, int32_t n_draws, int32_t rand_max = 2147483647)
        : b_{n_frames, total_kp, kp_begin, kp_xy, kp_octave, camera, mp_valid, mp_xw, n_levels, level_sigma2, draws, n_draws,
             rand_max, 0.99, 8, 300, 4, 0.4f, 5.991f, 1} {}   // the defaults of PnPsolver.h's SetRansacParameters
    void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
                             float epsilon = 0.4f, float th2 = 5.991f) {
        b_.probability = probability; b_.min_inliers = minInliers; b_.max_iterations = maxIterations;
        b_.min_set = minSet; b_.epsilon = epsilon; b_.th2 = th2;
    }
    // cv::Mat iterate(nIterations, bNoMore, vbInliers, nInliers) of every candidate's solver on HBM arrays.  Enqueue
    // only: r.found = 1 (refined) / 2 (best at termination) / 0, r.tcw the pose, r.inlier vbInliers, r.terminate bNoMore.
    void IterateBatch(int nIterations, orb_pnpsolver_result& r, void* stream = nullptr) {
        b_.maxk = nIterations;
        check(orb_pnpsolver_iterate_device(&b_, &r, stream), "orb_pnpsolver_iterate_device");
    }
    // The same on host arrays, synchronous.
    void iterate(int nIterations, orb_pnpsolver_result& r, int device = 0) {
        b_.maxk = nIterations;
        check(orb_pnpsolver_iterate(&b_, &r, device), "orb_pnpsolver_iterate");
    }
    // cv::Mat find(vbInliers, nInliers): iterate(maxIterations) (:159-163; the reference passes the adjusted cap,
    // which the OR rule makes the same range for a fresh solver).
    void find(orb_pnpsolver_result& r, int device = 0) { iterate(b_.max_iterations, r, device); }
    const orb_pnpsolver_batch& batch() const { return b_; }

private:
    orb_pnpsolver_batch b_;
};

// Initializer (include/Initializer.h, src/Initializer.cc): the H / F RANSAC and reconstruction of
// Tracking::MonocularInitialization, an initializer per (reference frame, current frame) pair in the slot layout of
// orb_initializer_batch.  The constructor takes the reference frames (their keypointsUn and cameras), sigma and the
// iterations, as Initializer(ReferenceFrame, sigma, iterations) does; Initialize takes the current frames and
// vMatches12 (what SearchForInitializationBatch wrote) and the rand() table.
class Initializer {
public:
    Initializer(int32_t n_pairs, int32_t total_kp1, const int32_t* kp1_begin, const float* kp1_xy, const float* camera,
                float sigma = 1.0f, int iterations = 200)
        : b_{n_pairs, total_kp1, 0, kp1_begin, nullptr, kp1_xy, nullptr, nullptr, camera, nullptr, 2147483647, sigma, iterations,
             1.0f, 50, 0.40} {}
    // bool Initialize(CurrentFrame, vMatches12, R21, t21, vP3D, vbTriangulated) of every pair on HBM arrays.  Enqueue
    // only: r.found = the return values, r.r21t21 R21 and t21, r.p3d vP3D, r.triangulated vbTriangulated.
    void InitializeBatch(int32_t total_kp2, const int32_t* kp2_begin, const float* kp2_xy, const int32_t* matches12,
                         const int32_t* draws, orb_initializer_result& r, void* stream = nullptr, int32_t rand_max = 2147483647) {
        set(total_kp2, kp2_begin, kp2_xy, matches12, draws, rand_max);
        check(orb_initializer_initialize_device(&b_, &r, stream), "orb_initializer_initialize_device");
    }
    // The same on host arrays, synchronous.
    void Initialize(int32_t total_kp2, const int32_t* kp2_begin, const float* kp2_xy, const int32_t* matches12,
                    const int32_t* draws, orb_initializer_result& r, int device = 0, int32_t rand_max = 2147483647) {
        set(total_kp2, kp2_begin, kp2_xy, matches12, draws, rand_max);
        check(orb_initializer_initialize(&b_, &r, device), "orb_initializer_initialize");
    }
    const orb_initializer_batch& batch() const { return b_; }

private:
    void set(int32_t total_kp2, const int32_t* kp2_begin, const float* kp2_xy, const int32_t* matches12, const int32_t* draws,
             int32_t rand_max) {
        b_.total_kp2 = total_kp2; b_.kp2_begin = kp2_begin; b_.kp2_xy = kp2_xy; b_.matches12 = matches12;
        b_.draws = draws; b_.rand_max = rand_max;
    }
    orb_initializer_batch b_;
};

// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:380-578) on HBM-resident extractor slots.  The constructor takes
// the keyframes (orblm_batch without a plan) and what the search needs beyond them (descriptors, FeatureVectors,
// onlyStereo); Run takes the plan of n_rounds x n_pairs (keyframe 1, keyframe 2) entries, negative = none, as host
// arrays (checked: within a round no keyframe twice, and none as both where the sets share their flags) and as
// device arrays, and enqueues prepare and then per round the search and the triangulation.  The host allocates the
// MapPoints from out.new_idx1 / new_idx2 / n_created afterwards.
class CreateNewMapPoints {
public:
    CreateNewMapPoints(const orblm_batch& keyframes, const orbm_tri_batch& search) : b_(keyframes), s_(search) {}
    void Run(int32_t n_rounds, int32_t n_pairs, const int32_t* h_frame1, const int32_t* h_frame2, const int32_t* d_frame1,
             const int32_t* d_frame2, const orblm_pairs& pairs, const orblm_points& out, int32_t* d_match12,
             int32_t* d_nmatches, void* stream = nullptr) {
        CheckPlan(n_rounds, n_pairs, h_frame1, h_frame2, out.has_mappoint1 == out.has_mappoint2);
        b_.n_pairs = n_pairs; b_.frame1 = d_frame1; b_.frame2 = d_frame2;
        check(orblm_create_new_map_points_device(&b_, &s_, n_rounds, &pairs, &out, d_match12, d_nmatches, stream),
              "orblm_create_new_map_points_device");
    }
    // One round by hand, for a caller that polls CheckNewKeyFrames() between neighbours (:401): PreparePairs once, then
    // per round the search (SearchForTriangulationBatch on pairs.F12 / ep2 / frame1 / frame2) and Triangulate.
    void PreparePairs(int32_t n_pairs, const int32_t* d_frame1, const int32_t* d_frame2, const orblm_pairs& pairs,
                      void* stream = nullptr) {
        b_.n_pairs = n_pairs; b_.frame1 = d_frame1; b_.frame2 = d_frame2;
        check(orblm_prepare_pairs_device(&b_, &pairs, stream), "orblm_prepare_pairs_device");
    }
    void Triangulate(const orblm_pairs& pairs, const int32_t* d_match12, const orblm_points& out, void* stream = nullptr) {
        check(orblm_triangulate_device(&b_, &pairs, d_match12, &out, stream), "orblm_triangulate_device");
    }
    static void CheckPlan(int32_t n_rounds, int32_t n_pairs, const int32_t* frame1, const int32_t* frame2, bool same_set) {
        if (n_rounds < 0 || n_pairs < 0 || ((n_rounds && n_pairs) && (!frame1 || !frame2)))
            throw std::invalid_argument("CreateNewMapPoints: bad plan");
        for (int32_t r = 0; r < n_rounds; r++)
            for (int32_t i = 0; i < n_pairs; i++) {
                const int32_t a = frame1[r * n_pairs + i], c = frame2[r * n_pairs + i];
                if ((a < 0) != (c < 0)) throw std::invalid_argument("CreateNewMapPoints: an entry with one keyframe only");
                if (a < 0) continue;
                for (int32_t j = 0; j < n_pairs; j++) {
                    const int32_t a2 = frame1[r * n_pairs + j], c2 = frame2[r * n_pairs + j];
                    if (a2 < 0) continue;
                    if (j > i && (a2 == a || c2 == c)) throw std::invalid_argument("CreateNewMapPoints: a round names a keyframe twice");
                    if (same_set && a == c2)
                        throw std::invalid_argument("CreateNewMapPoints: a round names a keyframe as keyframe 1 and as keyframe 2");
                }
            }
    }
    const orblm_batch& batch() const { return b_; }

private:
    orblm_batch b_;
    orbm_tri_batch s_;
};

// void MapPoint::ComputeDistinctiveDescriptors() (src/MapPoint.cc:257-320), batched over map points on HBM
// arrays: point p holds the rows [begin[p], begin[p + 1]) of d_desc.  Enqueue only; best[p] = the winning
// point-relative row (-1: empty), d_out_desc[p] = that row (an empty point's row is not written, so
// d_out_desc may be the resident map point descriptor array); d_best_median and d_out_desc may be nullptr.
inline void ComputeDistinctiveDescriptorsBatch(const uint8_t* d_desc, const int32_t* d_begin, int32_t n_points,
                                               int32_t* d_best, int32_t* d_best_median, uint8_t* d_out_desc,
                                               void* stream = nullptr) {
    check(orbm_distinctive_descriptors_device(d_desc, d_begin, n_points, d_best, d_best_median, d_out_desc, stream),
          "orbm_distinctive_descriptors_device");
}
// One map point on host rows (descriptors: N x 32 bytes in the reference's iteration order); returns bestIdx
// (-1 when N == 0) and copies the winning row to `descriptor` (32 bytes, untouched when N == 0).
inline int ComputeDistinctiveDescriptors(const std::vector<uint8_t>& descriptors, uint8_t* descriptor, int device = 0) {
    if (descriptors.size() % 32) throw std::invalid_argument("ComputeDistinctiveDescriptors: rows of 32 bytes");
    const int32_t begin[2] = {0, static_cast<int32_t>(descriptors.size() / 32)};
    int32_t best = -1;
    check(orbm_distinctive_descriptors(descriptors.data(), begin, 1, &best, nullptr, descriptor, device),
          "orbm_distinctive_descriptors");
    return best;
}

// DBoW2 ORBVocabulary: loadFromTextFile + transform(features, BowVector&, FeatureVector&, levelsup)
// (TemplatedVocabulary.h:1130-1196, :1341-1431) with the reference's container types.
class ORBVocabulary {
public:
    using BowVector = std::map<uint32_t, double>;
    using FeatureVector = std::map<uint32_t, std::vector<unsigned int>>;

    explicit ORBVocabulary(int device = 0) : device_(device) {}
    ~ORBVocabulary() { orbv_destroy(h_); }
    ORBVocabulary(const ORBVocabulary&) = delete;
    ORBVocabulary& operator=(const ORBVocabulary&) = delete;

    bool loadFromTextFile(const std::string& filename) {
        orbv_destroy(h_);
        h_ = nullptr;
        return orbv_load_text(filename.c_str(), device_, &h_) == ORB_OK;
    }
    bool empty() const {
        int nw = 0;
        return !h_ || orbv_info(h_, nullptr, nullptr, nullptr, &nw, nullptr, nullptr) != ORB_OK || nw == 0;
    }
    // descriptors: n rows of 32 bytes (Converter::toDescriptorVector(descriptors))
    void transform(const uint8_t* descriptors, int n, BowVector& v, FeatureVector& fv, int levelsup) const {
        v.clear();
        fv.clear();
        if (!h_) return;
        const size_t cap = (size_t)std::max(n, 1);
        std::vector<uint32_t> bw(cap), fn(cap);
        std::vector<double> bv(cap);
        std::vector<int32_t> fo(cap + 1), fi(cap);
        int nw = 0, nn = 0;
        check(orbv_transform(h_, descriptors, n, levelsup, bw.data(), bv.data(), &nw, fn.data(), fo.data(), fi.data(),
                             &nn),
              "orbv_transform");
        for (int i = 0; i < nw; i++) v.emplace_hint(v.end(), bw[i], bv[i]);
        for (int t = 0; t < nn; t++)
            fv.emplace_hint(fv.end(), fn[t], std::vector<unsigned int>(fi.begin() + fo[t], fi.begin() + fo[t + 1]));
    }

private:
    int device_;
    orbv_vocabulary* h_ = nullptr;
};

// KeyFrameDatabase (include/KeyFrameDatabase.h, src/KeyFrameDatabase.cc:34-265) on slots: the host keeps the
// KeyFrame* <-> slot table, the covisibility table (GetBestCovisibilityKeyFrames(10) per slot, -1 padded), the
// connected sets and the consistency groups of LoopDetector::Detect (src/LoopClosing.cc:190-241); the BowVectors,
// the common-word counts, the scores and the candidate sets stay in HBM.  The device methods only enqueue; arrays
// are device memory in orbv_transform_batch_device's layout.
class KeyFrameDatabase {
public:
    KeyFrameDatabase(const orbv_vocabulary* voc, int max_keyframes, int word_cap, int device = 0) {
        check(orbdb_create(voc, max_keyframes, word_cap, device, &h_), "orbdb_create");
    }
    ~KeyFrameDatabase() { orbdb_destroy(h_); }
    KeyFrameDatabase(const KeyFrameDatabase&) = delete;
    KeyFrameDatabase& operator=(const KeyFrameDatabase&) = delete;

    // add(KeyFrame*) for n keyframes: slot d_slot[i] takes frame d_frame[i] (nullptr: i) of the transform output
    void add(int n, const int32_t* d_slot, const int32_t* d_frame, const uint32_t* d_bow_word, const double* d_bow_weight,
             const int32_t* d_n_words, int cap, int n_frames, void* stream = nullptr) {
        check(orbdb_add_device(h_, n, d_slot, d_frame, d_bow_word, d_bow_weight, d_n_words, cap, n_frames, stream),
              "orbdb_add_device");
    }
    void erase(int n, const int32_t* d_slot, void* stream = nullptr) {
        check(orbdb_erase_device(h_, n, d_slot, stream), "orbdb_erase_device");
    }
    void clear(void* stream = nullptr) { check(orbdb_clear(h_, stream), "orbdb_clear"); }
    // LoopDetector::Detect's minScore (LoopClosing.cc:170-178) into d_min_score, which DetectLoopCandidates reads
    void MinScore(const orbdb_query_batch& b, const int32_t* d_cov_off, const int32_t* d_cov_idx, float* d_min_score,
                  void* stream = nullptr) {
        check(orbdb_min_score_device(h_, &b, d_cov_off, d_cov_idx, d_min_score, stream), "orbdb_min_score_device");
    }
    void DetectLoopCandidates(const orbdb_query_batch& b, const orbdb_result& out, void* stream = nullptr) {
        check(orbdb_detect_loop_device(h_, &b, &out, stream), "orbdb_detect_loop_device");
    }
    void DetectRelocalizationCandidates(const orbdb_query_batch& b, const orbdb_result& out, void* stream = nullptr) {
        check(orbdb_detect_reloc_device(h_, &b, &out, stream), "orbdb_detect_reloc_device");
    }
    orbdb_database* handle() const { return h_; }

private:
    orbdb_database* h_ = nullptr;
};

// Tracking's local map (src/Tracking.cc: LocalMap::Update :59-179 and SearchLocalPoints up to the matcher call :607-642):
// the host keeps the KeyFrame* / MapPoint* <-> slot tables and owns the arrays of orbtl_map in HBM; TrackLocalMap enqueues
// the votes, the keyframe list, the local points and the frustum pass for a batch of frames, then SearchByProjection on the
// arrays it produced, on one stream with nothing copied back.  The keypoint arrays have stride frames.kp_cap.
class LocalMap {
public:
    explicit LocalMap(const orbtl_map& map) : map_(map) {}

    // LocalMap::Update + the frustum pass; out's arrays become search's map-point fields
    void Update(const orbtl_frames& frames, const orbtl_result& out, void* stream = nullptr) const {
        check(orbtl_track_local_map_device(&map_, &frames, &out, stream), "orbtl_track_local_map_device");
    }
    // TrackLocalMap up to PoseOptimization: Update, then ORBmatcher(nnratio).SearchByProjection(frame, mappoints, th).
    // `kp` carries kp_xy, kp_octave, kp_uright, kp_desc, bounds, n_levels, scale_factors, th, nnratio; the rest is filled here.
    void TrackLocalMap(const orbtl_frames& frames, const orbtl_result& out, orbm_proj_batch kp, int32_t* d_kp_match,
                       int32_t* d_n_matches, void* stream = nullptr) const {
        Update(frames, out, stream);
        kp.n_frames = frames.n_frames;
        kp.total_kp = frames.n_frames * frames.kp_cap;
        kp.total_mp = frames.n_frames * frames.mp_cap;
        kp.kp_begin = out.kp_begin;
        kp.kp_claimed = out.kp_claimed;
        kp.mp_begin = out.mp_begin;
        kp.mp_valid = out.mp_valid;
        kp.mp_proj = out.mp_proj;
        kp.mp_view_cos = out.mp_view_cos;
        kp.mp_level = out.mp_level;
        kp.mp_desc = out.mp_desc;
        kp.mp_has_obs = out.mp_has_obs;
        check(orbm_search_by_projection_device(&kp, d_kp_match, d_n_matches, stream), "orbm_search_by_projection_device");
    }
    const orbtl_map& map() const { return map_; }

private:
    orbtl_map map_;
};

// Tracking's per-frame state (src/Tracking.cc): frame.mappoints, frame.outlier and the pose of a batch of frames stay in the
// arrays of orbtf_frames in HBM between LocalMap::TrackLocalMap, the searches and PoseOptimization.  Every method only
// enqueues on `stream`; the host reads back the per-frame integers it decides on (n_inliers, counts, the created lists).
class TrackingFrames {
public:
    TrackingFrames(const orbtf_frames& frames, const orbtf_map& map) : frames_(frames), map_(map) {}

    // frame.mappoints[i] = source[kp_match[i]]: ORBTF_MERGE behind the local-map search, ORBTF_REPLACE behind the motion and
    // BoW searches
    void ApplyMatches(int32_t mode, const int32_t* d_kp_match, const int32_t* d_src, int32_t n_rows, int32_t src_cap,
                      const int32_t* d_src_row = nullptr, void* stream = nullptr) const {
        check(orbtf_apply_matches_device(&frames_, mode, d_kp_match, d_src, n_rows, src_cap, d_src_row, map_.n_mappoints, stream),
              "orbtf_apply_matches_device");
    }
    // Optimizer::PoseOptimization(&frame) on the resident state: the gather, the optimiser, the result taken back
    // (ORBTF_DISCARD: DiscardOutliers; ORBTF_LOCAL_MAP: TrackLocalMap's statistics)
    void PoseOptimization(const float* d_inv_sigma2, int32_t n_levels, const orbtf_edges& edges, orbba_pose_result result,
                          int32_t mode, bool localization, bool stereo, int32_t* d_n_inliers, int32_t* d_discarded = nullptr,
                          int32_t* d_n_discarded = nullptr, void* stream = nullptr) const {
        check(orbtf_pose_edges_device(&frames_, &map_, d_inv_sigma2, n_levels, &edges, stream), "orbtf_pose_edges_device");
        const orbba_pose_batch batch{frames_.n_frames, edges.edge_begin, edges.pose_R, edges.pose_t, edges.cam,
                                     edges.xw,         edges.obs,        edges.inv_sigma2};
        check(orbba_pose_optimization_device(&batch, &result, stream), "orbba_pose_optimization_device");
        check(orbtf_finish_pose_device(&frames_, &map_, mode, &edges, &result, localization, stereo, d_n_inliers, d_discarded,
                                       d_n_discarded, stream),
              "orbtf_finish_pose_device");
    }
    // TrackWithMotionModel's setup; out's arrays become the map-point fields of an orbm_motion_batch
    void MotionProject(const orbtf_frames& last, const float* d_velocity, const float* d_baseline, bool monocular,
                       const orbtf_motion& out, void* stream = nullptr) const {
        check(orbtf_motion_project_device(&frames_, &last, &map_, d_velocity, d_baseline, monocular, &out, stream),
              "orbtf_motion_project_device");
    }
    // the end of Tracking::Update: nobservations_, the clean of visual-odometry matches, NeedNewKeyFrame's three counts
    void EndFrame(float thDepth, const int32_t* d_reference_kf, const int32_t* d_min_obs, int32_t* d_n_observations,
                  int32_t* d_counts, void* stream = nullptr) const {
        check(orbtf_end_frame_device(&frames_, &map_, thDepth, d_reference_kf, d_min_obs, d_n_observations, d_counts, stream),
              "orbtf_end_frame_device");
    }
    void DropOutliers(void* stream = nullptr) const { check(orbtf_drop_outliers_device(&frames_, stream), "orbtf_drop_outliers_device"); }
    // CreateMapPoints (ORBTF_KEYFRAME), CreateMapPointsVO (ORBTF_VO), StereoInitialization (ORBTF_INIT)
    void StereoPoints(int32_t mode, float thDepth, const orbtf_created& out, void* stream = nullptr) const {
        check(orbtf_stereo_points_device(&frames_, &map_, mode, thDepth, &out, stream), "orbtf_stereo_points_device");
    }
    const orbtf_frames& frames() const { return frames_; }

private:
    orbtf_frames frames_;
    orbtf_map map_;
};

// What System does between Extract and the Frame constructor (src/System.cc:153-219, :455, :512-520, :570) on the
// extractor's HBM-resident output: undistortion, RGB-D depth, image bounds and the split into the frame tables.  The
// builder holds the tables it writes as an orbtf_frames, so TrackingFrames(builder.frames(), map) is the next step with
// nothing copied; pose and kp_desc (the extractor's d_desc) are the caller's.  Build only enqueues on `stream`.
class FrameBuilder {
public:
    // tables: frame_n, frame_mappoint, frame_outlier, bounds, kp_xy, kp_octave, kp_uright, kp_depth and kp_angle are written
    // (a NULL one is skipped; ORBFR_STEREO leaves kp_uright / kp_depth to orbx_stereo_matches_batch_device), camera is read.
    // d_dist [F][5] = k1, k2, p1, p2, k3.  d_kp_un / d_kp_begin: keypointsUn records and f * kp_cap, or NULL.
    FrameBuilder(const orbtf_frames& tables, const float* d_dist, int rows, int cols, orbx_keypoint* d_kp_un = nullptr,
                 int32_t* d_kp_begin = nullptr)
        : frames_(tables), dist_(d_dist), rows_(rows), cols_(cols), kp_un_(d_kp_un), kp_begin_(d_kp_begin) {}

    // TrackMonocular (:570) and TrackStereo (:455): d_kps / d_counts are orbx_extract_batch_device's with cap == kp_cap
    void Build(int32_t mode, const orbx_keypoint* d_kps, const int32_t* d_counts, void* stream = nullptr) const {
        Build(mode, d_kps, d_counts, nullptr, 0, 0, 0, 0.f, stream);
    }
    // TrackRGBD (:512-520): depth images of depth_type elements, depth_factor = depthFactor_
    void Build(int32_t mode, const orbx_keypoint* d_kps, const int32_t* d_counts, const void* d_depth, int32_t depth_type,
               size_t depth_frame_stride, size_t depth_step, float depth_factor, void* stream = nullptr) const {
        const orbfr_input in{frames_.n_frames, frames_.kp_cap, rows_,   cols_,   mode,
                             depth_type,       d_kps,          d_counts, frames_.camera, dist_,
                             d_depth,          depth_frame_stride, depth_step, depth_factor};
        const orbfr_frames out{const_cast<int32_t*>(frames_.frame_n), const_cast<float*>(frames_.kp_xy),
                               const_cast<int32_t*>(frames_.kp_octave), const_cast<float*>(frames_.kp_angle), kp_un_,
                               const_cast<float*>(frames_.kp_uright), const_cast<float*>(frames_.kp_depth),
                               const_cast<float*>(frames_.bounds), frames_.frame_mappoint, frames_.frame_outlier, kp_begin_};
        check(orbfr_build_frames_device(&in, &out, stream), "orbfr_build_frames_device");
    }
    // ComputeImageBounds on the CPU, for the reference's once-per-run shape (:464-465): minx, maxx, miny, maxy
    static void ImageBounds(int rows, int cols, const float* camera, const float* dist, float bounds[4]) {
        check(orbfr_image_bounds(rows, cols, camera, dist, bounds), "orbfr_image_bounds");
    }
    const orbtf_frames& frames() const { return frames_; }

private:
    orbtf_frames frames_;
    const float* dist_;
    int rows_, cols_;
    orbx_keypoint* kp_un_;
    int32_t* kp_begin_;
};

// Where the map grows (src/KeyFrame.cc:51-64, src/MapPoint.cc:44-56 with src/Tracking.cc:724-736, :981-997, :1104-1126 and
// src/LocalMapping.cc:562-575): the host owns the slot tables in HBM and the KeyFrame* <-> slot table; it enqueues the KeyFrame
// constructor for the frames it chose slots for, and the MapPoint constructor with AddObservation / AddMapPoint /
// Map::AddMapPoint on the lists orbtf_stereo_points_device and orblm_create_new_map_points_device left in HBM, with the slots
// allocated on the device.  Both only enqueue on `stream`; nothing is copied back.
class MapBuilder {
public:
    MapBuilder(const orbmk_keyframes& keyframes, const orbmk_map& map) : keyframes_(keyframes), map_(map) {}

    // d_item_*: [n_items] frame of `frames`, keyframe slot, KeyFrame::id, camera.baseline
    void InsertKeyFrames(const orbmk_frames& frames, int32_t n_items, const int32_t* d_item_frame, const int32_t* d_item_kf,
                         const int32_t* d_item_id, const float* d_item_baseline, void* stream = nullptr) const {
        check(orbmk_insert_keyframes_device(&frames, &keyframes_, n_items, d_item_frame, d_item_kf, d_item_id, d_item_baseline, stream),
              "orbmk_insert_keyframes_device");
    }
    // out.status[0] (HBM) is ORBMK_OK or ORBMK_OVERFLOW: read it when convenient
    void CreatePoints(const orbmk_lists& lists, const orbmk_created& out, void* stream = nullptr) const {
        check(orbmk_create_points_device(&map_, &lists, &out, stream), "orbmk_create_points_device");
    }
    // CreateMapPoints / StereoInitialization (src/Tracking.cc:724-736, :981-997): the lists orbtf_stereo_points_device wrote
    // for `frames`, one observation in the keyframe d_item_kf[f]; frame_mappoint gets the new slots
    void CreatePoints(const orbtf_frames& frames, const orbtf_created& created, const int32_t* d_item_kf,
                      const int32_t* d_item_frame, const orbmk_created& out, void* stream = nullptr) const {
        orbmk_lists l{};
        l.n_items = frames.n_frames; l.list_cap = frames.kp_cap;
        l.kf1 = d_item_kf; l.n_list = created.n_created; l.idx1 = created.created_kp; l.xw = created.created_xw;
        l.n_frames = frames.n_frames; l.kp_cap = frames.kp_cap; l.item_frame = d_item_frame; l.frame_mappoint = frames.frame_mappoint;
        CreatePoints(l, out, stream);
    }
    // CreateNewMapPoints (src/LocalMapping.cc:562-575): the lists orblm_create_new_map_points_device wrote for n_plan plan
    // entries of keyframes d_kf1 / d_kf2 (slots), values by keypoint; out.recent is recentAddedMapPoints_
    void CreatePoints(const orblm_points& points, int32_t n_plan, int32_t cap1, const int32_t* d_kf1, const int32_t* d_kf2,
                      const orbmk_created& out, void* stream = nullptr) const {
        orbmk_lists l{};
        l.n_items = n_plan; l.list_cap = cap1; l.values_by_keypoint = 1;
        l.kf1 = d_kf1; l.kf2 = d_kf2; l.n_list = points.n_created; l.idx1 = points.new_idx1; l.idx2 = points.new_idx2;
        l.xw = points.xw; l.normal = points.normal; l.max_distance = points.max_distance; l.min_distance = points.min_distance;
        CreatePoints(l, out, stream);
    }
    const orbmk_keyframes& keyframes() const { return keyframes_; }
    const orbmk_map& map() const { return map_; }

private:
    orbmk_keyframes keyframes_;
    orbmk_map map_;
};

// Map maintenance (src/MapPoint.cc:341-380, src/KeyFrame.cc:94-119, 235-309): the host owns the arrays of orbmm_graph in
// HBM; after the map moved on the device (orbba_gba_update_map_device, the essential graph, new points, Fuse) it enqueues
// UpdateNormalAndDepth for the points and UpdateConnections for the keyframes on the stream the readers follow on
// (LocalMap::TrackLocalMap, KeyFrameDatabase::DetectLoopCandidates), with nothing copied back.
class MapMaintenance {
public:
    explicit MapMaintenance(const orbmm_graph& graph) : graph_(graph) {}

    // MapPoint::UpdateNormalAndDepth for points.point (NULL: every point): mp_normal and mp_max_min in place
    static void UpdateNormalAndDepth(const orbmm_points& points, void* stream = nullptr) {
        check(orbmm_update_normal_depth_device(&points, stream), "orbmm_update_normal_depth_device");
    }
    // KeyFrame::UpdateConnections of the keyframe slots d_item[0 .. n_items), in order; graph.status tells overflow
    void UpdateConnections(const int32_t* d_item, int32_t n_items, void* stream = nullptr) const {
        check(orbmm_update_connections_device(&graph_, n_items, d_item, stream), "orbmm_update_connections_device");
    }
    // GetChildren() of every keyframe as the CSR orbtl_map and orbba_gba_map take
    void UpdateChildren(int32_t* d_child_off, int32_t* d_child_idx, void* stream = nullptr) const {
        check(orbmm_children_device(graph_.n_keyframes, graph_.kf_parent, d_child_off, d_child_idx, stream), "orbmm_children_device");
    }
    // the rows as orbba_eg_tables' covis_* and orbdb_query_batch's conn_*
    void PackCovisibility(const orbmm_csr& out, void* stream = nullptr) const {
        check(orbmm_covis_csr_device(&graph_, &out, stream), "orbmm_covis_csr_device");
    }
    const orbmm_graph& graph() const { return graph_; }

private:
    orbmm_graph graph_;
};

// LocalMapping's culls (src/LocalMapping.cc:335-369, 641-701): the host owns the arrays of orbmm_cull in HBM and enqueues
// MapPointCulling before and KeyFrameCulling after the local bundle adjustment, on the stream the map-maintenance calls
// and the readers follow on; the map never comes back to the host.  An erased observation is a -1 in mp_obs_kf until
// CompactObservations writes the CSR without them.
class Culling {
public:
    explicit Culling(const orbmm_cull& tables) : tables_(tables) {}

    // MapPointCulling: d_recent (recentAddedMapPoints_ as point slots) rewritten in place, *d_n_recent_out what is left
    void MapPointCulling(int32_t* d_recent, int32_t n_recent, int32_t cur_kf_id, bool monocular, int32_t* d_n_recent_out,
                         void* stream = nullptr) const {
        check(orbmm_cull_map_points_device(&tables_, n_recent, d_recent, cur_kf_id, monocular ? 1 : 0, d_n_recent_out, stream),
              "orbmm_cull_map_points_device");
    }
    // KeyFrameCulling(cur): d_culled (conn_cap entries, -1 padded) is what orbdb_erase_device takes
    void KeyFrameCulling(int32_t cur, bool monocular, float th_depth, int32_t* d_culled, int32_t* d_n_culled, int32_t* d_status,
                         void* stream = nullptr) const {
        check(orbmm_cull_keyframes_device(&tables_, cur, monocular ? 1 : 0, th_depth, d_culled, d_n_culled, d_status, stream),
              "orbmm_cull_keyframes_device");
    }
    // the observation CSR without erased entries into arrays of the same capacity; the caller swaps them
    void CompactObservations(int32_t* d_out_off, int32_t* d_out_kf, int32_t* d_out_idx, void* stream = nullptr) const {
        check(orbmm_compact_observations_device(tables_.n_mappoints, tables_.n_obs, tables_.mp_obs_off, tables_.mp_obs_kf,
                                                tables_.mp_obs_idx, d_out_off, d_out_kf, d_out_idx, stream),
              "orbmm_compact_observations_device");
    }
    // GetChildren() of every keyframe with the culled left out, as the CSR orbtl_map and orbba_gba_map take
    void UpdateLiveChildren(int32_t* d_child_off, int32_t* d_child_idx, void* stream = nullptr) const {
        check(orbmm_children_live_device(tables_.n_keyframes, tables_.kf_parent, tables_.kf_bad, d_child_off, d_child_idx, stream),
              "orbmm_children_live_device");
    }
    const orbmm_cull& tables() const { return tables_; }

private:
    orbmm_cull tables_;
};

// The insert half of the observation graph (src/MapPoint.cc:109-122, 191-230): the host owns the arrays of orbmm_observe
// in HBM and enqueues ProcessNewKeyFrame's loop, the apply loop after each Fuse search and CorrectLoop's matched points on
// the stream the searches and the map-maintenance calls run on; best_idx never comes back to the host.  A row needs free
// entries (-1) for an insert: on ORBMM_OBS_OVERFLOW in *d_status, Grow and call FuseApply again with the same arrays.
class Observations {
public:
    explicit Observations(const orbmm_observe& tables) : tables_(tables) {}

    // LocalMapping.cc:309-326 for keyframe slot cur: d_added / d_recent hold kf_cap entries (-1 padded), d_counts their two
    // lengths, d_status kf_cap entries (ORBMM_OBS_OVERFLOW where a point's row was full)
    void AddKeyFrameObservations(int32_t cur, int32_t* d_added, int32_t* d_recent, int32_t* d_counts, int32_t* d_status,
                                 void* stream = nullptr) const {
        check(orbmm_add_keyframe_observations_device(&tables_, cur, d_added, d_recent, d_counts, d_status, stream),
              "orbmm_add_keyframe_observations_device");
    }
    // the apply loop of apply.mode over the list orbm_fuse_device left in HBM
    void FuseApply(const orbmm_apply& apply, void* stream = nullptr) const {
        check(orbmm_fuse_apply_device(&tables_, &apply, stream), "orbmm_fuse_apply_device");
    }
    // the observation CSR with `slack` free entries per row (d_extra[p] where given) into arrays of n_obs_out entries; the
    // caller swaps them and updates tables()
    void Grow(int32_t slack, const int32_t* d_extra, int32_t n_obs_out, int32_t* d_out_off, int32_t* d_out_kf, int32_t* d_out_idx,
              int32_t* d_status, void* stream = nullptr) const {
        check(orbmm_grow_observations_device(tables_.n_mappoints, tables_.n_obs, tables_.mp_obs_off, tables_.mp_obs_kf,
                                             tables_.mp_obs_idx, slack, d_extra, n_obs_out, d_out_off, d_out_kf, d_out_idx, d_status,
                                             stream),
              "orbmm_grow_observations_device");
    }
    orbmm_observe& tables() { return tables_; }
    const orbmm_observe& tables() const { return tables_; }

private:
    orbmm_observe tables_;
};

// LoopCorrector::Correct (src/LoopClosing.cc:546-676): the host owns the arrays of orblc_map in HBM and enqueues the steps
// on one stream; nothing is copied back.  The fuse steps between Propagate and LoopConnections are Observations' and
// ORBmatcher's.
class LoopCorrection {
public:
    explicit LoopCorrection(const orblc_map& map) : map_(map) {}
    // connectedKFs (:550-552): d_connected holds conn_cap + 1 entries, d_n_connected one
    void Connected(int32_t cur, int32_t* d_connected, int32_t* d_n_connected, void* stream = nullptr) const {
        check(orblc_connected_device(&map_, cur, d_connected, d_n_connected, stream), "orblc_connected_device");
    }
    // :554-613: the propagation, then UpdateConnections of the connected keyframes in ascending slot order (d_items,
    // max_connected entries, is filled by the first call and read by the second)
    void Propagate(int32_t cur, const float* d_scw, const int32_t* d_connected, int32_t max_connected, float* d_vertex_sim3,
                   float* d_edge_sim3, int32_t* d_point_ref, int32_t* d_items, void* stream = nullptr) const {
        check(orblc_propagate_device(&map_, cur, d_scw, d_connected, max_connected, d_vertex_sim3, d_edge_sim3, d_point_ref, d_items,
                                     stream), "orblc_propagate_device");
        const orbmm_graph g = orblc_graph(&map_);
        check(orbmm_update_connections_device(&g, max_connected, d_items, stream), "orbmm_update_connections_device");
    }
    // :661-676: the LoopConnections sets in orbba_eg_tables' form
    void LoopConnections(const int32_t* d_connected, int32_t max_connected, int32_t* d_conn_kf, int32_t* d_conn_begin,
                         int32_t* d_conn_slot, int32_t* d_n_connections, void* stream = nullptr) const {
        check(orblc_loop_connections_device(&map_, d_connected, max_connected, d_conn_kf, d_conn_begin, d_conn_slot, d_n_connections,
                                            stream), "orblc_loop_connections_device");
    }
    // Optimizer.cc:798-903 on the device; the lists past the count are (-1, -1, 0)
    static void EssentialGraphEdges(const orbba_eg_tables& tables, int32_t n_loop_slots, int32_t n_covis_slots, int32_t n_conn_slots,
                                    int32_t min_weight, int32_t capacity, int32_t* d_edge_i, int32_t* d_edge_j,
                                    uint8_t* d_edge_table, int32_t* d_n_edges, void* stream = nullptr) {
        check(orbba_essential_graph_edges_device(&tables, n_loop_slots, n_covis_slots, n_conn_slots, min_weight, capacity, d_edge_i,
                                                 d_edge_j, d_edge_table, d_n_edges, stream), "orbba_essential_graph_edges_device");
    }
    const orblc_map& map() const { return map_; }

private:
    orblc_map map_;
};

}  // namespace ORB_SLAM2_AMD

#endif  // ORBSLAM2_AMD_HPP
