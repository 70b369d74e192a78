// db_score.h — the per-pair and per-group arithmetic of KeyFrameDatabase's two candidate queries, for host and
// device (orbdb.hip, tests/native/keyframe_db_check.cpp).
//
// Reference: src/KeyFrameDatabase.cc:68-265 (DetectLoopCandidates, DetectRelocalizationCandidates),
// L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68), the minScore loop of LoopDetector::Detect
// (src/LoopClosing.cc:170-178).  Every float and double operation below is done in the reference's type and order;
// the library is built with -ffp-contract=off, so none of them fuses.
//
// A BowVector is two ascending arrays (word ids, fp64 weights), as orbv_transform* emits it.  The device sums the
// same db_term values in the same ascending word order as db_score does (orbdb.hip: db_wave_score); the lookup, the
// term, the final scaling, minw, the group walk and the retain rule are this code on both sides.
#pragma once

#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define DB_HD __host__ __device__ __forceinline__
#else
#define DB_HD inline
#endif

namespace orbamd {

constexpr int DB_COVIS = 10;   // GetBestCovisibilityKeyFrames(10)

// First position whose word id is >= x (BowVector::lower_bound on the ascending array).
DB_HD int db_lower_bound(const uint32_t* w, int n, uint32_t x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (w[mid] < x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// One common word's contribution (ScoringObject.cpp:41): vi from v1 (the query), wi from v2 (the keyframe).
DB_HD double db_term(double vi, double wi) { return fabs(vi - wi) - fabs(vi) - fabs(wi); }

// score = -score / 2.0 (:65); both queries and Detect cast the result to float.
DB_HD double db_finish(double s) { return -s / 2.0; }

// L1Scoring::score: the merge of two ascending vectors, the terms added to one double in ascending word order.
// *common (may be null) receives the number of shared word ids: loopWords / relocWords after the inverted-file walk.
DB_HD double db_score(const uint32_t* w1, const double* v1, int n1, const uint32_t* w2, const double* v2, int n2,
                      int* common) {
    double s = 0;
    int i = 0, j = 0, c = 0;
    while (i < n1 && j < n2) {
        if (w1[i] == w2[j]) {
            s += db_term(v1[i], v2[j]);
            ++i; ++j; ++c;
        } else if (w1[i] < w2[j]) {
            i += db_lower_bound(w1 + i, n1 - i, w2[j]);   // v1_it = v1.lower_bound(v2_it->first)
        } else {
            j += db_lower_bound(w2 + j, n2 - j, w1[i]);
        }
    }
    if (common) *common = c;
    return db_finish(s);
}

// const int minCommonWords = static_cast<int>(0.8f * maxCommonWords)  (KeyFrameDatabase.cc:106, :204)
DB_HD int db_minw(int maxw) { return (int)(0.8f * (float)maxw); }

// std::min / std::max as the reference applies them: the running value changes only on a strict comparison.
DB_HD float db_min(float run, float x) { return x < run ? x : run; }
DB_HD float db_max(float run, float x) { return run < x ? x : run; }

struct DbGroup {
    float acc;
    int bestk;
};

// One covisibility group (:131-154, :229-252): keyframe k with this query's score, its ten best covisible
// keyframes in table order.  A neighbour counts where member[nb] != 0 and then adds val[nb]:
//   relocalisation  member = shares a word with the query (relocQuery == frame->id), val = relocScore
//   loop            member = scored by this query (loopQuery == id && loopWords > minCommonWords), val = loopScore
// Entries outside [0, K) (-1 pads the table) are skipped.
DB_HD DbGroup db_group_walk(int k, float score_k, const int32_t* covis_row, int K, const uint8_t* member,
                            const float* val) {
    float best = score_k, acc = score_k;
    int bestk = k;
    for (int t = 0; t < DB_COVIS; t++) {
        const int nb = covis_row[t];
        if (nb < 0 || nb >= K || !member[nb]) continue;
        const float s = val[nb];
        acc += s;
        if (s > best) {
            bestk = nb;
            best = s;
        }
    }
    return DbGroup{acc, bestk};
}

// if (v.first > minScoreToRetain), minScoreToRetain = 0.75f * bestAccScore  (:157-167, :255-262)
DB_HD bool db_retained(float acc, float best_acc) { return acc > 0.75f * best_acc; }

}  // namespace orbamd
