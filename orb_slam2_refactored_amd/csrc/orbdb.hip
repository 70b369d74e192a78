// orbdb.hip — KeyFrameDatabase on gfx950: add / erase / clear, DetectLoopCandidates, DetectRelocalizationCandidates
// and LoopDetector::Detect's minScore, batched over query frames (include/orbslam2_amd.h, "KeyFrameDatabase").
//
// Reference: src/KeyFrameDatabase.cc:34-265, src/LoopClosing.cc:170-178, L1Scoring::score
// (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).  The arithmetic is csrc/db_score.h's.
//
// No inverted file: a slot is a row of (word, weight) pairs, add is a copy and erase a flag store.  Passes of one
// query call, stream-ordered, nothing read back:
//   db_words_kernel    one wavefront per (q, k): the slot's words looked up in the query's ascending list (in LDS)
//                      by binary search; integer work only
//   db_select_kernel   one workgroup per q: S (live, words > 0, not connected), maxw, minw, the scored flags
//   db_score_kernel    one wavefront per scored (q, k): 64 slot words per step looked up in the query, the common
//                      words' terms added to one double in ascending word order (ballot, then lane by lane)
//   db_reloc_scan_kernel  relocalisation: per slot the last-writer scan of reloc_score over q
//   db_group_kernel    one workgroup per q: one lane per group (ten neighbours in order, float adds), bestAcc by
//                      max, the retained groups' bestk marked and the marks compacted ascending
#include <algorithm>
#include <vector>

#include "common.h"
#include "db_score.h"

struct orbdb_database {
    int device = 0;
    int K = 0, W = 0;
    orbamd::DevBuf buf;   // live | nw | reloc | word | weight
    uint8_t* live = nullptr;
    int32_t* nw = nullptr;
    float* reloc = nullptr;
    uint32_t* word = nullptr;
    double* weight = nullptr;
    orbamd::DevBuf ws, io;   // per-call [Q][K] arrays; host-entry staging
};

namespace orbamd {

constexpr int DB_MAXQ = ORBV_MAX_FEATURES;   // words of a query BowVector (its list sits in LDS)
constexpr int DB_WAVES = 4;                  // wavefronts per workgroup (256 threads)
constexpr int DB_SLOTS_PER_WAVE = 4;         // db_words_kernel: slots per wavefront, one query list load for 16

struct DbQuery {
    const uint32_t* word;
    const double* weight;
    const int32_t* n_words;
    const int32_t* frame;
    int cap, n_frames;
};

struct DbStore {   // the slots, writable (add)
    uint8_t* live;
    int32_t* nw;
    float* reloc;
    uint32_t* word;
    double* weight;
    int K, W;
};

struct DbSlots {
    const uint8_t* live;
    const int32_t* nw;
    const uint32_t* word;
    const double* weight;
    int K, W;
};

// Query q's BowVector; an out-of-range frame or count is an empty / clamped one (device memory is not trusted).
__device__ __forceinline__ int db_query(const DbQuery& b, int q, const uint32_t*& w, const double*& v) {
    const int f = b.frame ? b.frame[q] : q;
    if (f < 0 || f >= b.n_frames) { w = nullptr; v = nullptr; return 0; }
    w = b.word + (size_t)f * b.cap;
    v = b.weight + (size_t)f * b.cap;
    return min(max(b.n_words[f], 0), b.cap);
}

__device__ __forceinline__ int db_slot_words(const DbSlots& s, int k) {
    return s.live[k] ? min(max(s.nw[k], 0), s.W) : 0;
}

__device__ __forceinline__ double db_readlane(double x, int lane) {   // lane is wave-uniform
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(x), lane);
    return __hiloint2double(hi, lo);
}

// L1Scoring::score's sum on one wavefront: the slot's words 64 at a time, each looked up in the query; the common
// words' terms are then added one by one in lane order = ascending word order, every lane keeping the same sum.
__device__ __forceinline__ double db_wave_score(const uint32_t* qw, const double* qv, int nq, const uint32_t* kw,
                                                const double* kv, int nk, int lane) {
    double s = 0;
    for (int base = 0; base < nk; base += 64) {   // nk is wave-uniform
        const int i = base + lane;
        bool hit = false;
        double term = 0;
        if (i < nk) {
            const uint32_t x = kw[i];
            const int p = db_lower_bound(qw, nq, x);
            if (p < nq && qw[p] == x) {
                hit = true;
                term = db_term(qv[p], kv[i]);
            }
        }
        unsigned long long m = __ballot(hit);
        while (m) {
            const int l = __builtin_ctzll(m);
            m &= m - 1;
            s += db_readlane(term, l);
        }
    }
    return s;
}

__global__ __launch_bounds__(256) void db_words_kernel(DbQuery b, DbSlots s, int blocks_per_q, int32_t* words) {
    __shared__ uint32_t s_q[DB_MAXQ];
    const int q = blockIdx.x / blocks_per_q, blk = blockIdx.x % blocks_per_q;
    const uint32_t* qw;
    const double* qv;
    const int nq = db_query(b, q, qw, qv);
    for (int i = threadIdx.x; i < nq; i += 256) s_q[i] = qw[i];
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int t = 0; t < DB_SLOTS_PER_WAVE; t++) {
        const int k = (blk * DB_WAVES + wave) * DB_SLOTS_PER_WAVE + t;
        if (k >= s.K) break;   // wave-uniform
        const int n = nq ? db_slot_words(s, k) : 0;
        const uint32_t* kw = s.word + (size_t)k * s.W;
        int c = 0;
        for (int i = lane; i < n; i += 64) {
            const uint32_t x = kw[i];
            const int p = db_lower_bound(s_q, nq, x);
            c += (p < nq && s_q[p] == x) ? 1 : 0;
        }
#pragma unroll
        for (int m = 32; m > 0; m >>= 1) c += __shfl_xor(c, m, 64);
        if (lane == 0) words[(size_t)q * s.K + k] = c;
    }
}

struct DbWork {   // per call, [Q][K] each
    int32_t* words;
    uint8_t* scored;
    float* score;
    float* acc;
    int32_t* bestk;
    uint8_t* in_s;
    uint8_t* mark;
    float* eff;   // relocalisation: reloc_score as query q's groups read it
};

__global__ __launch_bounds__(256) void db_select_kernel(DbSlots s, DbWork w, const int32_t* conn_off,
                                                        const int32_t* conn_idx) {
    __shared__ int s_max[256];
    const int q = blockIdx.x, K = s.K;
    const size_t row = (size_t)q * K;
    for (int k = threadIdx.x; k < K; k += 256) {
        w.in_s[row + k] = (s.live[k] && w.words[row + k] > 0) ? 1 : 0;
        w.score[row + k] = 0.f;
        w.acc[row + k] = 0.f;
        w.bestk[row + k] = -1;
        w.mark[row + k] = 0;
    }
    __syncthreads();
    if (conn_off) {   // if (!connectedKFs.count(sharingKF)) (:85)
        const int e0 = conn_off[q], e1 = conn_off[q + 1];
        for (int e = e0 + (int)threadIdx.x; e0 >= 0 && e < e1; e += 256) {
            const int k = conn_idx[e];
            if (k >= 0 && k < K) w.in_s[row + k] = 0;
        }
        __syncthreads();
    }
    int m = 0;
    for (int k = threadIdx.x; k < K; k += 256)
        if (w.in_s[row + k]) m = max(m, w.words[row + k]);
    s_max[threadIdx.x] = m;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s_max[threadIdx.x] = max(s_max[threadIdx.x], s_max[threadIdx.x + h]);
        __syncthreads();
    }
    const int minw = db_minw(s_max[0]);
    for (int k = threadIdx.x; k < K; k += 256)
        w.scored[row + k] = (w.in_s[row + k] && w.words[row + k] > minw) ? 1 : 0;
}

__global__ __launch_bounds__(256) void db_score_kernel(DbQuery b, DbSlots s, int blocks_per_q, const uint8_t* scored,
                                                       float* score) {
    const int q = blockIdx.x / blocks_per_q, blk = blockIdx.x % blocks_per_q;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int k = blk * DB_WAVES + wave;
    if (k >= s.K || !scored[(size_t)q * s.K + k]) return;   // wave-uniform
    const uint32_t* qw;
    const double* qv;
    const int nq = db_query(b, q, qw, qv);
    const double sum = db_wave_score(qw, qv, nq, s.word + (size_t)k * s.W, s.weight + (size_t)k * s.W,
                                     db_slot_words(s, k), lane);
    if (lane == 0) score[(size_t)q * s.K + k] = (float)db_finish(sum);
}

// Relocalisation: sharingKF->relocScore = score (:217) by query q, read by the groups of queries q, q+1, ...
__global__ __launch_bounds__(256) void db_reloc_scan_kernel(int Q, int K, const uint8_t* scored, const float* score,
                                                            float* eff, float* reloc) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    float e = reloc[k];
    for (int q = 0; q < Q; q++) {
        const size_t i = (size_t)q * K + k;
        if (scored[i]) e = score[i];
        eff[i] = e;
    }
    reloc[k] = e;
}

__global__ __launch_bounds__(256) void db_group_kernel(int K, DbWork w, const int32_t* covis, const float* min_score,
                                                       int32_t* cand, int32_t* n_cand) {
    __shared__ float s_best[256];
    __shared__ int s_part[257];
    const int q = blockIdx.x;
    const size_t row = (size_t)q * K;
    const bool loop = min_score != nullptr;
    const float floor_score = loop ? min_score[q] : 0.f;
    // loop: neighborKF->loopQuery == id && loopWords > minCommonWords (:141); reloc: relocQuery == frame->id (:239)
    const uint8_t* member = (loop ? w.scored : w.in_s) + row;
    const float* val = (loop ? w.score : w.eff) + row;
    float best = floor_score;   // float bestAccScore = minScore (:128) / = 0 (:226)
    for (int k = threadIdx.x; k < K; k += 256) {
        if (!w.scored[row + k] || (loop && !(w.score[row + k] >= floor_score))) continue;
        const DbGroup g = db_group_walk(k, w.score[row + k], covis + (size_t)k * DB_COVIS, K, member, val);
        w.acc[row + k] = g.acc;
        w.bestk[row + k] = g.bestk;
        best = db_max(best, g.acc);
    }
    s_best[threadIdx.x] = best;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s_best[threadIdx.x] = db_max(s_best[threadIdx.x], s_best[threadIdx.x + h]);
        __syncthreads();
    }
    best = s_best[0];
    for (int k = threadIdx.x; k < K; k += 256) {
        const int bk = w.bestk[row + k];
        if (bk >= 0 && db_retained(w.acc[row + k], best)) w.mark[row + bk] = 1;   // candidateKFs.insert (a set)
    }
    __syncthreads();
    // the marks, ascending: each thread owns `per` consecutive slots
    const int per = (K + 255) / 256;
    const int k0 = min((int)threadIdx.x * per, K), k1 = min(k0 + per, K);
    int c = 0;
    for (int k = k0; k < k1; k++) c += w.mark[row + k];
    s_part[threadIdx.x] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int t = 0; t < 256; t++) { const int x = s_part[t]; s_part[t] = run; run += x; }
        s_part[256] = run;
        n_cand[q] = run;
    }
    __syncthreads();
    int pos = s_part[threadIdx.x];
    for (int k = k0; k < k1; k++)
        if (w.mark[row + k]) cand[row + pos++] = k;
    const int total = s_part[256];
    for (int i = total + (int)threadIdx.x; i < K; i += 256) cand[row + i] = -1;
}

// minScore of Detect: 16 wavefronts per query take its covisible slots in turn; the running minimum changes on a
// strict comparison only (std::min), so among equal values the earliest entry's stays: (value, entry) pairs.
__global__ __launch_bounds__(1024) void db_min_score_kernel(DbQuery b, DbSlots s, const int32_t* cov_off,
                                                            const int32_t* cov_idx, float* min_score) {
    __shared__ float s_val[16];
    __shared__ int s_ent[16];
    const int q = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t* qw;
    const double* qv;
    const int nq = db_query(b, q, qw, qv);
    const int e0 = cov_off[q], e1 = cov_off[q + 1];
    float m = 1.f;   // float minScore = 1.f
    int ent = -1;
    for (int e = e0 + wave; e0 >= 0 && e < e1; e += 16) {
        const int k = cov_idx[e];
        if (k < 0 || k >= s.K || !s.live[k]) continue;   // wave-uniform
        const double sum = db_wave_score(qw, qv, nq, s.word + (size_t)k * s.W, s.weight + (size_t)k * s.W,
                                         db_slot_words(s, k), lane);
        const float sc = (float)db_finish(sum);
        if (sc < m) { m = sc; ent = e; }
    }
    if (lane == 0) { s_val[wave] = m; s_ent[wave] = ent; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int t = 1; t < 16; t++) {
            const bool take = s_ent[t] >= 0 && (s_val[t] < m || (!(m < s_val[t]) && ent >= 0 && s_ent[t] < ent));
            if (take) { m = s_val[t]; ent = s_ent[t]; }
        }
        min_score[q] = m;
    }
}

__global__ __launch_bounds__(256) void db_add_kernel(DbStore d, const int32_t* slot, const int32_t* frame,
                                                     const uint32_t* bow_word, const double* bow_weight,
                                                     const int32_t* n_words, int cap, int n_frames) {
    const int i = blockIdx.x;
    const int k = slot[i], f = frame ? frame[i] : i;
    if (k < 0 || k >= d.K || f < 0 || f >= n_frames) return;
    const int n = n_words[f];
    if (n < 0 || n > d.W || n > cap) return;
    for (int t = threadIdx.x; t < n; t += 256) {
        d.word[(size_t)k * d.W + t] = bow_word[(size_t)f * cap + t];
        d.weight[(size_t)k * d.W + t] = bow_weight[(size_t)f * cap + t];
    }
    if (threadIdx.x == 0) {
        d.nw[k] = n;
        d.live[k] = 1;
        d.reloc[k] = 0.f;
    }
}

__global__ __launch_bounds__(256) void db_erase_kernel(uint8_t* live, int K, const int32_t* slot, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int k = slot[i];
    if (k >= 0 && k < K) live[k] = 0;
}

}  // namespace orbamd

using namespace orbamd;

namespace {

DbStore db_view(const orbdb_database* db) { return DbStore{db->live, db->nw, db->reloc, db->word, db->weight, db->K, db->W}; }

DbSlots db_slots(const orbdb_database* db) { return DbSlots{db->live, db->nw, db->word, db->weight, db->K, db->W}; }

int db_check_query(const orbdb_database* db, const orbdb_query_batch* b, bool covis) {
    ORB_CHECK_ARG(db && b, "null database or batch");
    ORB_CHECK_ARG(b->n_queries >= 0, "n_queries must not be negative");
    ORB_CHECK_ARG(b->cap >= 1 && b->cap <= DB_MAXQ, "cap must be in [1, ORBV_MAX_FEATURES]");
    ORB_CHECK_ARG(b->n_frames >= 0, "n_frames must not be negative");
    if (b->n_queries == 0) return ORB_OK;
    ORB_CHECK_ARG(b->bow_word && b->bow_weight && b->n_words, "null query BowVector array");
    ORB_CHECK_ARG(!covis || b->covis, "null covisibility table");
    return ORB_OK;
}

DbQuery db_query_view(const orbdb_query_batch* b) {
    return DbQuery{b->bow_word, b->bow_weight, b->n_words, b->frame, b->cap, b->n_frames};
}

int db_detect(orbdb_database* db, const orbdb_query_batch* b, const orbdb_result* out, bool loop, hipStream_t st) {
    int rc;
    if ((rc = db_check_query(db, b, true))) return rc;
    ORB_CHECK_ARG(out, "null result");
    if (b->n_queries == 0) return ORB_OK;
    ORB_CHECK_ARG(out->cand && out->n_cand, "null candidate output");
    ORB_CHECK_ARG(!loop || (b->conn_off && b->conn_idx && b->min_score), "null connected set or min_score");
    ORB_HIP_TRY(hipSetDevice(db->device));
    const int Q = b->n_queries, K = db->K;
    const size_t n = (size_t)Q * K, a4 = align_up(n * 4, 256), a1 = align_up(n, 256);
    if ((rc = db->ws.reserve(a4 * 5 + a1 * 3))) return rc;
    char* p = db->ws.as<char>();
    DbWork w;
    w.words = out->words ? out->words : (int32_t*)p;
    w.score = out->score ? out->score : (float*)(p + a4);
    w.acc = out->acc ? out->acc : (float*)(p + a4 * 2);
    w.bestk = out->bestk ? out->bestk : (int32_t*)(p + a4 * 3);
    w.eff = (float*)(p + a4 * 4);
    w.scored = out->scored ? out->scored : (uint8_t*)(p + a4 * 5);
    w.in_s = (uint8_t*)(p + a4 * 5 + a1);
    w.mark = (uint8_t*)(p + a4 * 5 + a1 * 2);
    const DbQuery qv = db_query_view(b);
    const DbSlots sl = db_slots(db);
    const int wblocks = (K + DB_WAVES * DB_SLOTS_PER_WAVE - 1) / (DB_WAVES * DB_SLOTS_PER_WAVE);
    const int sblocks = (K + DB_WAVES - 1) / DB_WAVES;
    ORB_CHECK_ARG((long long)Q * sblocks <= 0x7fffffffLL, "n_queries x max_keyframes too large for one call");
    hipLaunchKernelGGL(db_words_kernel, dim3((unsigned)(Q * wblocks)), dim3(256), 0, st, qv, sl, wblocks, w.words);
    hipLaunchKernelGGL(db_select_kernel, dim3(Q), dim3(256), 0, st, sl, w, loop ? b->conn_off : nullptr,
                       loop ? b->conn_idx : nullptr);
    hipLaunchKernelGGL(db_score_kernel, dim3((unsigned)(Q * sblocks)), dim3(256), 0, st, qv, sl, sblocks, w.scored,
                       w.score);
    if (!loop)
        hipLaunchKernelGGL(db_reloc_scan_kernel, dim3((K + 255) / 256), dim3(256), 0, st, Q, K, w.scored, w.score, w.eff,
                           db->reloc);
    hipLaunchKernelGGL(db_group_kernel, dim3(Q), dim3(256), 0, st, K, w, b->covis, loop ? b->min_score : nullptr,
                       out->cand, out->n_cand);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

// ---- host forms: validation (before any device call) and staging

int db_check_host_query(const orbdb_database* db, const orbdb_query_batch* b, bool covis) {
    int rc;
    if ((rc = db_check_query(db, b, covis))) return rc;
    for (int q = 0; q < b->n_queries; q++) {
        const int f = b->frame ? b->frame[q] : q;
        ORB_CHECK_ARG(f >= 0 && f < b->n_frames, "query frame outside [0, n_frames)");
        ORB_CHECK_ARG(b->n_words[f] >= 0 && b->n_words[f] <= b->cap, "query n_words outside [0, cap]");
    }
    if (covis && b->n_queries)
        for (size_t i = 0; i < (size_t)db->K * DB_COVIS; i++)
            ORB_CHECK_ARG(b->covis[i] >= -1 && b->covis[i] < db->K, "covisibility entry outside [-1, max_keyframes)");
    return ORB_OK;
}

int db_check_csr(const orbdb_database* db, int Q, const int32_t* off, const int32_t* idx, const char* what) {
    ORB_CHECK_ARG(off && off[0] == 0, std::string(what) + ": offsets must start at 0");
    for (int q = 0; q < Q; q++) ORB_CHECK_ARG(off[q + 1] >= off[q], std::string(what) + ": offsets must not decrease");
    ORB_CHECK_ARG(off[Q] == 0 || idx, std::string(what) + ": null index array");
    for (int e = 0; e < off[Q]; e++)
        ORB_CHECK_ARG(idx[e] >= 0 && idx[e] < db->K, std::string(what) + ": slot outside [0, max_keyframes)");
    return ORB_OK;
}

struct Stage {   // bump allocation in the handle's staging buffer, two passes: measure, then place
    size_t o = 0;
    char* base = nullptr;
    size_t take(size_t bytes) { const size_t r = o; o += align_up(std::max<size_t>(bytes, 1), 256); return r; }
};

int db_detect_host(orbdb_database* db, const orbdb_query_batch* b, const orbdb_result* out, bool loop) {
    int rc;
    if ((rc = db_check_host_query(db, b, true))) return rc;
    ORB_CHECK_ARG(out, "null result");
    if (b->n_queries == 0) return ORB_OK;
    ORB_CHECK_ARG(out->cand && out->n_cand, "null candidate output");
    const int Q = b->n_queries, K = db->K;
    int nconn = 0;
    if (loop) {
        ORB_CHECK_ARG(b->min_score, "null min_score");
        if ((rc = db_check_csr(db, Q, b->conn_off, b->conn_idx, "connected set"))) return rc;
        nconn = b->conn_off[Q];
    }
    ORB_HIP_TRY(hipSetDevice(db->device));
    const size_t F = (size_t)b->n_frames, n = (size_t)Q * K;
    Stage s;
    const size_t o_w = s.take(F * b->cap * 4), o_v = s.take(F * b->cap * 8), o_n = s.take(F * 4), o_f = s.take((size_t)Q * 4),
                 o_cv = s.take((size_t)K * DB_COVIS * 4), o_co = s.take((size_t)(Q + 1) * 4), o_ci = s.take((size_t)nconn * 4),
                 o_ms = s.take((size_t)Q * 4), o_cand = s.take(n * 4), o_nc = s.take((size_t)Q * 4), o_words = s.take(n * 4),
                 o_scored = s.take(n), o_score = s.take(n * 4), o_acc = s.take(n * 4), o_bk = s.take(n * 4);
    if ((rc = db->io.reserve(s.o))) return rc;
    char* d = db->io.as<char>();
    ORB_HIP_TRY(hipMemcpy(d + o_w, b->bow_word, F * b->cap * 4, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(d + o_v, b->bow_weight, F * b->cap * 8, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(d + o_n, b->n_words, F * 4, hipMemcpyHostToDevice));
    if (b->frame) ORB_HIP_TRY(hipMemcpy(d + o_f, b->frame, (size_t)Q * 4, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(d + o_cv, b->covis, (size_t)K * DB_COVIS * 4, hipMemcpyHostToDevice));
    orbdb_query_batch g = *b;
    g.bow_word = (const uint32_t*)(d + o_w);
    g.bow_weight = (const double*)(d + o_v);
    g.n_words = (const int32_t*)(d + o_n);
    g.frame = b->frame ? (const int32_t*)(d + o_f) : nullptr;
    g.covis = (const int32_t*)(d + o_cv);
    if (loop) {
        ORB_HIP_TRY(hipMemcpy(d + o_co, b->conn_off, (size_t)(Q + 1) * 4, hipMemcpyHostToDevice));
        if (nconn) ORB_HIP_TRY(hipMemcpy(d + o_ci, b->conn_idx, (size_t)nconn * 4, hipMemcpyHostToDevice));
        ORB_HIP_TRY(hipMemcpy(d + o_ms, b->min_score, (size_t)Q * 4, hipMemcpyHostToDevice));
        g.conn_off = (const int32_t*)(d + o_co);
        g.conn_idx = (const int32_t*)(d + o_ci);
        g.min_score = (const float*)(d + o_ms);
    }
    const orbdb_result r{(int32_t*)(d + o_cand), (int32_t*)(d + o_nc), (int32_t*)(d + o_words), (uint8_t*)(d + o_scored),
                         (float*)(d + o_score), (float*)(d + o_acc), (int32_t*)(d + o_bk)};
    if ((rc = db_detect(db, &g, &r, loop, nullptr))) return rc;
    ORB_HIP_TRY(hipMemcpy(out->cand, r.cand, n * 4, hipMemcpyDeviceToHost));
    ORB_HIP_TRY(hipMemcpy(out->n_cand, r.n_cand, (size_t)Q * 4, hipMemcpyDeviceToHost));
    if (out->words) ORB_HIP_TRY(hipMemcpy(out->words, r.words, n * 4, hipMemcpyDeviceToHost));
    if (out->scored) ORB_HIP_TRY(hipMemcpy(out->scored, r.scored, n, hipMemcpyDeviceToHost));
    if (out->score) ORB_HIP_TRY(hipMemcpy(out->score, r.score, n * 4, hipMemcpyDeviceToHost));
    if (out->acc) ORB_HIP_TRY(hipMemcpy(out->acc, r.acc, n * 4, hipMemcpyDeviceToHost));
    if (out->bestk) ORB_HIP_TRY(hipMemcpy(out->bestk, r.bestk, n * 4, hipMemcpyDeviceToHost));
    return ORB_OK;
}

}  // namespace

extern "C" int orbdb_create(const orbv_vocabulary* voc, int max_keyframes, int word_cap, int device,
                            orbdb_database** out) {
    ORB_CHECK_ARG(voc && out, "null vocabulary or output");
    int scoring = -1;
    const int rc0 = orbv_info(voc, nullptr, nullptr, nullptr, nullptr, &scoring, nullptr);
    if (rc0) return rc0;
    ORB_CHECK_ARG(scoring == 0, "KeyFrameDatabase: only L1_NORM scoring (0, ORBvoc's) is supported");
    ORB_CHECK_ARG(max_keyframes >= 1 && max_keyframes <= (1 << 20), "max_keyframes must be in [1, 1048576]");
    ORB_CHECK_ARG(word_cap >= 1 && word_cap <= DB_MAXQ, "word_cap must be in [1, ORBV_MAX_FEATURES]");
    ORB_HIP_TRY(hipSetDevice(device));
    orbdb_database* db = new orbdb_database;
    db->device = device;
    db->K = max_keyframes;
    db->W = word_cap;
    const size_t K = (size_t)max_keyframes, W = (size_t)word_cap;
    Stage s;
    const size_t o_l = s.take(K), o_n = s.take(K * 4), o_r = s.take(K * 4), o_w = s.take(K * W * 4), o_v = s.take(K * W * 8);
    const int rc = db->buf.reserve(s.o);
    if (rc) { delete db; return rc; }
    char* b = db->buf.as<char>();
    db->live = (uint8_t*)(b + o_l);
    db->nw = (int32_t*)(b + o_n);
    db->reloc = (float*)(b + o_r);
    db->word = (uint32_t*)(b + o_w);
    db->weight = (double*)(b + o_v);
    const hipError_t e = hipMemset(b, 0, o_w);   // flags, counts, reloc_score
    if (e != hipSuccess) {
        set_error(std::string("hipMemset: ") + hipGetErrorString(e));
        db->buf.release();
        delete db;
        return ORB_EHIP;
    }
    *out = db;
    return ORB_OK;
}

extern "C" int orbdb_destroy(orbdb_database* db) {
    if (!db) return ORB_OK;
    (void)hipSetDevice(db->device);
    db->buf.release();
    db->ws.release();
    db->io.release();
    delete db;
    return ORB_OK;
}

extern "C" int orbdb_info(const orbdb_database* db, int* max_keyframes, int* word_cap) {
    ORB_CHECK_ARG(db, "null database");
    if (max_keyframes) *max_keyframes = db->K;
    if (word_cap) *word_cap = db->W;
    return ORB_OK;
}

extern "C" int orbdb_clear(orbdb_database* db, void* stream) {
    ORB_CHECK_ARG(db, "null database");
    ORB_HIP_TRY(hipSetDevice(db->device));
    ORB_HIP_TRY(hipMemsetAsync(db->live, 0, (size_t)db->K, (hipStream_t)stream));
    return ORB_OK;
}

extern "C" int orbdb_add_device(orbdb_database* db, int n, const int32_t* d_slot, const int32_t* d_frame,
                                const uint32_t* d_bow_word, const double* d_bow_weight, const int32_t* d_n_words,
                                int cap, int n_frames, void* stream) {
    ORB_CHECK_ARG(db, "null database");
    ORB_CHECK_ARG(n >= 0 && n_frames >= 0, "n and n_frames must not be negative");
    ORB_CHECK_ARG(cap >= 1 && cap <= DB_MAXQ, "cap must be in [1, ORBV_MAX_FEATURES]");
    if (n == 0) return ORB_OK;
    ORB_CHECK_ARG(d_slot && d_bow_word && d_bow_weight && d_n_words, "null device array");
    ORB_HIP_TRY(hipSetDevice(db->device));
    hipLaunchKernelGGL(db_add_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, db_view(db), d_slot, d_frame,
                       d_bow_word, d_bow_weight, d_n_words, cap, n_frames);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbdb_erase_device(orbdb_database* db, int n, const int32_t* d_slot, void* stream) {
    ORB_CHECK_ARG(db, "null database");
    ORB_CHECK_ARG(n >= 0, "n must not be negative");
    if (n == 0) return ORB_OK;
    ORB_CHECK_ARG(d_slot, "null device array");
    ORB_HIP_TRY(hipSetDevice(db->device));
    hipLaunchKernelGGL(db_erase_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, db->live, db->K,
                       d_slot, n);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbdb_min_score_device(orbdb_database* db, const orbdb_query_batch* b, const int32_t* d_cov_off,
                                      const int32_t* d_cov_idx, float* d_min_score, void* stream) {
    int rc;
    if ((rc = db_check_query(db, b, false))) return rc;
    if (b->n_queries == 0) return ORB_OK;
    ORB_CHECK_ARG(d_cov_off && d_cov_idx && d_min_score, "null covisible list or output");
    ORB_HIP_TRY(hipSetDevice(db->device));
    hipLaunchKernelGGL(db_min_score_kernel, dim3(b->n_queries), dim3(1024), 0, (hipStream_t)stream, db_query_view(b),
                       db_slots(db), d_cov_off, d_cov_idx, d_min_score);
    ORB_HIP_TRY(hipGetLastError());
    return ORB_OK;
}

extern "C" int orbdb_detect_reloc_device(orbdb_database* db, const orbdb_query_batch* b, const orbdb_result* out,
                                         void* stream) {
    return db_detect(db, b, out, false, (hipStream_t)stream);
}

extern "C" int orbdb_detect_loop_device(orbdb_database* db, const orbdb_query_batch* b, const orbdb_result* out,
                                        void* stream) {
    return db_detect(db, b, out, true, (hipStream_t)stream);
}

extern "C" int orbdb_add(orbdb_database* db, int n, const int32_t* slot, const int32_t* frame, const uint32_t* bow_word,
                         const double* bow_weight, const int32_t* n_words, int cap, int n_frames) {
    ORB_CHECK_ARG(db, "null database");
    ORB_CHECK_ARG(n >= 0 && n_frames >= 0, "n and n_frames must not be negative");
    ORB_CHECK_ARG(cap >= 1 && cap <= DB_MAXQ, "cap must be in [1, ORBV_MAX_FEATURES]");
    if (n == 0) return ORB_OK;
    ORB_CHECK_ARG(slot && bow_word && bow_weight && n_words, "null array");
    std::vector<uint8_t> seen((size_t)db->K, 0);
    for (int i = 0; i < n; i++) {
        ORB_CHECK_ARG(slot[i] >= 0 && slot[i] < db->K, "slot outside [0, max_keyframes)");
        ORB_CHECK_ARG(!seen[slot[i]], "a slot is named twice in one add");
        seen[slot[i]] = 1;
        const int f = frame ? frame[i] : i;
        ORB_CHECK_ARG(f >= 0 && f < n_frames, "frame outside [0, n_frames)");
        ORB_CHECK_ARG(n_words[f] >= 0 && n_words[f] <= cap, "n_words outside [0, cap]");
        ORB_CHECK_ARG(n_words[f] <= db->W, "n_words > word_cap");
    }
    ORB_HIP_TRY(hipSetDevice(db->device));
    const size_t F = (size_t)n_frames;
    Stage s;
    const size_t o_s = s.take((size_t)n * 4), o_f = s.take((size_t)n * 4), o_w = s.take(F * cap * 4),
                 o_v = s.take(F * cap * 8), o_n = s.take(F * 4);
    int rc;
    if ((rc = db->io.reserve(s.o))) return rc;
    char* d = db->io.as<char>();
    ORB_HIP_TRY(hipMemcpy(d + o_s, slot, (size_t)n * 4, hipMemcpyHostToDevice));
    if (frame) ORB_HIP_TRY(hipMemcpy(d + o_f, frame, (size_t)n * 4, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(d + o_w, bow_word, F * cap * 4, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(d + o_v, bow_weight, F * cap * 8, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(d + o_n, n_words, F * 4, hipMemcpyHostToDevice));
    if ((rc = orbdb_add_device(db, n, (const int32_t*)(d + o_s), frame ? (const int32_t*)(d + o_f) : nullptr,
                               (const uint32_t*)(d + o_w), (const double*)(d + o_v), (const int32_t*)(d + o_n), cap,
                               n_frames, nullptr)))
        return rc;
    ORB_HIP_TRY(hipStreamSynchronize(nullptr));
    return ORB_OK;
}

extern "C" int orbdb_erase(orbdb_database* db, int n, const int32_t* slot) {
    ORB_CHECK_ARG(db, "null database");
    ORB_CHECK_ARG(n >= 0, "n must not be negative");
    if (n == 0) return ORB_OK;
    ORB_CHECK_ARG(slot, "null array");
    for (int i = 0; i < n; i++) ORB_CHECK_ARG(slot[i] >= 0 && slot[i] < db->K, "slot outside [0, max_keyframes)");
    ORB_HIP_TRY(hipSetDevice(db->device));
    int rc;
    if ((rc = db->io.reserve(align_up((size_t)n * 4, 256)))) return rc;
    ORB_HIP_TRY(hipMemcpy(db->io.ptr, slot, (size_t)n * 4, hipMemcpyHostToDevice));
    if ((rc = orbdb_erase_device(db, n, db->io.as<int32_t>(), nullptr))) return rc;
    ORB_HIP_TRY(hipStreamSynchronize(nullptr));
    return ORB_OK;
}

extern "C" int orbdb_min_score(orbdb_database* db, const orbdb_query_batch* b, const int32_t* cov_off,
                               const int32_t* cov_idx, float* min_score) {
    int rc;
    if ((rc = db_check_host_query(db, b, false))) return rc;
    if (b->n_queries == 0) return ORB_OK;
    ORB_CHECK_ARG(min_score, "null output");
    const int Q = b->n_queries;
    if ((rc = db_check_csr(db, Q, cov_off, cov_idx, "covisible list"))) return rc;
    const int nc = cov_off[Q];
    ORB_HIP_TRY(hipSetDevice(db->device));
    const size_t F = (size_t)b->n_frames;
    Stage s;
    const size_t o_w = s.take(F * b->cap * 4), o_v = s.take(F * b->cap * 8), o_n = s.take(F * 4), o_f = s.take((size_t)Q * 4),
                 o_co = s.take((size_t)(Q + 1) * 4), o_ci = s.take((size_t)nc * 4), o_ms = s.take((size_t)Q * 4);
    if ((rc = db->io.reserve(s.o))) return rc;
    char* d = db->io.as<char>();
    ORB_HIP_TRY(hipMemcpy(d + o_w, b->bow_word, F * b->cap * 4, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(d + o_v, b->bow_weight, F * b->cap * 8, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(d + o_n, b->n_words, F * 4, hipMemcpyHostToDevice));
    if (b->frame) ORB_HIP_TRY(hipMemcpy(d + o_f, b->frame, (size_t)Q * 4, hipMemcpyHostToDevice));
    ORB_HIP_TRY(hipMemcpy(d + o_co, cov_off, (size_t)(Q + 1) * 4, hipMemcpyHostToDevice));
    if (nc) ORB_HIP_TRY(hipMemcpy(d + o_ci, cov_idx, (size_t)nc * 4, hipMemcpyHostToDevice));
    orbdb_query_batch g = *b;
    g.bow_word = (const uint32_t*)(d + o_w);
    g.bow_weight = (const double*)(d + o_v);
    g.n_words = (const int32_t*)(d + o_n);
    g.frame = b->frame ? (const int32_t*)(d + o_f) : nullptr;
    if ((rc = orbdb_min_score_device(db, &g, (const int32_t*)(d + o_co), (const int32_t*)(d + o_ci), (float*)(d + o_ms),
                                     nullptr)))
        return rc;
    ORB_HIP_TRY(hipMemcpy(min_score, d + o_ms, (size_t)Q * 4, hipMemcpyDeviceToHost));
    return ORB_OK;
}

extern "C" int orbdb_detect_reloc(orbdb_database* db, const orbdb_query_batch* b, const orbdb_result* out) {
    return db_detect_host(db, b, out, false);
}

extern "C" int orbdb_detect_loop(orbdb_database* db, const orbdb_query_batch* b, const orbdb_result* out) {
    return db_detect_host(db, b, out, true);
}

extern "C" int orbdb_read_slots(orbdb_database* db, uint8_t* live, float* reloc_score) {
    ORB_CHECK_ARG(db, "null database");
    ORB_HIP_TRY(hipSetDevice(db->device));
    if (live) ORB_HIP_TRY(hipMemcpy(live, db->live, (size_t)db->K, hipMemcpyDeviceToHost));
    if (reloc_score) ORB_HIP_TRY(hipMemcpy(reloc_score, db->reloc, (size_t)db->K * 4, hipMemcpyDeviceToHost));
    return ORB_OK;
}
