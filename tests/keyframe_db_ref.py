"""numpy restatement of KeyFrameDatabase (src/KeyFrameDatabase.cc:34-265), L1Scoring::score
(Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) and the minScore loop of LoopDetector::Detect
(src/LoopClosing.cc:170-178), on slots: the semantics include/orbslam2_amd.h states for the orbdb_* entries.

A stateful class, one query at a time, the reference's loops in the reference's order.  The score is added up by a
sequential loop over the common words in ascending word order in float64 (never np.sum, which adds pairwise); every
float step (the cast of the score, 0.8f * maxw, the accumulated group score, 0.75f * bestAcc) is np.float32."""
import numpy as np

F32 = np.float32
COVIS = 10


def score(w1, v1, w2, v2):
    """L1Scoring::score(v1, v2) -> (double score, number of common words)."""
    w1, w2 = np.asarray(w1, np.int64), np.asarray(w2, np.int64)
    v1, v2 = np.asarray(v1, np.float64), np.asarray(v2, np.float64)
    _, i1, i2 = np.intersect1d(w1, w2, assume_unique=True, return_indices=True)   # ascending word order
    s = np.float64(0.0)
    for a, b in zip(i1, i2):
        vi, wi = v1[a], v2[b]
        s = s + ((np.abs(vi - wi) - np.abs(vi)) - np.abs(wi))
    return np.float64(-s / np.float64(2.0)), len(i1)


def minw_of(maxw):
    return int(F32(0.8) * F32(maxw))   # static_cast<int>(0.8f * maxCommonWords): truncation


def retained(acc, best_acc):
    return bool(F32(acc) > F32(0.75) * F32(best_acc))


def group_walk(k, score_k, covis_row, member, val):
    """One covisibility group: (acc, bestk)."""
    best = acc = F32(score_k)
    bestk = k
    for nb in covis_row:
        nb = int(nb)
        if nb < 0 or nb >= len(member) or not member[nb]:
            continue
        s = F32(val[nb])
        acc = F32(acc + s)
        if s > best:
            bestk, best = nb, s
    return acc, bestk


class KeyFrameDatabase:
    def __init__(self, max_keyframes, word_cap):
        self.K, self.W = max_keyframes, word_cap
        self.live = np.zeros(max_keyframes, bool)
        self.bow = [(np.zeros(0, np.uint32), np.zeros(0)) for _ in range(max_keyframes)]
        self.reloc_score = np.zeros(max_keyframes, F32)

    def add(self, slot, words, weights):
        assert 0 <= slot < self.K and len(words) <= self.W
        self.bow[slot] = (np.array(words, np.uint32), np.array(weights, np.float64))
        self.live[slot] = True
        self.reloc_score[slot] = F32(0)   # the reference leaves KeyFrame::relocScore uninitialised

    def erase(self, slot):
        self.live[slot] = False

    def clear(self):
        self.live[:] = False

    def _blank(self):
        K = self.K
        return dict(words=np.zeros(K, np.int32), scored=np.zeros(K, np.uint8), score=np.zeros(K, F32), acc=np.zeros(K, F32),
                    bestk=np.full(K, -1, np.int32), cand=np.full(K, -1, np.int32), n_cand=0, stale=[])

    def _share(self, qw, qv, r):
        """words[k] for the live slots (the inverted-file walk's loopWords / relocWords) and their scores."""
        sc = {}
        for k in np.flatnonzero(self.live):
            s, c = score(qw, qv, *self.bow[k])
            r["words"][k] = c
            sc[k] = F32(s)
        return sc

    def MinScore(self, qw, qv, covisible):
        m = F32(1.0)
        for k in covisible:
            if k < 0 or k >= self.K or not self.live[k]:
                continue
            s = F32(score(qw, qv, *self.bow[k])[0])
            if s < m:          # std::min(minScore, score)
                m = s
        return m

    def _finish(self, r, groups, best_acc):
        keep = sorted({bk for acc, bk in groups if retained(acc, best_acc)})
        r["n_cand"] = len(keep)
        r["cand"][:len(keep)] = keep
        r["n_groups"], r["n_retained"] = len(groups), sum(retained(a, best_acc) for a, _ in groups)
        return r

    def DetectRelocalizationCandidates(self, qw, qv, covis):
        r = self._blank()
        sc = self._share(qw, qv, r)
        in_s = self.live & (r["words"] > 0)
        if not in_s.any():
            return self._finish(r, [], F32(0))
        minw = minw_of(r["words"][in_s].max())
        scored = np.flatnonzero(in_s & (r["words"] > minw))
        for k in scored:
            r["scored"][k], r["score"][k] = 1, sc[k]
            self.reloc_score[k] = sc[k]
        groups, best_acc = [], F32(0)
        for k in scored:
            acc, bk = group_walk(int(k), r["score"][k], covis[k], in_s, self.reloc_score)
            r["stale"] += [float(self.reloc_score[nb]) for nb in covis[k] if 0 <= nb < self.K and in_s[nb] and not r["scored"][nb]]
            r["acc"][k], r["bestk"][k] = acc, bk
            groups.append((acc, bk))
            if best_acc < acc:
                best_acc = acc
        return self._finish(r, groups, best_acc)

    def DetectLoopCandidates(self, qw, qv, covis, connected, min_score):
        r = self._blank()
        sc = self._share(qw, qv, r)
        in_s = self.live & (r["words"] > 0)
        for k in connected:
            if 0 <= k < self.K:
                in_s[k] = False
        min_score = F32(min_score)
        if not in_s.any():
            return self._finish(r, [], min_score)
        minw = minw_of(r["words"][in_s].max())
        scored = np.flatnonzero(in_s & (r["words"] > minw))
        for k in scored:
            r["scored"][k], r["score"][k] = 1, sc[k]
        groups, best_acc = [], min_score
        for k in scored:
            if not r["score"][k] >= min_score:
                continue
            acc, bk = group_walk(int(k), r["score"][k], covis[k], r["scored"], r["score"])
            r["acc"][k], r["bestk"][k] = acc, bk
            groups.append((acc, bk))
            if best_acc < acc:
                best_acc = acc
        return self._finish(r, groups, best_acc)


def run_case(case, kind, db=None, queries=None):
    """The generator's case through the restatement: stacked [Q][K] arrays (+ min_score for the loop form)."""
    if db is None:
        db = filled(case)
    out = []
    ms = []
    for q in (range(case["n_queries"]) if queries is None else queries):
        qw, qv = query_of(case, q)
        if kind == "reloc":
            out.append(db.DetectRelocalizationCandidates(qw, qv, case["covis"]))
        else:
            m = db.MinScore(qw, qv, csr(case, "cov", q))
            ms.append(m)
            out.append(db.DetectLoopCandidates(qw, qv, case["covis"], csr(case, "conn", q), m))
    res = {k: np.stack([o[k] for o in out]) for k in ("words", "scored", "score", "acc", "bestk", "cand")}
    res["n_cand"] = np.array([o["n_cand"] for o in out], np.int32)
    res["per_query"] = out
    if kind != "reloc":
        res["min_score"] = np.array(ms, F32)
    res["reloc_score"] = db.reloc_score.copy()
    return res


def query_of(case, q):
    f = int(case["q_frame"][q])
    n = int(case["q_n_words"][f])
    return case["q_bow_word"][f, :n], case["q_bow_weight"][f, :n]


def csr(case, name, q):
    off = case[name + "_off"]
    return [int(x) for x in case[name + "_idx"][off[q]:off[q + 1]]]


def filled(case):
    """A restatement database after the case's adds and erases."""
    db = KeyFrameDatabase(case["max_keyframes"], case["word_cap"])
    for i, k in enumerate(case["slot"]):
        n = int(case["n_words"][i])
        db.add(int(k), case["bow_word"][i, :n], case["bow_weight"][i, :n])
    for k in case["erased"]:
        db.erase(int(k))
    return db
