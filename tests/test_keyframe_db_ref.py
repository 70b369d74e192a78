"""tests/keyframe_db_ref.py pinned by hand-built cases, each derived by reading src/KeyFrameDatabase.cc (line numbers in the
tests), and the generator's cases shown to reach both sides of every rule.  CPU only."""
import numpy as np

import keyframe_db_cases as KC
import keyframe_db_ref as R

F32 = np.float32
K = 12
QW, QV = np.arange(10, dtype=np.uint32), np.full(10, 0.1)   # the query: words 0..9, L1-normalised


def vec(common, n=10, filler=50):
    """A keyframe sharing words 0..common-1 with the query, n words in all, equal weights (score = common * 0.1)."""
    w = np.concatenate([np.arange(common), filler + np.arange(n - common)]).astype(np.uint32)
    return w, np.full(n, 1.0 / n)


def db_of(commons):
    db = R.KeyFrameDatabase(K, 16)
    for k, c in commons.items():
        db.add(k, *vec(c, filler=50 + 20 * k))
    return db


def covis_of(rows):
    cv = np.full((K, 10), -1, np.int32)
    for k, row in rows.items():
        cv[k, :len(row)] = row
    return cv


def test_score_is_the_sequential_l1_sum():
    s, c = R.score(QW, QV, *vec(3))
    assert c == 3 and s == -((((0.0 + (0.0 - 0.1 - 0.1)) + (0.0 - 0.1 - 0.1)) + (0.0 - 0.1 - 0.1))) / 2.0
    s0, c0 = R.score(QW, QV, *vec(0))
    assert c0 == 0 and s0 == 0 and np.signbit(s0)          # -score / 2.0 of score = 0 (ScoringObject.cpp:65)
    w1, v1, w2, v2 = [2, 5, 9], [0.5, 0.25, 0.25], [1, 5, 9, 11], [0.1, 0.2, 0.3, 0.4]
    want = -(((abs(0.25 - 0.2) - 0.25) - 0.2) + ((abs(0.25 - 0.3) - 0.25) - 0.3)) / 2.0
    assert R.score(w1, v1, w2, v2) == (want, 2)


def test_minw_truncates_one_float_product():
    assert R.minw_of(5) == 4 and R.minw_of(10) == 8 and R.minw_of(1) == 0 and R.minw_of(4) == 3 and R.minw_of(9) == 7


def test_words_equal_to_minw_is_not_scored_and_one_more_is():
    db = db_of({0: 10, 1: 8, 2: 9, 3: 5, 4: 4})              # maxw 10 -> minw 8 (:204-213)
    r = db.DetectRelocalizationCandidates(QW, QV, covis_of({}))
    assert r["words"][:5].tolist() == [10, 8, 9, 5, 4] and r["scored"][:5].tolist() == [1, 0, 1, 0, 0]
    db = db_of({3: 5, 4: 4})                                 # maxw 5 -> minw 4
    r = db.DetectRelocalizationCandidates(QW, QV, covis_of({}))
    assert r["scored"][3] == 1 and r["scored"][4] == 0 and r["score"][4] == 0 and r["bestk"][4] == -1


def test_score_equal_to_min_score_opens_a_group():
    db = db_of({0: 10, 1: 9})
    s9 = F32(R.score(QW, QV, *vec(9))[0])
    r = db.DetectLoopCandidates(QW, QV, covis_of({}), [], s9)                 # score >= minScore (:119)
    assert r["bestk"][1] == 1 and r["n_groups"] == 2
    r = db.DetectLoopCandidates(QW, QV, covis_of({}), [], np.nextafter(s9, F32(2)))
    assert r["scored"][1] == 1 and r["bestk"][1] == -1 and r["acc"][1] == 0 and r["n_groups"] == 1


def test_acc_equal_to_retain_is_not_a_candidate():
    assert not R.retained(F32(0.75), F32(1.0)) and R.retained(np.nextafter(F32(0.75), F32(1)), F32(1.0))   # > (:166, :260)
    db = R.KeyFrameDatabase(K, 16)
    r = db._finish(db._blank(), [(F32(0.75), 3), (F32(1.0), 4), (F32(0.76), 7)], F32(1.0))
    assert r["n_cand"] == 2 and r["cand"][:3].tolist() == [4, 7, -1] and r["n_retained"] == 2


def test_a_neighbour_with_an_equal_score_does_not_take_bestk():
    db = db_of({0: 10, 1: 10, 2: 9})
    for r in (db.DetectRelocalizationCandidates(QW, QV, covis_of({0: [1, 2], 2: [0, 1]})),
              db.DetectLoopCandidates(QW, QV, covis_of({0: [1, 2], 2: [0, 1]}), [], F32(0))):
        assert r["score"][0] == r["score"][1] and r["bestk"][0] == 0               # > bestScore (:144, :243)
        assert r["bestk"][2] == 0                                                  # the first of two equal better ones
        assert r["acc"][0] == F32(F32(r["score"][0] + r["score"][1]) + r["score"][2])


def test_a_connected_slot_is_neither_candidate_nor_neighbour_term():
    db = db_of({0: 10, 1: 10, 2: 9})
    cv = covis_of({0: [1], 2: [1]})
    r = db.DetectLoopCandidates(QW, QV, cv, [1, 11, -3, 99], F32(0))                # :85; ids outside the slots ignored
    assert r["words"][1] == 10 and r["scored"][1] == 0 and r["acc"][0] == r["score"][0] and r["bestk"][2] == 2
    assert r["cand"][:r["n_cand"]].tolist() == [0, 2]
    r = db.DetectLoopCandidates(QW, QV, cv, [], F32(0))
    assert r["scored"][1] == 1 and r["bestk"][2] == 1 and r["acc"][0] == F32(r["score"][0] + r["score"][1])


def test_an_erased_slot_is_neither():
    db = db_of({0: 10, 1: 10, 2: 9})
    db.erase(1)
    cv = covis_of({0: [1], 2: [1]})
    for r in (db.DetectRelocalizationCandidates(QW, QV, cv), db.DetectLoopCandidates(QW, QV, cv, [], F32(0))):
        assert r["words"][1] == 0 and r["scored"][1] == 0 and r["acc"][0] == r["score"][0] and r["bestk"][2] == 2
        assert r["cand"][:r["n_cand"]].tolist() == [0, 2]


def test_two_groups_with_one_bestk_give_one_candidate():
    db = db_of({0: 10, 1: 9, 2: 9})
    r = db.DetectRelocalizationCandidates(QW, QV, covis_of({1: [0], 2: [0]}))
    assert r["bestk"][:3].tolist() == [0, 0, 0] and r["n_retained"] == 2 and r["n_cand"] == 1 and r["cand"][0] == 0
    assert not R.retained(r["acc"][0], r["acc"][1])         # the keyframe's own group is below 0.75 x the best


def test_a_loop_neighbour_below_min_score_still_adds_to_acc():
    db = db_of({0: 10, 1: 9})
    r = db.DetectLoopCandidates(QW, QV, covis_of({0: [1], 1: [0]}), [], F32(0.95))   # :141-143 test the words only
    assert r["bestk"][1] == -1 and r["acc"][0] == F32(r["score"][0] + r["score"][1]) and r["n_groups"] == 1


def test_relocalisation_reads_the_score_an_earlier_query_left():
    db = db_of({0: 10, 1: 1})
    db.add(2, np.arange(50, 60, dtype=np.uint32), np.full(10, 0.1))                  # shares nothing with the query
    cv = covis_of({0: [1, 2]})
    r = db.DetectRelocalizationCandidates(QW, QV, cv)
    assert r["scored"][1] == 0 and r["words"][1] == 1 and r["acc"][0] == r["score"][0]   # in S, never scored: adds 0
    other = np.array([0, 60, 61], np.uint32), np.array([0.5, 0.25, 0.25])            # a query that scores slot 1
    r1 = db.DetectRelocalizationCandidates(*other, cv)
    assert r1["scored"][1] == 1 and db.reloc_score[1] == r1["score"][1] > 0
    r = db.DetectRelocalizationCandidates(QW, QV, cv)                                # relocQuery == id only (:239-242)
    assert r["scored"][1] == 0 and r["acc"][0] == F32(r["score"][0] + r1["score"][1]) and r["stale"] == [float(r1["score"][1])]
    db.add(1, *vec(1, filler=70))                                                    # a fresh add: 0 again
    r = db.DetectRelocalizationCandidates(QW, QV, cv)
    assert db.reloc_score[1] == 0 and r["acc"][0] == r["score"][0]


def test_empty_query_and_empty_database_give_nothing():
    db = db_of({0: 10})
    none = np.zeros(0, np.uint32), np.zeros(0)
    for r in (db.DetectRelocalizationCandidates(*none, covis_of({})), db.DetectLoopCandidates(*none, covis_of({}), [], F32(0)),
              R.KeyFrameDatabase(K, 16).DetectRelocalizationCandidates(QW, QV, covis_of({})),
              R.KeyFrameDatabase(K, 16).DetectLoopCandidates(QW, QV, covis_of({}), [], F32(0))):
        assert r["n_cand"] == 0 and not r["words"].any() and not r["scored"].any() and (r["cand"] == -1).all()
    assert db.MinScore(QW, QV, []) == 1 and db.MinScore(*none, [0]) == 0 and np.signbit(db.MinScore(*none, [0]))
    db.clear()
    assert db.MinScore(QW, QV, [0]) == 1


def test_the_generators_cases_reach_both_sides_of_every_rule():
    for name in KC.CASES:
        c = KC.case(name)
        assert c["max_keyframes"] == 70 and len(c["slot"]) - len(c["erased"]) == 65
        for kind in ("reloc", "loop"):
            r = KC.reference(name, kind)
            pq = r["per_query"]
            in_s = r["words"] > 0
            assert (r["scored"] == 1).any() and (in_s & (r["scored"] == 0)).any(), (name, kind)          # scored / unscored
            assert 0 < sum(o["n_retained"] for o in pq) < sum(o["n_groups"] for o in pq)                # retained / not
            assert ((r["bestk"] >= 0) & (r["bestk"] != np.arange(70))).any() and (r["bestk"] == np.arange(70)).any()
            assert any(0 < o["n_cand"] < int(o["scored"].sum()) for o in pq)                            # neither none nor all
        assert sum(s > 0 for o in KC.reference(name, "reloc")["per_query"] for s in o["stale"]) > 0     # stale reads > 0
        lp = KC.reference(name, "loop")
        assert any(o["n_groups"] < int(o["scored"].sum()) for o in lp["per_query"]) or name == "plain"  # score < min_score
    counts = set(KC.case("edges")["n_words"].tolist()) | set(KC.case("mixed")["n_words"].tolist())
    assert {0, 1, 63, 64, 65, 200} <= counts
    assert (KC.reference("edges", "reloc")["words"] == 0).all(1).any()                                  # an empty query
