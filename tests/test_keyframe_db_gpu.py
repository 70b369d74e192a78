"""KeyFrameDatabase on the GPU (orbdb_*, include/orbslam2_amd.h) through the C-ABI against tests/keyframe_db_ref.py: words,
scored, score and acc as float bits, bestk, n_cand, cand, min_score and reloc_score after the batch, all bit-identical, no
entry left out.  Shapes: tests/keyframe_db_cases.py."""
import numpy as np
import pytest

import keyframe_db_cases as KC
import keyframe_db_ref as R
from orb_slam2_refactored_amd.keyframe_db import KeyFrameDatabase
from orb_slam2_refactored_amd.synth import make_vocabulary, vocabulary_features
from orb_slam2_refactored_amd.vocabulary import ORBVocabulary

pytestmark = pytest.mark.gpu

FIELDS = ("words", "scored", "score", "acc", "bestk", "n_cand", "cand")


@pytest.fixture(scope="module")
def voc():
    v = make_vocabulary(0, k=4, L=2)
    return ORBVocabulary.from_arrays(v["k"], v["L"], v["scoring"], v["weighting"], v["parent"], v["is_leaf"], v["desc"], v["weight"])


def filled(voc, c):
    db = KeyFrameDatabase(voc, c["max_keyframes"], c["word_cap"])
    db.add(c["slot"], c["bow_word"], c["bow_weight"], c["n_words"])
    db.erase(c["erased"])
    return db


def same(out, ref, what=""):
    for f in FIELDS:
        g = out[f].cpu().numpy() if hasattr(out[f], "cpu") else out[f]
        assert np.array_equal(KC.bits(g), KC.bits(ref[f])), (what, f)


@pytest.mark.parametrize("name,Q", [("mixed", 1), ("mixed", 3), ("mixed", 5), ("edges", 5), ("plain", 5)])
def test_relocalization_batch_is_bit_identical(voc, name, Q):
    c = KC.case(name)
    db = filled(voc, c)
    live, rs = db.slots()
    assert live.sum() == 65 and not rs.any()
    out = db.DetectRelocalizationCandidates(KC.query(c, Q))
    ref = KC.reference(name, "reloc", Q)
    same(out, ref, (name, Q))
    assert np.array_equal(KC.bits(db.slots()[1]), KC.bits(ref["reloc_score"]))


@pytest.mark.parametrize("name,Q", [("mixed", 1), ("mixed", 3), ("mixed", 5), ("edges", 5), ("plain", 5)])
def test_loop_batch_with_min_score_on_the_device_is_bit_identical(voc, name, Q):
    """MinScore's output stays on the device and is what the loop query reads."""
    import torch
    c = KC.case(name)
    db = filled(voc, c)
    q = {k: torch.from_numpy(np.ascontiguousarray(v).view(np.int32) if v.dtype == np.uint32 else np.ascontiguousarray(v)).cuda()
         for k, v in KC.query(c, Q).items()}
    ms = db.min_score_device(q, q["cov_off"], q["cov_idx"])
    out = db.detect_loop_candidates_device(q, ms)
    torch.cuda.synchronize()
    ref = KC.reference(name, "loop", Q)
    assert np.array_equal(KC.bits(ms.cpu().numpy()), KC.bits(ref["min_score"]))
    same(out, ref, (name, Q))
    assert np.array_equal(db.MinScore(KC.query(c, Q), c["cov_off"][:Q + 1], c["cov_idx"]).view(np.uint32), KC.bits(ref["min_score"]))
    assert not db.slots()[1].any()   # the loop query leaves reloc_score alone


def test_a_batch_of_five_equals_five_batches_of_one_and_a_rerun_on_a_copy(voc):
    c = KC.case("mixed")
    a, b, a2 = filled(voc, c), filled(voc, c), filled(voc, c)
    qa = KC.query(c)
    whole = a.DetectRelocalizationCandidates(qa)
    again = a2.DetectRelocalizationCandidates(qa)
    for q in range(5):
        one = b.DetectRelocalizationCandidates(dict(qa, frame=c["q_frame"][q:q + 1]))
        for f in FIELDS:
            assert np.array_equal(KC.bits(one[f][0]), KC.bits(whole[f][q])), (q, f)
    for f in FIELDS:
        assert np.array_equal(KC.bits(again[f]), KC.bits(whole[f])), f
    assert np.array_equal(KC.bits(a.slots()[1]), KC.bits(b.slots()[1])) and np.array_equal(KC.bits(a.slots()[1]), KC.bits(a2.slots()[1]))


def test_add_after_erase_into_the_same_slot_and_clear(voc):
    c = KC.case("mixed")
    db, ref = filled(voc, c), R.filled(c)
    q = KC.query(c)
    db.DetectRelocalizationCandidates(q)            # leaves scores behind
    R.run_case(c, "reloc", db=ref)
    k_gone, k_new = int(c["slot"][7]), int(c["erased"][0])
    src = 11                                        # another keyframe's vector into both slots
    n = int(c["n_words"][src])
    for k in (k_gone, k_new):
        db.erase([k])
        ref.erase(k)
        db.add(np.array([k], np.int32), c["bow_word"], c["bow_weight"], c["n_words"], frame=np.array([src], np.int32))
        ref.add(k, c["bow_word"][src, :n], c["bow_weight"][src, :n])
    live, rs = db.slots()
    assert live.sum() == 66 and rs[k_gone] == 0 and rs[k_new] == 0 and np.array_equal(KC.bits(rs), KC.bits(ref.reloc_score))
    want = R.run_case(c, "reloc", db=ref)
    same(db.DetectRelocalizationCandidates(q), want, "re-added")
    assert np.array_equal(KC.bits(db.slots()[1]), KC.bits(want["reloc_score"]))
    db.clear()
    ref.clear()
    assert not db.slots()[0].any()
    for kind, out in (("reloc", db.DetectRelocalizationCandidates(q)), ("loop", db.DetectLoopCandidates(q, np.ones(5, np.float32)))):
        assert not out["n_cand"].any() and not out["words"].any() and not out["scored"].any() and (out["cand"] == -1).all(), kind
    same(db.DetectRelocalizationCandidates(q), R.run_case(c, "reloc", db=ref), "cleared")


def test_transform_output_is_consumed_on_the_device(voc):
    """Slots and queries straight from orbv_transform_batch_device: no BowVector leaves HBM before the query."""
    import torch
    big = make_vocabulary(5, k=10, L=3)
    gv = ORBVocabulary.from_arrays(big["k"], big["L"], big["scoring"], big["weighting"], big["parent"], big["is_leaf"], big["desc"],
                                   big["weight"])
    F, cap = 12, 150
    rng = np.random.default_rng(4)
    counts = np.array([150, 140, 0, 1, 63, 64, 65, 150, 120, 130, 150, 90], np.int32)
    desc = np.zeros((F, cap, 32), np.uint8)
    base = vocabulary_features(big, 9, cap)
    for f in range(F):
        x = vocabulary_features(big, 20 + f, cap)
        keep = rng.random(cap) < 0.6
        desc[f] = np.where(keep[:, None], base, x)
    t = gv.transform_batch_device(torch.from_numpy(desc).cuda(), torch.from_numpy(counts).cuda(), levelsup=2)
    K = 70
    db = KeyFrameDatabase(gv, K, cap)
    slot = np.array([69, 3, 64, 0, 17, 65, 1, 30, 31], np.int32)     # frames 0..8 are keyframes, 9..11 the queries
    db.add_device(torch.from_numpy(slot).cuda(), t["bow_word"], t["bow_weight"], t["n_words"])
    covis = np.full((K, 10), -1, np.int32)
    for i, k in enumerate(slot):
        covis[k, :4] = [slot[(i + 1) % 9], slot[(i + 4) % 9], 5, slot[(i + 7) % 9]]
    q = dict(bow_word=t["bow_word"], bow_weight=t["bow_weight"], n_words=t["n_words"],
             frame=torch.tensor([9, 10, 11], dtype=torch.int32).cuda(), covis=torch.from_numpy(covis).cuda())
    out = db.detect_relocalization_candidates_device(q)
    torch.cuda.synchronize()
    bw, bv, nw = t["bow_word"].cpu().numpy().view(np.uint32), t["bow_weight"].cpu().numpy(), t["n_words"].cpu().numpy()
    ref = R.KeyFrameDatabase(K, cap)
    for i, k in enumerate(slot):
        ref.add(int(k), bw[i, :nw[i]], bv[i, :nw[i]])
    want = [ref.DetectRelocalizationCandidates(bw[f, :nw[f]], bv[f, :nw[f]], covis) for f in (9, 10, 11)]
    for f in FIELDS:
        assert np.array_equal(KC.bits(out[f].cpu().numpy()), KC.bits(np.stack([np.asarray(w[f]) for w in want]))), f
    assert sum(w["n_cand"] for w in want) > 0 and sum(int(w["scored"].sum()) for w in want) > 3
    assert np.array_equal(KC.bits(db.slots()[1]), KC.bits(ref.reloc_score))
