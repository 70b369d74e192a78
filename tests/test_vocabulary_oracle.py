"""CPU checks of the DBoW2 restatement (oracle/orb_oracle.cpp Vocabulary; TemplatedVocabulary.h
:1130-1263, :1341-1431) against an independent numpy restatement, and of the text loader against
the array form.  The real ORBvoc.txt is absent, so vocabularies are synthetic (synth.make_vocabulary);
the reference ships no BoW fixtures (parity unpinned vs a real DBoW2 build).

The hand-built cases of tests/vocabulary_cases.py follow: for each the oracle equals the restatement bit for bit, and each plant
is shown to do what it is there for (a tie that the last-minimum rule resolves differently, a word whose features differ in
weight, a sum that is not n * w, a fan-out that a feature really descends through), so the GPU tests on the same cases
(tests/test_vocabulary_gpu.py) cannot pass vacuously."""
import numpy as np
import pytest

import vocabulary_cases as VC
from orb_slam2_refactored_amd.synth import make_vocabulary, vocabulary_features, write_vocabulary_text
from vocabulary_ref import children_of, descend, np_transform as _np_transform, word_ids


@pytest.mark.parametrize("kw,levelsup", [
    (dict(seed=0), 4), (dict(seed=1, L=5, k=6), 2), (dict(seed=2, scoring=1, weighting=1), 1),
    (dict(seed=3, scoring=5, weighting=0), 3), (dict(seed=4, scoring=5, weighting=2, order="dfs"), 2),
    (dict(seed=5, weighting=3, early_leaf=0.3), 0), (dict(seed=6, k=12, L=3, early_leaf=0.0), 5),
])
def test_oracle_transform_matches_numpy(oracle, kw, levelsup):
    voc = make_vocabulary(**kw)
    X = vocabulary_features(voc, 100 + kw["seed"], 400)
    (bw, bv), (fn, fo, fi) = oracle.Vocabulary(voc).transform(X, levelsup)
    (nbw, nbv), (nfn, nfo, nfi) = _np_transform(voc, X, levelsup)
    assert np.array_equal(bw, nbw) and np.array_equal(bv, nbv)   # bit-exact doubles
    assert np.array_equal(fn, nfn) and np.array_equal(fo, nfo) and np.array_equal(fi, nfi)


def test_text_loader_equals_arrays(oracle, tmp_path):
    voc = make_vocabulary(7, order="dfs", early_leaf=0.2)
    p = tmp_path / "voc.txt"
    write_vocabulary_text(voc, p)
    a, b = oracle.Vocabulary(voc), oracle.Vocabulary(path=p)
    assert a.info() == b.info()
    X = vocabulary_features(voc, 8, 300)
    ra, rb = a.transform(X, 2), b.transform(X, 2)
    for u, v in zip(ra[0] + ra[1], rb[0] + rb[1]):
        assert np.array_equal(u, v)


def test_empty_input_and_stopped_words(oracle):
    voc = make_vocabulary(9, stop_frac=1.0)   # every word stopped: both vectors empty
    (bw, bv), (fn, fo, fi) = oracle.Vocabulary(voc).transform(vocabulary_features(voc, 1, 50))
    assert len(bw) == 0 and len(fn) == 0 and list(fo) == [0]
    (bw, bv), (fn, fo, fi) = oracle.Vocabulary(make_vocabulary(10)).transform(np.zeros((0, 32), np.uint8))
    assert len(bw) == 0 and len(fn) == 0


# ---- tests/vocabulary_cases.py ------------------------------------------------------------------------------------------------

def _equal(a, b):
    (aw, av), (an, ao, ai) = a
    (bw, bv), (bn, bo, bi) = b
    return (np.array_equal(aw, bw) and np.array_equal(av.view(np.uint64), bv.view(np.uint64)) and np.array_equal(an, bn) and
            np.array_equal(ao, bo) and np.array_equal(ai, bi))


@pytest.mark.parametrize("name", VC.NAMES)
def test_case_oracle_matches_numpy(oracle, name):
    voc, X, levelsup = VC.case(name)
    assert _equal(oracle.Vocabulary(voc).transform(X, levelsup), _np_transform(voc, X, levelsup))


@pytest.mark.parametrize("name", VC.TIE_NAMES)
def test_ties_take_the_first_sibling(oracle, name):
    c = VC.case(name)
    voc, X, levelsup = c
    word, flag, parent = word_ids(voc), voc["is_leaf"], voc["parent"]
    ow, owt, _ = oracle.Vocabulary(voc).words(X, levelsup)
    last = descend(voc, X, first_min=False)
    kids = children_of(voc)
    assert len(c.ties) >= 7
    for q, a, b in c.ties:
        assert a < b and parent[a] == parent[b] and flag[a] and flag[b] and word[a] != word[b]
        assert voc["weight"][a] != voc["weight"][b] and min(voc["weight"][a], voc["weight"][b]) > 0
        d = {n: VC.hamming(X[q], voc["desc"][n]) for n in kids[parent[a]]}
        assert d[a] == d[b] and all(d[n] > d[a] for n in d if n not in (a, b))
        assert ow[q] == word[a] and owt[q] == voc["weight"][a]          # the oracle: the first of the two
        assert last[q][-1] == b                                           # the last-minimum rule: the other one
    assert any(VC.hamming(X[q], voc["desc"][a]) == 0 for q, a, _ in c.ties)
    assert any(VC.hamming(X[q], voc["desc"][a]) > 0 for q, a, _ in c.ties)
    assert not _equal(oracle.Vocabulary(voc).transform(X, levelsup), _np_transform(voc, X, levelsup, first_min=False))


@pytest.mark.parametrize("name,limit,over", [("fanout8_lu1", 16, False), ("fanout64", 64, True)])
def test_fanouts_are_descended(name, limit, over):
    c = VC.case(name)
    voc, X, _ = c
    assert (VC.max_children(voc) > limit) == over          # which voc_descend_kernel the tree takes
    kids = children_of(voc)
    paths = descend(voc, X)
    seen = {len(kids[n]) for p in paths for n in [0] + p[:-1]}
    assert set(c.fanouts) <= seen
    # the extreme distances: a child taken at 256 (the complement) and one at 0
    dist = {VC.hamming(x, voc["desc"][n]) for x, p in zip(X, paths) for n in p}
    assert 256 in dist and 0 in dist


def test_fanout8_depths_and_levelsup_sweep(oracle):
    voc, X, _ = VC.case("fanout8_lu1")
    L = voc["L"]
    assert L == VC.FANOUT8_L
    depths = {len(p) for p in descend(voc, X)}
    assert set(range(1, L + 1)) <= depths and max(depths) > L     # leaves at every depth 1 .. L and one below L
    o = oracle.Vocabulary(voc)
    for lu in range(L + 2):
        c = VC.case(f"fanout8_lu{lu}")
        assert c.levelsup == lu and c.voc["parent"] is not None and np.array_equal(c.X, X)
        fn = o.transform(X, lu)[1][0]
        if L - lu <= 0:
            assert list(fn) == [0]                                # nid = the root
    # nid at level L: a leaf above it stands for itself, the deep chain is cut at L
    _, _, nid = o.words(X, 0)
    paths = descend(voc, X)
    assert any(len(p) < L and nid[i] == p[-1] for i, p in enumerate(paths))
    assert any(len(p) > L and nid[i] == p[L - 1] != p[-1] for i, p in enumerate(paths))


@pytest.mark.parametrize("name", VC.ALIAS_NAMES)
def test_alias_word_sums_each_features_own_weight(oracle, name):
    c = VC.case(name)
    voc, X, levelsup = c
    W, flag = voc["weight"], voc["is_leaf"]
    real, other = sorted(set(c.alias))
    assert flag[real] == 1 and flag[other] == 0 and W[real] != W[other] and W[other] > 0
    assert word_ids(voc)[real] == 0 and not children_of(voc)[other]
    ow, owt, _ = oracle.Vocabulary(voc).words(X, levelsup)
    on_zero = [i for i in range(len(X)) if ow[i] == 0]
    assert [float(owt[i]) for i in on_zero] == [float(W[n]) for n in c.alias]    # both nodes, interleaved
    # without normalisation the value is readable: the running sum, divided by the word count for TF / TF-IDF
    plain = dict(voc, scoring=5)
    (bw, bv), _ = oracle.Vocabulary(plain).transform(X, levelsup)
    assert bw[0] == 0
    first, count = float(W[c.alias[0]]), len(c.alias)
    if voc["weighting"] in (0, 1):
        run = 0.0
        for n in c.alias:
            run += float(W[n])
        assert bv[0] == run / len(bw)
        assert bv[0] != first * count / len(bw)      # "the first feature's weight, once per feature" is another number
        acc = first
        for _ in range(count - 1):
            acc += first
        assert bv[0] != acc / len(bw)
    else:
        assert bv[0] == first                        # addIfNotExist: the first feature's, here the flag-0 node's
        assert first == VC.ALIAS_OTHER


@pytest.mark.parametrize("n", [2, 257, 4096])
def test_one_word_is_a_sequential_sum(oracle, n):
    voc, X, levelsup = VC.case(f"one_word_{n}")
    (bw, bv), (fn, fo, fi) = oracle.Vocabulary(voc).transform(X, levelsup)
    assert len(X) == n and len(bw) == 1 and len(fn) == 1 and list(fo) == [0, n]
    w, run = VC.ONE_WORD_WEIGHT, 0.0
    for _ in range(n):
        run += w
    assert bv[0] == run
    if n == 4096:
        assert run != n * w


def test_all_distinct_all_stopped_and_empty(oracle):
    voc, X, levelsup = VC.case("all_distinct")
    (bw, bv), (fn, fo, fi) = oracle.Vocabulary(voc).transform(X, levelsup)
    assert len(bw) == len(X) == 343 and fo[-1] == len(X)
    voc, X, levelsup = VC.case("all_stopped")
    assert not (voc["weight"] > 0).any() and voc["is_leaf"].any() and len(X) == 100
    for name in ("all_stopped", "root_only", "no_words"):
        voc, X, levelsup = VC.case(name)
        (bw, bv), (fn, fo, fi) = oracle.Vocabulary(voc).transform(X, levelsup)
        assert len(X) > 0 and len(bw) == 0 and len(fn) == 0 and list(fo) == [0]
    assert len(VC.case("root_only").voc["parent"]) == 1
    nw = VC.case("no_words").voc
    assert not nw["is_leaf"].any() and (nw["weight"][1:] > 0).all()


def test_grid_covers_every_scoring_and_weighting():
    seen = {(VC.case(n).voc["scoring"], VC.case(n).voc["weighting"]) for n in VC.NAMES if n.startswith("grid_")}
    assert seen == {(s, w) for s in range(6) for w in range(4)}
    voc, X, _ = VC.case("grid_s1_w0")
    assert len(X) == 300 and any(w != round(w) for w in voc["weight"])   # L2 over non-integers: squares that round


@pytest.mark.parametrize("variant", VC.VARIANTS)
def test_loader_variant_equals_arrays(oracle, tmp_path, variant):
    p = tmp_path / f"{variant}.txt"
    voc, X, levelsup = VC.write_variant(variant, p)
    raw = p.read_bytes()
    assert {"crlf": b"\r\n" in raw, "blank_lines": b"\n\n" in raw and b"\n \t \n" in raw,
            "no_final_newline": not raw.endswith(b"\n"), "tabs": b"\t" in raw and b" " not in raw,
            "exponent": b"e+00" in raw and b"E+00" in raw, "more_than_k": VC.max_children(voc) > voc["k"]}[variant]
    a, b = oracle.Vocabulary(voc), oracle.Vocabulary(path=p)
    assert a.info() == b.info() and a.info()["n_nodes"] == len(voc["parent"])
    assert _equal(a.transform(X, levelsup), b.transform(X, levelsup))
    wa, wb = a.words(voc["desc"][1:], levelsup), b.words(voc["desc"][1:], levelsup)   # every node's descriptor and weight
    assert all(np.array_equal(u, v) for u, v in zip(wa, wb))
