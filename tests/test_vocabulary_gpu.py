"""GPU DBoW2 transform (orbv_*, TemplatedVocabulary.h:1130-1263) vs the oracle: BowVector word ids and
weights (raw doubles) and FeatureVector CSR bit-identical."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import vocabulary_cases as VC
from orb_slam2_refactored_amd._lib import OrbError
from orb_slam2_refactored_amd.synth import make_vocabulary, synth_image, vocabulary_features, write_vocabulary_text
from orb_slam2_refactored_amd.vocabulary import ORBVocabulary

pytestmark = pytest.mark.gpu


def _same(g, o):
    (gw, gv), (gn, go, gi) = g
    (ow, ov), (on, oo, oi) = o
    assert np.array_equal(gw, ow)
    assert np.array_equal(gv.view(np.uint64), ov.view(np.uint64))
    assert np.array_equal(gn, on) and np.array_equal(go, oo) and np.array_equal(gi, oi)


@pytest.mark.parametrize("kw,levelsup,n", [
    (dict(seed=0), 4, 1000), (dict(seed=1, L=5, k=6), 2, 2000), (dict(seed=2, scoring=1, weighting=1), 1, 700),
    (dict(seed=3, scoring=5, weighting=0), 3, 300), (dict(seed=4, scoring=5, weighting=2, order="dfs"), 2, 500),
    (dict(seed=5, weighting=3, early_leaf=0.3), 0, 800), (dict(seed=6, k=12, L=3, early_leaf=0.0), 5, 4096),
    (dict(seed=7, k=20, L=2), 1, 600), (dict(seed=8, stop_frac=0.5), 2, 900),
])
def test_transform_matches_oracle(oracle, kw, levelsup, n):
    voc = make_vocabulary(**kw)
    X = vocabulary_features(voc, 200 + kw["seed"], n)
    g = ORBVocabulary.from_arrays(voc["k"], voc["L"], voc["scoring"], voc["weighting"], voc["parent"],
                                  voc["is_leaf"], voc["desc"], voc["weight"])
    _same(g.transform(X, levelsup), oracle.Vocabulary(voc).transform(X, levelsup))


def test_text_loader_and_limits(oracle, tmp_path):
    voc = make_vocabulary(11, order="dfs", early_leaf=0.2)
    p = tmp_path / "voc.txt"
    write_vocabulary_text(voc, p)
    g = ORBVocabulary.loadFromTextFile(p)
    o = oracle.Vocabulary(path=p)
    assert g.info() == o.info()
    X = vocabulary_features(voc, 12, 1500)
    _same(g.transform(X, 2), o.transform(X, 2))
    _same(g.transform(X[:0], 2), o.transform(X[:0], 2))
    with pytest.raises(OrbError):
        g.transform(np.zeros((4097, 32), np.uint8))
    bad = tmp_path / "bad.txt"
    bad.write_text("30 6 0 0\n")
    with pytest.raises(OrbError):
        ORBVocabulary.loadFromTextFile(bad)


def test_batch_device_on_extracted_frames(oracle):
    """ComputeBoW on a batch straight from orbx_extract_batch_device (descriptors never leave HBM)."""
    import torch
    from orb_slam2_refactored_amd import ORBextractor
    voc = make_vocabulary(13, L=5, k=8)
    g = ORBVocabulary.from_arrays(voc["k"], voc["L"], voc["scoring"], voc["weighting"], voc["parent"],
                                  voc["is_leaf"], voc["desc"], voc["weight"])
    ex = ORBextractor(ORBextractor.Parameters(1000), device=0)
    imgs = torch.from_numpy(np.stack([synth_image(300 + i, 640, 480) for i in range(6)])).cuda()
    kps, desc, counts = ex.extract_batch_device(imgs)
    out = g.transform_batch_device(desc, counts, levelsup=3)
    torch.cuda.synchronize()
    o = oracle.Vocabulary(voc)
    dh, ch = desc.cpu().numpy(), counts.cpu().numpy()
    for f in range(6):
        ow = o.transform(dh[f, :ch[f]], 3)
        nw, nn = int(out["n_words"][f]), int(out["n_nodes"][f])
        off = out["fv_off"][f, :nn + 1].cpu().numpy()
        gw = ((out["bow_word"][f, :nw].cpu().numpy().astype(np.uint32), out["bow_weight"][f, :nw].cpu().numpy()),
              (out["fv_node"][f, :nn].cpu().numpy().astype(np.uint32), off, out["fv_idx"][f, :off[-1]].cpu().numpy()))
        _same(gw, ow)


# ---- tests/vocabulary_cases.py: the branches that make_vocabulary's even k-ary trees do not reach ----------------------------

def _handle(voc):
    return ORBVocabulary.from_arrays(voc["k"], voc["L"], voc["scoring"], voc["weighting"], voc["parent"], voc["is_leaf"],
                                     voc["desc"], voc["weight"])


@pytest.mark.parametrize("name", VC.NAMES)
def test_case_matches_oracle(oracle, name):
    """Uneven fan-out on the 8- and the 64-lane descent, planted ties, a word id shared by two nodes of different weight, one
    word for every feature, a word per feature, all words stopped, no words at all, nid at every level, and every scoring x
    weighting pair.  tests/test_vocabulary_oracle.py shows on the CPU that each plant does what it is named for."""
    voc, X, levelsup = VC.case(name)
    _same(_handle(voc).transform(X, levelsup), oracle.Vocabulary(voc).transform(X, levelsup))


@pytest.fixture(scope="module")
def edge_set(oracle):
    voc = VC.case("fanout8_lu1").voc
    return _handle(voc), oracle.Vocabulary(voc), vocabulary_features(voc, 41, 4096)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 255, 256, 257, 4096])
def test_feature_count_edges(edge_set, n):
    """The aggregate's sort length is the next power of two and its loops stride by 256 threads."""
    g, o, X = edge_set
    _same(g.transform(X[:n], 1), o.transform(X[:n], 1))


def test_handle_reuse_large_small_large(edge_set):
    """One handle keeps its staging and per-feature buffers across calls: a small call after a large one sees stale slots."""
    g, o, X = edge_set
    for sl in (slice(0, 3000), slice(3000, 3005), slice(0, 4096)):
        _same(g.transform(X[sl], 2), o.transform(X[sl], 2))


def _batch_vs_oracle(g, o, desc, counts, levelsup):
    import torch
    F, cap = desc.shape[:2]
    out = g.transform_batch_device(torch.from_numpy(desc).cuda(), torch.from_numpy(counts).cuda(), levelsup=levelsup)
    torch.cuda.synchronize()
    out = {k: v.cpu().numpy() for k, v in out.items()}
    assert out["fv_off"].shape == (F, cap + 1)
    empty = []
    for f in range(F):
        ow = o.transform(desc[f, :counts[f]], levelsup)
        nw, nn = int(out["n_words"][f]), int(out["n_nodes"][f])
        off = out["fv_off"][f, :nn + 1]
        _same(((out["bow_word"][f, :nw].astype(np.uint32), out["bow_weight"][f, :nw]),
               (out["fv_node"][f, :nn].astype(np.uint32), off, out["fv_idx"][f, :off[-1]])), ow)
        if len(ow[0][0]) == 0:
            assert nw == 0 and nn == 0 and out["fv_off"][f, 0] == 0
            empty.append(f)
    return empty


def test_batch_entry_counts_and_caps(oracle):
    """cap = 700 (no power of two), frames that are empty, of one feature, full (count == cap), all on stopped words, and one
    short of full; slots past a frame's count hold other descriptors that must not be read as features.  Then cap = 1."""
    import torch
    voc = make_vocabulary(33, k=6, L=3, stop_frac=0.2)
    g, o = _handle(voc), oracle.Vocabulary(voc)
    cap, counts = 700, np.array([0, 1, 700, 257, 0, 699], np.int32)
    desc = np.stack([vocabulary_features(voc, 50 + f, cap) for f in range(len(counts))])
    stopped = np.nonzero((voc["is_leaf"] == 1) & (voc["weight"] == 0))[0]
    own = [i for i in stopped if o.words(voc["desc"][i:i + 1])[1][0] == 0]      # stopped leaves that their own descriptor reaches
    assert len(own) >= 2
    desc[3, :257] = voc["desc"][np.resize(own, 257)]
    assert _batch_vs_oracle(g, o, desc, counts, 2) == [0, 3, 4]
    empty = _batch_vs_oracle(g, o, desc[:3, 5:6].copy(), np.array([1, 0, 1], np.int32), 2)
    assert 1 in empty and 2 not in empty
    with pytest.raises(OrbError):
        g.transform_batch_device(torch.zeros((1, 4097, 32), dtype=torch.uint8, device="cuda"),
                                 torch.zeros(1, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("variant", VC.VARIANTS)
def test_loader_variants(oracle, tmp_path, variant):
    p = tmp_path / f"{variant}.txt"
    voc, X, levelsup = VC.write_variant(variant, p)
    g, o = ORBVocabulary.loadFromTextFile(p), oracle.Vocabulary(path=p)
    assert g.info() == o.info() == oracle.Vocabulary(voc).info()
    _same(g.transform(X, levelsup), o.transform(X, levelsup))
    _same(g.transform(voc["desc"][1:], 0), oracle.Vocabulary(voc).transform(voc["desc"][1:], 0))   # every node's own descriptor


def test_loader_rejects(tmp_path):
    texts = VC.malformed_texts()
    assert len(texts) == 10
    for name, text in texts.items():
        p = tmp_path / f"{name}.txt"
        p.write_text(text)
        with pytest.raises(OrbError):
            ORBVocabulary.loadFromTextFile(p)
    with pytest.raises(OrbError):
        ORBVocabulary.loadFromTextFile(tmp_path / "missing.txt")
    voc = make_vocabulary(34, k=3, L=2)
    for node, par in ((5, len(voc["parent"])), (5, -1), (5, 5)):
        bad = dict(voc, parent=voc["parent"].copy())
        bad["parent"][node] = par
        with pytest.raises(OrbError):
            _handle(bad)
    bad = dict(voc, parent=voc["parent"].copy())
    bad["parent"][[5, 6]] = [6, 5]
    with pytest.raises(OrbError):
        _handle(bad)
    ok = tmp_path / "ok.txt"
    ok.write_text(VC.wellformed_text())   # what each text above spoils in one place
    assert ORBVocabulary.loadFromTextFile(ok).info() == dict(k=4, L=3, n_nodes=4, n_words=3, scoring=0, weighting=0)


@pytest.mark.parametrize("lanes", ["4", "16"])
def test_orbv_lanes(oracle, tmp_path, lanes):
    """ORBV_LANES = 4 / 16 (voc_descend_kernel<4> / <16>) on the fanout8 case, in a child process because the library reads
    the variable once.  Nothing observable proves that the lane count took effect: the results are the same by design, so
    this only shows that a process started with the variable set computes what the oracle does."""
    out = tmp_path / f"lanes{lanes}.npz"
    child = Path(__file__).with_name("vocabulary_lanes_child.py")
    r = subprocess.run([sys.executable, str(child), str(out)], env={**os.environ, "ORBV_LANES": lanes}, timeout=120,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    z = np.load(out)
    voc, X, levelsup = VC.case("fanout8_lu1")
    _same(((z["bow_word"], z["bow_weight"]), (z["fv_node"], z["fv_off"], z["fv_idx"])),
          oracle.Vocabulary(voc).transform(X, levelsup))
