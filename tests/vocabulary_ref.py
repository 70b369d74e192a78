"""Plain numpy restatement of DBoW2's transform (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1130-1263, BowVector.cpp:34-84,
FeatureVector.cpp:31-45) on a vocabulary given as arrays (synth.make_vocabulary's dict), independent of oracle/orb_oracle.cpp
and of csrc/orbv.hip: Python dicts for the two maps, Python floats (IEEE doubles, one rounding per operation) for the weights.

first_min=False takes the LAST closest child instead of the first.  It is wrong on purpose: tests/test_vocabulary_oracle.py
uses it only to show that the planted ties of tests/vocabulary_cases.py tell the two rules apart."""
import numpy as np


def children_of(voc):
    """Per node the list of its children in file order (the reference's push_back order)."""
    parent = voc["parent"]
    children = [[] for _ in range(len(parent))]
    for i in range(1, len(parent)):
        children[parent[i]].append(i)
    return children


def word_ids(voc):
    """Per node its word id: the running count of leaf-flagged nodes in file order, 0 (Node's default) elsewhere."""
    leaf = np.asarray(voc["is_leaf"])
    word = np.zeros(len(leaf), np.int64)
    word[np.nonzero(leaf)[0]] = np.arange(int(leaf.astype(bool).sum()))
    return word


def descend(voc, X, first_min=True):
    """Per descriptor the list of nodes below the root that the descent visits, ending at a childless node."""
    children = children_of(voc)
    bitsD = np.unpackbits(np.asarray(voc["desc"], np.uint8), axis=1)
    paths = []
    for x in np.unpackbits(np.asarray(X, np.uint8).reshape(-1, 32), axis=1):
        node, path = 0, []
        while children[node]:
            ch = children[node]
            d = (bitsD[ch] != x).sum(axis=1)
            best = np.nonzero(d == d.min())[0]
            node = ch[int(best[0] if first_min else best[-1])]
            path.append(node)
        paths.append(path)
    return paths


def np_transform(voc, X, levelsup, first_min=True):
    """((word ids, weights) ascending, (node ids, offsets, feature indices)) as oracle_api.Vocabulary.transform returns."""
    leaf, W = np.asarray(voc["is_leaf"]), voc["weight"]
    word = word_ids(voc)
    nid_level = voc["L"] - levelsup
    bow, fv = {}, {}
    tf = voc["weighting"] in (0, 1)
    paths = descend(voc, X, first_min) if leaf.any() else []   # empty(): no words, both vectors stay empty (:1137-1140)
    for i, path in enumerate(paths):
        node = path[-1] if path else 0
        nid = 0 if nid_level <= 0 else (path[nid_level - 1] if nid_level <= len(path) else node)
        w = float(W[node])
        if w > 0:
            wid = int(word[node])
            if tf:
                bow[wid] = bow[wid] + w if wid in bow else w
            elif wid not in bow:
                bow[wid] = w
            fv.setdefault(nid, []).append(i)
    keys = sorted(bow)
    vals = [bow[k] for k in keys]
    sc = voc["scoring"]
    if sc != 5:
        norm = 0.0
        if sc == 1:
            for v in vals:
                norm += v * v
            norm = float(np.sqrt(norm))
        else:
            for v in vals:
                norm += abs(v)
        if norm > 0:
            vals = [v / norm for v in vals]
    elif tf and vals:
        vals = [v / float(len(vals)) for v in vals]
    nodes = sorted(fv)
    off = np.concatenate([[0], np.cumsum([len(fv[k]) for k in nodes])]).astype(np.int32)
    idx = np.array([i for k in nodes for i in fv[k]], np.int32)
    return (np.array(keys, np.uint32), np.array(vals, np.float64)), (np.array(nodes, np.uint32), off, idx)
