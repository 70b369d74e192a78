"""Hand-built vocabularies and planted feature sets for the DBoW2 transform (tests/test_vocabulary_oracle.py on the CPU,
tests/test_vocabulary_gpu.py and tests/vocabulary_lanes_child.py on the device): one named case per branch group of
csrc/orbv.hip that synth.make_vocabulary's even k-ary trees never reach.

case(name) returns a Case: it unpacks as (voc, X, levelsup), voc being make_vocabulary's dict, and carries the facts its plants
exist for, which the CPU tests assert against the oracle and the numpy restatement so that no case passes vacuously:
  ties     (feature index, first tied sibling, other tied sibling): the feature is at the same distance from both siblings
           (both leaf-flagged, with different words) and farther from every other child of their parent
  fanouts  child counts that at least one feature has to descend through
  alias    the features that land on word id 0 through two different nodes, in feature order
A descriptor "near" another is that one with some bits flipped, so distances follow the tree as in synth.make_vocabulary.
Weights carry at most 6 significant digits, so the text form (ostream << double) reads back as the same doubles.

Cases are built once per process (lru_cache); treat them as read-only."""
import functools

import numpy as np

from orb_slam2_refactored_amd.synth import make_vocabulary, vocabulary_features


def flip(d, bits):
    """d with the given bit indices flipped: Hamming distance len(set(bits)) exactly."""
    x = np.array(d, np.uint8)
    for b in bits:
        x[b >> 3] ^= np.uint8(1 << (b & 7))
    return x


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


class Tree:
    """Nodes in file order (a parent before its children); node 0 is the root."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.parent, self.flag, self.desc, self.weight = [0], [0], [np.zeros(32, np.uint8)], [0.0]

    def near(self, d, lo=16, hi=48):
        return flip(d, self.rng.choice(256, size=int(self.rng.integers(lo, hi + 1)), replace=False))

    def add(self, p, leaf, weight=None, desc=None, flips=(16, 48)):
        """A child of p: random under the root, else near p's descriptor; a leaf-flagged node gets a word and, unless given,
        a weight in (0.5, 8) of 6 significant digits; an inner node weight 0."""
        if desc is None:
            desc = self.rng.integers(0, 256, 32, dtype=np.uint8) if p == 0 else self.near(self.desc[p], *flips)
        if weight is None:
            weight = float(f"{self.rng.uniform(0.5, 8.0):g}") if leaf else 0.0
        self.parent.append(p)
        self.flag.append(1 if leaf else 0)
        self.desc.append(np.array(desc, np.uint8))
        self.weight.append(float(weight))
        return len(self.parent) - 1

    def voc(self, k, L, scoring=0, weighting=0):
        return dict(k=k, L=L, scoring=scoring, weighting=weighting, parent=np.array(self.parent, np.int32),
                    is_leaf=np.array(self.flag, np.uint8), desc=np.stack(self.desc).astype(np.uint8),
                    weight=np.array(self.weight, np.float64))


class Case:
    def __init__(self, voc, X, levelsup, ties=(), fanouts=(), alias=None):
        self.voc, self.X, self.levelsup = voc, np.ascontiguousarray(X, np.uint8).reshape(-1, 32), levelsup
        self.ties, self.fanouts, self.alias = tuple(ties), tuple(fanouts), alias
        self.X.setflags(write=False)

    def __iter__(self):
        return iter((self.voc, self.X, self.levelsup))


def max_children(voc):
    return int(np.bincount(voc["parent"][1:], minlength=1).max()) if len(voc["parent"]) > 1 else 0


class _Plants:
    """Collects the planted features of one tree and the tie records that go with them."""

    def __init__(self, t):
        self.t, self.X, self.ties = t, [], []

    def query(self, d):
        self.X.append(np.array(d, np.uint8))
        return len(self.X) - 1

    def identical(self, kids, a, b):
        """Children a < b of one parent get the same descriptor; a feature equal to it: distance 0 to both."""
        self.t.desc[kids[b]] = self.t.desc[kids[a]].copy()
        self.ties.append((self.query(self.t.desc[kids[a]]), kids[a], kids[b]))

    def equidistant(self, kids, a, b, base):
        """Children a < b become base with bits 0..4 / 5..9 flipped: different descriptors, both at distance 5 from the
        feature `base`; every other child of the parent has to be farther (checked here)."""
        self.t.desc[kids[a]] = flip(base, range(0, 5))
        self.t.desc[kids[b]] = flip(base, range(5, 10))
        assert all(hamming(base, self.t.desc[c]) > 5 for i, c in enumerate(kids) if i not in (a, b))
        self.ties.append((self.query(base), kids[a], kids[b]))

    def complement_only_child(self, p):
        """p's only child becomes the complement of a descriptor 3 bits from p's: that descriptor as a feature reaches p
        and is at distance 256, the largest there is, from the child it has to take."""
        q = self.t.near(self.t.desc[p], 3, 3)
        c = self.t.add(p, leaf=True, desc=np.bitwise_not(q))
        self.query(q)
        return c


def _finish(t, pl, k, L, levelsup, seed, n_random, fanouts):
    voc = t.voc(k, L)
    X = np.concatenate([np.stack(pl.X), vocabulary_features(voc, seed, n_random)])
    return Case(voc, X, levelsup, ties=pl.ties, fanouts=fanouts)


def _fanout8(levelsup):
    """At most 16 children anywhere (voc_descend_kernel<8>, <4> or <16>): the root has 16, its first six children 1, 7, 8, 9, 15
    and 16, leaves sit at depths 1, 2 and 3 (= L) and one chain goes on to depth 5.  Tied leaves: in the 16 at (0, 15), (7, 8)
    and (3, 11) identical and (6, 14) equidistant; in the 15 at (0, 14), (3, 4) and (1, 5) identical (the pass boundary and
    the same lane twice for 8 lanes and for 4)."""
    t = Tree(801)
    pl = _Plants(t)
    fan = [1, 7, 8, 9, 15, 16, 0, 2] + [0] * 8
    top = [t.add(0, leaf=f == 0) for f in fan]
    pl.complement_only_child(top[0])
    k7 = [t.add(top[1], leaf=i != 0) for i in range(7)]
    for _ in range(3):
        t.add(k7[0], leaf=True)                       # depth 3 = L
    k8 = [t.add(top[2], leaf=True) for _ in range(8)]
    k9 = [t.add(top[3], leaf=True) for _ in range(9)]
    k15 = [t.add(top[4], leaf=True) for _ in range(15)]
    k16 = [t.add(top[5], leaf=True) for _ in range(16)]
    k2 = [t.add(top[7], leaf=i != 0) for i in range(2)]
    d3 = [t.add(k2[0], leaf=i != 0) for i in range(2)]
    d4 = t.add(d3[0], leaf=False)
    t.add(d4, leaf=True)                              # depth 5 > L
    pl.identical(k16, 0, 15)
    pl.identical(k16, 7, 8)
    pl.identical(k16, 3, 11)
    pl.equidistant(k16, 6, 14, t.near(t.desc[top[5]]))
    pl.identical(k15, 0, 14)
    pl.identical(k15, 3, 4)
    pl.identical(k15, 1, 5)
    pl.query(t.desc[k9[8]])                           # distance 0, the lone child of the second pass
    for kids in (k7, k8, k9):
        pl.query(t.near(t.desc[kids[-1]], 0, 4))
    return _finish(t, pl, 10, 3, levelsup, 811, 200, (1, 7, 8, 9, 15, 16))


def _fanout64():
    """More than 64 children (the two-pass loop of voc_descend_kernel<64>): the root has 70, one node exactly 64, one 65, nine
    others 1 .. 9.  Tied leaves: under the root (0, 69), (63, 64) and (3, 67) identical and (20, 66) equidistant; in the 64 at
    (0, 63) identical and (10, 40) equidistant; in the 65 at (0, 64) and (1, 63) identical."""
    t = Tree(802)
    pl = _Plants(t)
    inner = {1: 64, 2: 65, **{4 + i: 1 + i for i in range(9)}}
    top = [t.add(0, leaf=i not in inner) for i in range(70)]
    pl.complement_only_child(top[4])
    for i in range(5, 13):
        for _ in range(inner[i]):
            t.add(top[i], leaf=True)
    k64 = [t.add(top[1], leaf=i != 5) for i in range(64)]
    for _ in range(2):
        t.add(k64[5], leaf=True)                      # depth 3 = L
    k65 = [t.add(top[2], leaf=True) for _ in range(65)]
    pl.identical(top, 0, 69)
    pl.identical(top, 63, 64)
    pl.identical(top, 3, 67)
    pl.equidistant(top, 20, 66, t.rng.integers(0, 256, 32, dtype=np.uint8))
    pl.identical(k64, 0, 63)
    pl.equidistant(k64, 10, 40, t.near(t.desc[top[1]]))
    pl.identical(k65, 0, 64)
    pl.identical(k65, 1, 63)
    pl.query(t.desc[k65[30]])                         # distance 0
    for i in range(5, 13):
        pl.query(t.near(t.desc[top[i]], 0, 4))
    return _finish(t, pl, 10, 3, 1, 812, 200, (70, 64, 65) + tuple(range(1, 10)))


ALIAS_REAL, ALIAS_OTHER = 3.0, 0.712345


def _alias(scoring, weighting, first):
    """Word id 0 reached through two nodes: node 1 is the real word 0 (weight 3.0), node 2 is childless but flagged "not a
    leaf" in the file, so it keeps Node's default word_id = 0 with its own weight 0.712345 > 0.  The features land on both in
    turn; `first` says which node the first one lands on."""
    t = Tree(803)
    real = t.add(0, leaf=True, weight=ALIAS_REAL)
    other = t.add(0, leaf=False, weight=ALIAS_OTHER)
    w1 = t.add(0, leaf=True, weight=1.7)
    w2 = t.add(0, leaf=True, weight=0.45)
    order = [real, other, real, w1, other, w2, real]
    if first == "other":
        order = [other] + order
    X = [t.near(t.desc[i], 0, 4) for i in order]
    return Case(t.voc(4, 1, scoring, weighting), X, 0, alias=[int(i) for i in order if i in (real, other)])


ONE_WORD_WEIGHT = 0.1


def _one_word(n):
    """Every feature on one word of weight 0.1 (no finite binary expansion): an n-long sequential sum.  TF-IDF without
    normalisation (DOT_PRODUCT divides by the number of words, 1), so the sum itself is the result."""
    t = Tree(804)
    a = t.add(0, leaf=True, weight=ONE_WORD_WEIGHT)
    t.add(0, leaf=True, weight=2.5)
    return Case(t.voc(2, 1, 5, 0), [t.near(t.desc[a], 0, 6) for _ in range(n)], 0)


def _all_distinct():
    """343 leaves of a 7-ary tree, each the word of exactly one feature (its own descriptor), in shuffled order: U == n."""
    t = Tree(805)
    leaves = []
    for _ in range(7):
        a = t.add(0, leaf=False)
        for _ in range(7):
            b = t.add(a, leaf=False, flips=(20, 20))
            leaves += [t.add(b, leaf=True, flips=(6, 6)) for _ in range(7)]
    X = np.stack([t.desc[i] for i in leaves])[t.rng.permutation(len(leaves))]
    return Case(t.voc(7, 3), X, 1)


def _all_stopped():
    voc = make_vocabulary(9, k=4, L=3, stop_frac=1.0)
    return Case(voc, vocabulary_features(voc, 1, 100), 1)


def _root_only():
    voc = dict(k=10, L=4, scoring=0, weighting=0, parent=np.zeros(1, np.int32), is_leaf=np.zeros(1, np.uint8),
               desc=np.zeros((1, 32), np.uint8), weight=np.zeros(1))
    return Case(voc, np.random.default_rng(806).integers(0, 256, (5, 32), dtype=np.uint8), 4)


def _no_words():
    """Nodes with weights but not one leaf flag: empty() holds, as for the root alone, and both vectors stay empty."""
    t = Tree(807)
    for _ in range(3):
        t.add(0, leaf=False, weight=1.5)
    return Case(t.voc(3, 1), [t.near(t.desc[1 + i % 3], 0, 4) for i in range(9)], 0)


@functools.lru_cache(maxsize=None)
def _grid_base():
    voc = make_vocabulary(31, k=5, L=3, early_leaf=0.1, stop_frac=0.05)
    X = vocabulary_features(voc, 32, 300)
    return voc, X


def _grid(scoring, weighting):
    voc, X = _grid_base()
    return Case(dict(voc, scoring=scoring, weighting=weighting), X, 1)


FANOUT8_L = 3
BUILDERS = {
    **{f"fanout8_lu{lu}": functools.partial(_fanout8, lu) for lu in range(FANOUT8_L + 2)},   # nid at the root .. below L
    "fanout64": _fanout64,
    "alias_dot": functools.partial(_alias, 5, 0, "real"),
    "alias_l1": functools.partial(_alias, 0, 0, "real"),
    "alias_tf_l2": functools.partial(_alias, 1, 1, "other"),
    "alias_idf": functools.partial(_alias, 0, 2, "other"),
    **{f"one_word_{n}": functools.partial(_one_word, n) for n in (2, 257, 4096)},
    "all_distinct": _all_distinct,
    "all_stopped": _all_stopped,
    "root_only": _root_only,
    "no_words": _no_words,
    **{f"grid_s{s}_w{w}": functools.partial(_grid, s, w) for s in range(6) for w in range(4)},
}
NAMES = tuple(BUILDERS)
TIE_NAMES = tuple(f"fanout8_lu{lu}" for lu in range(FANOUT8_L + 2)) + ("fanout64",)
ALIAS_NAMES = ("alias_dot", "alias_l1", "alias_tf_l2", "alias_idf")


@functools.lru_cache(maxsize=None)
def case(name):
    return BUILDERS[name]()


# ---- text files --------------------------------------------------------------------------------------------------------------

def write_text(voc, path, sep=" ", eol="\n", final_eol=True, blank_every=0, exponent=False):
    """saveToTextFile's layout (TemplatedVocabulary.h:1434-1450) with the separators, line ends and number form chosen."""
    lines = [sep.join(str(voc[f]) for f in ("k", "L", "scoring", "weighting"))]
    for i in range(1, len(voc["parent"])):
        w = float(voc["weight"][i])
        ws = (f"{w:.16e}" if i % 2 else f"{w:.16E}") if exponent else f"{w:g}"   # 17 digits: the same double back
        lines.append(sep.join([str(int(voc["parent"][i])), str(int(voc["is_leaf"][i]))] +
                              [str(int(b)) for b in voc["desc"][i]] + [ws]))
        if blank_every and i % blank_every == 0:
            lines.append("" if (i // blank_every) % 2 else " \t ")
    with open(path, "wb") as f:
        f.write((eol.join(lines) + (eol if final_eol else "")).encode())


VARIANTS = ("crlf", "blank_lines", "no_final_newline", "tabs", "exponent", "more_than_k")


def write_variant(name, path):
    """Writes the variant file; returns (voc, X, levelsup) of what it holds."""
    if name == "more_than_k":   # header k = 10, nodes with 15 and 16 children
        c = case("fanout8_lu1")
    else:
        voc = make_vocabulary(21, k=4, L=3, order="dfs", early_leaf=0.2)
        c = Case(voc, vocabulary_features(voc, 22, 200), 2)
    write_text(c.voc, path, **{"crlf": dict(eol="\r\n"), "blank_lines": dict(blank_every=7),
                               "no_final_newline": dict(final_eol=False), "tabs": dict(sep="\t"),
                               "exponent": dict(exponent=True), "more_than_k": {}}[name])
    return c


def _node_line(p):
    return f"{p} 1 " + " ".join(str((7 * p + j) % 256) for j in range(32)) + " 1.5\n"


def wellformed_text():
    """The file that malformed_texts() spoils in one place at a time: three leaves under the root."""
    return "4 3 0 0\n" + "".join(_node_line(p) for p in (0, 0, 0))


def malformed_texts():
    """name -> file text that csrc/orbv.hip's loader has to reject.  Not for the oracle: as the reference, it indexes m_nodes
    with the parent id unchecked."""
    body = lambda *ps: "".join(_node_line(p) for p in ps)   # noqa: E731
    ok = body(0, 0, 0)
    return {
        "k_21": "21 3 0 0\n" + ok, "k_negative": "-1 3 0 0\n" + ok, "L_0": "4 0 0 0\n" + ok, "L_11": "4 11 0 0\n" + ok,
        "scoring_6": "4 3 6 0\n" + ok, "weighting_4": "4 3 0 4\n" + ok,
        "parent_past_end": "4 3 0 0\n" + body(0, 0, 4),        # 4 nodes with the root: ids 0 .. 3
        "parent_negative": "4 3 0 0\n" + body(0, -1, 0),
        "self_parent": "4 3 0 0\n" + body(0, 2, 0),
        "parent_cycle": "4 3 0 0\n" + body(0, 3, 2),            # nodes 2 and 3 name each other: unreachable from the root
    }
