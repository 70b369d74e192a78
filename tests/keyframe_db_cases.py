"""The KeyFrameDatabase cases the CPU, native and GPU tests share, and their results from tests/keyframe_db_ref.py, computed
once per process.  The shapes are the smallest at which the kernels can go wrong: 70 slots (more than one wavefront of them,
no multiple of a workgroup's 16), 65 live after three erasures, vectors of 0, 1, 63, 64, 65 and 200 words at word_cap 200
(below, at and above one wavefront's 64 lookups; a full row), up to five queries."""
import functools

import numpy as np

import keyframe_db_ref as R
from orb_slam2_refactored_amd.synth import make_keyframe_db_case

EDGE_COUNTS = [0, 1, 63, 64, 65, 200]


def _counts(seed, n=68):
    rng = np.random.default_rng(100 + seed)
    c = rng.integers(60, 201, n)
    c[rng.random(n) < 0.5] = rng.integers(170, 201)
    c[rng.permutation(n)[:len(EDGE_COUNTS)]] = EDGE_COUNTS
    return c


CASES = {
    "mixed": dict(seed=1, counts=_counts(1), q_counts=[200, 190, 65, 180, 200]),
    "edges": dict(seed=2, counts=_counts(2), q_counts=[64, 0, 1, 63, 200]),
    "plain": dict(seed=3),
}


@functools.lru_cache(maxsize=None)
def case(name):
    return make_keyframe_db_case(**CASES[name])


@functools.lru_cache(maxsize=None)
def reference(name, kind, Q=None):
    """The first Q queries (None: all) as one batch on a freshly filled database."""
    c = case(name)
    return R.run_case(c, kind, queries=range(c["n_queries"] if Q is None else Q))


def query(c, Q=None):
    Q = c["n_queries"] if Q is None else Q
    return dict(bow_word=c["q_bow_word"], bow_weight=c["q_bow_weight"], n_words=c["q_n_words"], frame=c["q_frame"][:Q],
                covis=c["covis"], conn_off=c["conn_off"][:Q + 1], conn_idx=c["conn_idx"], cov_off=c["cov_off"][:Q + 1],
                cov_idx=c["cov_idx"])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint64) if a.dtype == np.float64 else a
