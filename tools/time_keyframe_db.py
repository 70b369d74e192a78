"""Device time of the KeyFrameDatabase queries (orbdb_*) on the generator's places: torch CUDA events, the median of
`--launches` launches after `--warmup`.  Per batch size Q: the common-word pass alone (a loop query whose connected set
names every slot: nothing is scored, no group opens), a relocalisation batch, a loop batch (MinScore + the query), and
once `add` of every keyframe.  One JSON line.  There is no earlier device path for these calls: the numbers stand alone.

    python tools/time_keyframe_db.py [--keyframes 4096] [--words 1000] [--queries 1,64] [--launches 20] [--warmup 3]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))
from orb_slam2_refactored_amd.keyframe_db import KeyFrameDatabase  # noqa: E402
from orb_slam2_refactored_amd.synth import make_keyframe_db_case, make_vocabulary  # noqa: E402
from orb_slam2_refactored_amd.vocabulary import ORBVocabulary  # noqa: E402


def timed(fn, launches, warmup):
    ms = []
    for i in range(warmup + launches):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        if i >= warmup:
            ms.append(e0.elapsed_time(e1))
    return {"median": round(statistics.median(ms), 3), "min": round(min(ms), 3), "max": round(max(ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keyframes", type=int, default=4096)
    ap.add_argument("--words", type=int, default=1000)
    ap.add_argument("--queries", default="1,64")
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    K, W = a.keyframes, a.words
    Qs = [int(x) for x in a.queries.split(",")]
    c = make_keyframe_db_case(0, max_keyframes=K, n_add=K, n_erased=0, word_cap=W, n_places=max(K // 16, 2), n_queries=max(Qs),
                              vocab=max(100 * W, 100000))
    v = make_vocabulary(0, k=4, L=2)
    voc = ORBVocabulary.from_arrays(v["k"], v["L"], v["scoring"], v["weighting"], v["parent"], v["is_leaf"], v["desc"], v["weight"])
    db = KeyFrameDatabase(voc, K, W)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32) if x.dtype == np.uint32 else np.ascontiguousarray(x)).cuda()  # noqa: E731
    slot, bw, bv, nw = dev(c["slot"]), dev(c["bow_word"]), dev(c["bow_weight"]), dev(c["n_words"])
    res = {"keyframes": K, "words": W, "mean_words": round(float(c["n_words"].mean()), 1),
           "add_ms": timed(lambda: db.add_device(slot, bw, bv, nw), a.launches, a.warmup)}
    qw, qv, qn, covis = dev(c["q_bow_word"]), dev(c["q_bow_weight"]), dev(c["q_n_words"]), dev(c["covis"])
    every = torch.arange(K, dtype=torch.int32).cuda()
    for Q in Qs:
        q = dict(bow_word=qw, bow_weight=qv, n_words=qn, frame=dev(c["q_frame"][:Q]), covis=covis,
                 conn_off=dev(c["conn_off"][:Q + 1]), conn_idx=dev(c["conn_idx"]))
        cov_off, cov_idx = dev(c["cov_off"][:Q + 1]), dev(c["cov_idx"])
        none = dict(q, conn_off=(torch.arange(Q + 1, dtype=torch.int32) * K).cuda(), conn_idx=every.repeat(Q))
        one = torch.ones(Q, dtype=torch.float32).cuda()
        out = db.detect_relocalization_candidates_device(q, extras=False)
        ms = db.min_score_device(q, cov_off, cov_idx)
        lout = db.detect_loop_candidates_device(q, ms, extras=False)
        torch.cuda.synchronize()

        def loop():
            db.min_score_device(q, cov_off, cov_idx, out=ms)
            db.detect_loop_candidates_device(q, ms, out=lout)

        res[f"Q{Q}"] = {
            "reloc_candidates": int(out["n_cand"].sum()), "loop_candidates": int(lout["n_cand"].sum()),
            "words_ms": timed(lambda: db.detect_loop_candidates_device(none, one, out=lout), a.launches, a.warmup),
            "reloc_ms": timed(lambda: db.detect_relocalization_candidates_device(q, out=out), a.launches, a.warmup),
            "loop_ms": timed(loop, a.launches, a.warmup)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
