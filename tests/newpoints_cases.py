"""The batches of tests/test_newpoints_gpu.py and the conditions under which the device may be compared with
tests/newpoints_ref.py, both computed here so that the CPU suite can check them (tests/test_newpoints_conditions.py).

A decision within rounding of its gate may legitimately differ between the device and numpy (cosf / atan2f, the fp64
Jacobi against numpy.linalg).  So, measured on the restatement alone, with every entry of A and the stereo cosines moved
one float ulp (newpoints_ref.jitter_effect, the largest figure over JITTER_SEEDS and over every batch, given matches and
every round of both loops):
    MARGIN = 16 x the largest change of any gated value relative to its scale: one bound for every kind of gate
    TOL    = 16 x the largest relative change of Xw, the normal and the distances
and the seeds and geometry of the batches are chosen such that no gate of any match lies within MARGIN of its threshold.
`python tests/newpoints_cases.py` prints the figures."""
import functools
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))   # (run as a program)

import newpoints_ref as R
from orb_slam2_refactored_amd.synth import make_new_points_batch

JITTER_SEEDS = tuple(range(8))
# neighbours 1.6 to 2.6 away, mostly sideways: every pair of rays is several degrees apart, far from the 0.9998 gate
GEOMETRY = dict(baseline=(1.6, 2.6), along=(1.0, 0.4, 0.05))


def cases():
    """name -> host batch.  cap 65 and 130 (no multiple of 64) and 300 (more than one tile of 256 lanes, in the
    triangulation and in the median's rank count), counts 0, 1, 64, 65, 257 and cap, P = 1, 2 and 13, all-mono,
    all-stereo and mixed uright, K1 != K2 throughout (the generator's cameras differ per keyframe)."""
    c13 = np.full(26, 130, np.int32)
    c13[[1, 14]] = 0       # an empty keyframe 1, an empty keyframe 2 (of pair 1)
    c13[[2, 16]] = 1
    c13[[3, 17]] = 64
    c13[[4, 18]] = 65
    return dict(mono_p1=make_new_points_batch(11, n_kf1=1, n_rounds=1, cap=65, mode="mono", short_frac=0.0, **GEOMETRY),
                mixed_p13=make_new_points_batch(72, n_kf1=13, n_rounds=1, cap=130, mode="mixed", counts=c13, short_frac=0.4, **GEOMETRY),
                mono_tiles=make_new_points_batch(15, n_kf1=2, n_rounds=1, cap=300, mode="mono", counts=[300, 257, 300, 290],
                                                 short_frac=0.0, mp_frac=0.9, **GEOMETRY),
                stereo_loop=make_new_points_batch(13, n_kf1=2, n_rounds=3, cap=65, mode="stereo", short_frac=0.0, **GEOMETRY),
                mono_loop=make_new_points_batch(14, n_kf1=2, n_rounds=3, cap=130, mode="mono", short_frac=0.0, **GEOMETRY))


GIVEN = ("mono_p1", "mixed_p13", "mono_tiles", "stereo_loop")
LOOPS = ("stereo_loop", "mono_loop")


def flat(b):
    """The plan as one call's pairs."""
    return dict(b, frame1=b["frame1"].reshape(-1), frame2=b["frame2"].reshape(-1))


def nearest_matches(b, pairs):
    """A match12 without the search: the keypoint of keyframe 2 with the nearest descriptor, where it is below 50; pair
    0 of a batch of more than two gets no match at all."""
    P, cap = len(pairs["frame1"]), b["kps1"].shape[1]
    m = np.full((P, cap), -1, np.int32)
    for p in range(P):
        a, c = pairs["frame1"][p], pairs["frame2"][p]
        n1, n2 = b["counts1"][a], b["counts2"][c]
        if n2 == 0 or (P > 2 and p == 0):
            continue
        for i in range(n1):
            d = np.unpackbits(b["desc"][c, :n2] ^ b["desc"][a, i], axis=1).sum(1)
            if d.min() < 50:
                m[p, i] = int(np.argmin(d))
    return m


def oracle_search(O, b):
    """search(round pairs, flags1, flags2) for newpoints_ref.loop: the oracle's SearchForTriangulation per pair."""
    import tri_case

    def search(pr, flags1, flags2):
        P, cap = len(pr["frame1"]), b["kps1"].shape[1]
        out = np.full((P, cap), -1, np.int32)
        for p in range(P):
            if pr["skip"][p] == 2:
                continue
            kf = []
            for f, flags, s in ((pr["frame1"][p], flags1, "1"), (pr["frame2"][p], flags2, "2")):
                n = int(b["counts" + s][f])
                k = b["kps" + s][f, :n]
                ur = b.get("uright" + s)
                kf.append(dict(xy=np.stack([k["x"], k["y"]], 1).astype(np.float32), octave=k["octave"].astype(np.int32),
                               uright=np.full(n, -1, np.float32) if ur is None else ur[f, :n], has_mappoint=flags[f, :n].copy(),
                               desc=b["desc"][f, :n],
                               fv=(np.array([0], np.uint32), np.array([0, n], np.int32), np.arange(n, dtype=np.int32))))
            if len(kf[0]["xy"]) == 0 or len(kf[1]["xy"]) == 0:
                continue
            kf[1].update(scale_factors=b["scale_factors2"], sigma2=b["sigma2_2"], ep2=pr["ep2"][p])
            m12, _ = tri_case.oracle_run(O, kf[0], kf[1], pr["F12"][p].reshape(3, 3))
            out[p, :len(m12)] = m12
        return out
    return search


@functools.lru_cache(maxsize=1)
def _reference(O):
    """Everything the restatement says about the batches: per batch the given-match result and the loop's rounds."""
    out = {}
    for name, b in cases().items():
        e = dict(batch=b)
        if name in GIVEN:
            fb = flat(b)
            e["pairs"] = R.prepare(fb)
            e["m12"] = nearest_matches(fb, e["pairs"])
            e["given"] = R.triangulate(fb, e["pairs"], e["m12"])
        if name in LOOPS:
            search = oracle_search(O, b)
            flags = b["has_mappoint"].copy()
            e["loop_pairs"], e["rounds"], e["matches"] = R.loop(b, search, flags, flags)
            e["flags"] = flags
            frozen = b["has_mappoint"].copy()
            e["matches_frozen"] = R.loop(b, search, frozen, frozen, update_flags=False)[2]
        out[name] = e
    return out


def reference(O):
    return _reference(O)


@functools.lru_cache(maxsize=1)
def _conditions(O):
    ref = reference(O)
    spread, jitter, smallest = 0.0, {}, {}
    for name, e in ref.items():
        b = e["batch"]
        calls = []
        if "given" in e:
            calls.append((flat(b), e["pairs"], e["m12"], e["given"]))
        if "rounds" in e:
            P = b["frame1"].shape[1]
            for r, res in enumerate(e["rounds"]):
                calls.append((b, {k: v[r * P:(r + 1) * P] for k, v in e["loop_pairs"].items()}, e["matches"][r], res))
        for fb, pr, m12, res in calls:
            for g in res["gates"].values():
                R.margins(g, smallest)
            for seed in JITTER_SEEDS:
                s, gj = R.jitter_effect(fb, pr, m12, seed)
                spread = max(spread, s)
                for k, v in gj.items():
                    jitter[k] = max(jitter.get(k, 0.0), v)
    return dict(spread=spread, gate_jitter=jitter, smallest_margin=smallest, MARGIN=16 * max(jitter.values()), TOL=16 * spread)


def conditions(O):
    """dict(spread, gate_jitter per kind, smallest_margin per kind, MARGIN, TOL)."""
    return _conditions(O)


if __name__ == "__main__":
    import oracle_api
    oracle_api.lib()
    c = conditions(oracle_api)
    print("spread", c["spread"], "TOL", c["TOL"], "MARGIN", c["MARGIN"])
    for k in sorted(c["smallest_margin"]):
        print(f"{k:14s} jitter {c['gate_jitter'].get(k, 0.0):.3g}  smallest margin {c['smallest_margin'][k]:.3g}")
    for name, e in reference(oracle_api).items():
        if "given" in e:
            print(name, "given: statuses", np.bincount(e["given"]["status"][e["m12"] >= 0].ravel(), minlength=11).tolist(), "skip", e["pairs"]["skip"].tolist())
        if "rounds" in e:
            print(name, "loop: created", [r["n_created"].tolist() for r in e["rounds"]], "round 1 differs from frozen",
                  not np.array_equal(e["matches"][1], e["matches_frozen"][1]))
