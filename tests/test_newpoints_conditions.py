"""The conditions of tests/test_newpoints_gpu.py, asserted on the CPU (tests/newpoints_cases.py): in the restatement no
gate of any match of any batch, given matches and every round of both loops, lies within MARGIN of its threshold, the
batches reach what they are meant to reach, and the loop without the flag update differs from round 1 on."""
import numpy as np

import newpoints_cases as C
import newpoints_ref as R


def test_no_gate_lies_within_margin(oracle):
    c = C.conditions(oracle)
    print("spread", c["spread"], "TOL", c["TOL"], "MARGIN", c["MARGIN"], "gate jitter", c["gate_jitter"], "smallest margins",
          c["smallest_margin"])
    assert c["MARGIN"] == 16 * max(c["gate_jitter"].values()) and c["TOL"] == 16 * c["spread"] > 0
    assert min(c["smallest_margin"].values()) >= c["MARGIN"], "choose another seed, never another margin"
    # the jitter of the restatement bounds what the platform's cosf / atan2f may differ by: an ulp or two of a cosine
    assert c["MARGIN"] >= 16 * 2.0 ** -23


def test_batches_reach_what_they_are_for(oracle):
    ref = C.reference(oracle)
    S = R.STATUS
    seen = set()
    for name in C.GIVEN:
        e = ref[name]
        seen |= set(np.unique(e["given"]["status"][e["m12"] >= 0]).tolist())
    assert {S["created"], S["pair_skipped"], S["reproj1"], S["reproj2"]} <= seen
    t = ref["mono_tiles"]
    assert (t["given"]["new_idx1"][0] >= 256).sum() > 0 and t["batch"]["counts1"].max() > 256
    assert 0 < ref["mixed_p13"]["pairs"]["skip"].sum() < 13 and (ref["mixed_p13"]["m12"][0] < 0).all()
    for name in C.LOOPS:
        e = ref[name]
        assert e["rounds"][0]["n_created"].sum() > 0
        assert not np.array_equal(e["matches"][1], e["matches_frozen"][1]), "round 0's points must change round 1's search"
        assert e["rounds"][1]["n_created"].sum() > 0
