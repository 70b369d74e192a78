"""tests/stereo_ref.py against the oracle on the branch-targeted scenes of tests/stereo_cases.py, and the scenes' coverage
witnesses: each scene names the reason codes and boundary facts it exists for, and the restatement's trace must show every
one of them.  A scene that stops reaching its branch fails here, without a GPU.  CPU only."""
import numpy as np
import pytest

import stereo_cases as SC
import stereo_ref as SR

SCENES = SC.all_scenes()
IDS = [s.name for _, s in SCENES]


@pytest.mark.parametrize("case,scene", SCENES, ids=IDS)
def test_reference_equals_oracle_bit_for_bit(oracle, case, scene):
    r = SC.reference(scene.name)
    eu, ed = oracle.compute_stereo_matches(*scene.args())
    assert np.array_equal(r["uright"].view(np.int32), eu.view(np.int32))
    assert np.array_equal(r["depth"].view(np.int32), ed.view(np.int32))
    assert np.all((eu == -1) == (ed == -1))


@pytest.mark.parametrize("case,scene", SCENES, ids=IDS)
def test_scene_reaches_what_it_exists_for(case, scene):
    r = SC.reference(scene.name)
    assert scene.witnesses
    missed = [label for label, pred in scene.witnesses if not pred(r)]
    assert not missed, missed
    # the trace agrees with the outputs
    t = r["trace"]
    kept = np.isin(t["reason"], (SR.MATCH, SR.MATCH_EPS))
    assert np.array_equal(kept, r["depth"] > 0) and np.array_equal(kept, r["uright"] != -1)
    assert r["n_matched"] == t["matched"].sum() == (kept | (t["reason"] == SR.FILTERED)).sum()


@pytest.mark.parametrize("case", list(SC.CASES))
def test_case_witnesses_its_reason_codes(case):
    seen = set()
    for s in SC.all_cases()[case]:
        seen |= set(SC.reference(s.name)["trace"]["reason"].tolist())
    assert SC.CASE_REASONS[case] <= seen, [SR.REASONS[c] for c in SC.CASE_REASONS[case] - seen]


def test_every_reason_code_appears():
    seen = set()
    for _, s in SCENES:
        seen |= set(SC.reference(s.name)["trace"]["reason"].tolist())
    assert seen == set(range(len(SR.REASONS))), [SR.REASONS[c] for c in set(range(len(SR.REASONS))) - seen]


def test_hamming_tie_orders_give_different_outputs():
    """The same scene with the right keypoints reversed: the other tied candidate wins, at another x."""
    fwd, rev = (SC.reference(s.name) for s in SC.all_cases()["hamming_tie"])
    assert np.all(fwd["depth"] > 0) and np.all(rev["depth"] > 0)
    assert np.all(np.abs(fwd["uright"] - rev["uright"]) > 10)


def test_contract_check_refuses_what_the_reference_cannot_read():
    s = SC.Scene("out_of_contract", 0, 40)
    i = s.left(30, 8.5)
    s.right(9, 8.5, 0, SC.flip(s._dl[i], 10))     # suR == 9: the window would start at column -1
    with pytest.raises(AssertionError, match="suR < 10"):
        s.finish()
    s = SC.Scene("out_of_contract", 0, 40)
    i = s.left(30, 4.25)                          # svL == 4: the patch would start at row -1
    s.right(20, 4.25, 0, SC.flip(s._dl[i], 10))
    with pytest.raises(AssertionError, match="left patch"):
        s.finish()
    s.kl, s.kr = np.array(s._kl, SC.KP_DTYPE), np.array(s._kr, SC.KP_DTYPE)
    s.dl, s.dr = np.array(s._dl, np.uint8), np.array(s._dr, np.uint8)
    with pytest.raises(IndexError):
        SR.compute(*s.args())


def test_reference_on_empty_sides():
    s = SC.all_cases()["disparity"][0]
    r = SR.compute(s.kl, s.dl, s.pl, s.kr[:0], s.dr[:0], s.pr, SC.SCALE, SC.INV_SCALE, s.bf, s.baseline)
    assert np.all(r["trace"]["reason"] == SR.NO_CAND) and np.all(r["uright"] == -1) and r["n_matched"] == 0
    r = SR.compute(s.kl[:0], s.dl[:0], s.pl, s.kr, s.dr, s.pr, SC.SCALE, SC.INV_SCALE, s.bf, s.baseline)
    assert len(r["uright"]) == 0 and r["median"] == -1
