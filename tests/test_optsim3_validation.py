"""OptimizeSim3's argument checks: arrays shorter than the C-ABI reads are refused in Python, an out-of-range
match12 by the host entry before anything is copied.  CPU only: neither call reaches a device."""
import numpy as np
import pytest

from orb_slam2_refactored_amd._lib import LIB_PATH, OrbError
from orb_slam2_refactored_amd.optimizer import OptimizeSim3
from orb_slam2_refactored_amd.synth import make_optsim3_batch


@pytest.mark.parametrize("key", ["kp1_xy", "kp2_octave", "mp1_xw", "mp2_valid", "match12", "s12", "pose2", "camera1"])
def test_short_arrays_are_refused(key):
    b = make_optsim3_batch(1, n_corr=[12, 20])
    b[key] = b[key][:-1]
    with pytest.raises(ValueError, match=key):
        OptimizeSim3(b)


def test_missing_array_is_refused():
    b = make_optsim3_batch(1, n_corr=[12])
    del b["mp2_xw"]
    with pytest.raises(ValueError, match="mp2_xw"):
        OptimizeSim3(b)


@pytest.mark.skipif(not LIB_PATH.exists(), reason="library not built (run __graft_entry__.build())")
@pytest.mark.parametrize("value", [-2, 10 ** 6])
def test_out_of_range_match12_is_refused_by_the_host_entry(value):
    b = make_optsim3_batch(2, n_corr=[12, 20])
    b["match12"][5] = value
    with pytest.raises(OrbError, match="match12"):
        OptimizeSim3(b)
    b = make_optsim3_batch(2, n_corr=[12, 20])
    n2 = int(b["kp2_begin"][1])
    b["match12"][0] = n2   # one past keyframe 2 of pair 0, though inside the batch
    with pytest.raises(OrbError, match="match12"):
        OptimizeSim3(b)
