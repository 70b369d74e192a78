"""Child process of tests/test_vocabulary_gpu.py::test_orbv_lanes: csrc/orbv.hip reads ORBV_LANES once per process, so each value
needs a process of its own.  Transforms the fanout8 case (tests/vocabulary_cases.py) through the C-ABI and saves the five
result arrays to the .npz path given as the only argument; the parent compares them with the oracle.  numpy and ctypes only."""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import numpy as np  # noqa: E402

import vocabulary_cases as VC  # noqa: E402
from orb_slam2_refactored_amd.vocabulary import ORBVocabulary  # noqa: E402

CASE = "fanout8_lu1"


def main(out):
    voc, X, levelsup = VC.case(CASE)
    g = ORBVocabulary.from_arrays(voc["k"], voc["L"], voc["scoring"], voc["weighting"], voc["parent"], voc["is_leaf"],
                                  voc["desc"], voc["weight"])
    (bw, bv), (fn, fo, fi) = g.transform(X, levelsup)
    assert "torch" not in sys.modules
    np.savez(out, bow_word=bw, bow_weight=bv, fv_node=fn, fv_off=fo, fv_idx=fi)


if __name__ == "__main__":
    main(sys.argv[1])
