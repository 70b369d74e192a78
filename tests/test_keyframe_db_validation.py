"""Argument validation of the KeyFrameDatabase entries: ORB_EINVAL with a message from the C ABI, ValueError from the Python
wrappers.  Checks that precede any device call run here without a GPU; those that need a database handle are marked gpu."""
import ctypes as C

import numpy as np
import pytest

import keyframe_db_cases as KC
from orb_slam2_refactored_amd._lib import OrbdbQueryBatch, OrbdbResult, OrbError, lib
from orb_slam2_refactored_amd.synth import make_vocabulary


def last_error():
    return lib().orb_last_error().decode()


def test_null_handles_and_outputs_are_refused_before_any_device_call():
    L = lib()
    h = C.c_void_p()
    assert L.orbdb_create(None, 70, 200, 0, C.byref(h)) == -1 and "null" in last_error()
    b, r = OrbdbQueryBatch(), OrbdbResult()
    for rc in (L.orbdb_clear(None, None), L.orbdb_info(None, None, None), L.orbdb_read_slots(None, None, None),
               L.orbdb_add_device(None, 1, None, None, None, None, None, 1, 1, None), L.orbdb_erase_device(None, 1, None, None),
               L.orbdb_add(None, 1, None, None, None, None, None, 1, 1), L.orbdb_erase(None, 1, None),
               L.orbdb_min_score_device(None, C.byref(b), None, None, None, None), L.orbdb_min_score(None, C.byref(b), None, None, None),
               L.orbdb_detect_reloc_device(None, C.byref(b), C.byref(r), None), L.orbdb_detect_loop_device(None, C.byref(b), C.byref(r), None),
               L.orbdb_detect_reloc(None, C.byref(b), C.byref(r)), L.orbdb_detect_loop(None, C.byref(b), C.byref(r))):
        assert rc == -1 and "null database" in last_error()
    assert L.orbdb_destroy(None) == 0


def test_python_wrappers_refuse_wrong_shapes_and_dtypes():
    from orb_slam2_refactored_amd.keyframe_db import KeyFrameDatabase
    db = KeyFrameDatabase.__new__(KeyFrameDatabase)      # no handle: the wrappers refuse before they need one
    db.max_keyframes, db.word_cap, db._h = 70, 200, None
    c = KC.case("plain")
    q = KC.query(c)
    with pytest.raises(ValueError, match="slot must be int32"):
        db.add(c["slot"].astype(np.float32), c["bow_word"], c["bow_weight"], c["n_words"])
    with pytest.raises(ValueError, match="bow_weight"):
        db.add(c["slot"], c["bow_word"], c["bow_weight"].astype(np.float32), c["n_words"])
    with pytest.raises(ValueError, match="bow_word must have shape"):
        db.add(c["slot"], c["bow_word"][:-1], c["bow_weight"], c["n_words"])
    with pytest.raises(ValueError, match="covis must have shape"):
        db.DetectRelocalizationCandidates(dict(q, covis=c["covis"][:, :9]))
    with pytest.raises(ValueError, match="covis is required"):
        db.DetectRelocalizationCandidates(dict(q, covis=None))
    with pytest.raises(ValueError, match="conn_off must have shape"):
        db.DetectLoopCandidates(dict(q, conn_off=c["conn_off"][:-1]), np.ones(5, np.float32))
    with pytest.raises(ValueError, match="conn_idx is shorter"):
        db.DetectLoopCandidates(dict(q, conn_idx=c["conn_idx"][:-1]), np.ones(5, np.float32))
    with pytest.raises(ValueError, match="min_score must have shape"):
        db.DetectLoopCandidates(q, np.ones(4, np.float32))
    with pytest.raises(ValueError, match="GPU tensor"):
        db.detect_relocalization_candidates_device(q)    # host arrays to the device form


@pytest.fixture(scope="module")
def handles():
    from orb_slam2_refactored_amd.keyframe_db import KeyFrameDatabase
    from orb_slam2_refactored_amd.vocabulary import ORBVocabulary
    mk = lambda **kw: ORBVocabulary.from_arrays(*(lambda v: (v["k"], v["L"], v["scoring"], v["weighting"], v["parent"], v["is_leaf"],  # noqa: E731
                                                             v["desc"], v["weight"]))(make_vocabulary(0, k=4, L=2, **kw)))
    voc = mk()
    return voc, mk(scoring=1), KeyFrameDatabase(voc, 70, 200)


@pytest.mark.gpu
def test_create_refuses_other_scorings_and_sizes(handles):
    from orb_slam2_refactored_amd.keyframe_db import KeyFrameDatabase
    voc, l2, _ = handles
    with pytest.raises(OrbError, match="L1_NORM"):
        KeyFrameDatabase(l2, 70, 200)
    with pytest.raises(OrbError, match="max_keyframes"):
        KeyFrameDatabase(voc, 0, 200)
    with pytest.raises(OrbError, match="word_cap"):
        KeyFrameDatabase(voc, 70, 4097)


@pytest.mark.gpu
def test_host_entries_refuse_bad_slots_counts_and_lists(handles):
    _, _, db = handles
    c = KC.case("plain")
    q = KC.query(c)
    ms = np.ones(5, np.float32)
    bad = c["slot"].copy()
    bad[3] = 70
    with pytest.raises(OrbError, match="slot outside"):
        db.add(bad, c["bow_word"], c["bow_weight"], c["n_words"])
    bad[3] = bad[2]
    with pytest.raises(OrbError, match="twice"):
        db.add(bad, c["bow_word"], c["bow_weight"], c["n_words"])
    wide = np.zeros((2, 201), np.uint32)
    with pytest.raises(OrbError, match="n_words > word_cap"):
        db.add(np.array([0, 1], np.int32), wide, wide.astype(np.float64), np.array([3, 201], np.int32))
    with pytest.raises(OrbError, match="n_words outside"):
        db.add(np.array([0], np.int32), wide[:1], wide[:1].astype(np.float64), np.array([202], np.int32))
    with pytest.raises(OrbError, match="frame outside"):
        db.add(np.array([0], np.int32), wide[:1], wide[:1].astype(np.float64), np.array([2], np.int32), frame=np.array([1], np.int32))
    with pytest.raises(OrbError, match="slot outside"):
        db.erase([-1])
    assert not db.slots()[0].any()                       # nothing was added by the refused calls
    with pytest.raises(OrbError, match="query frame outside"):
        db.DetectRelocalizationCandidates(dict(q, frame=np.array([0, 6], np.int32)))
    n = c["q_n_words"].copy()
    n[c["q_frame"][0]] = 201
    with pytest.raises(OrbError, match="query n_words"):
        db.DetectRelocalizationCandidates(dict(q, n_words=n))
    cv = c["covis"].copy()
    cv[5, 5] = 70
    with pytest.raises(OrbError, match="covisibility entry"):
        db.DetectRelocalizationCandidates(dict(q, covis=cv))
    off = c["conn_off"].copy()
    off[2] = off[1] - 1
    with pytest.raises(OrbError, match="must not decrease"):
        db.DetectLoopCandidates(dict(q, conn_off=off), ms)
    idx = c["conn_idx"].copy()
    idx[0] = -2
    with pytest.raises(OrbError, match="connected set: slot outside"):
        db.DetectLoopCandidates(dict(q, conn_idx=idx), ms)
    with pytest.raises(OrbError, match="covisible list: slot outside"):
        db.MinScore(q, c["cov_off"], np.where(np.arange(len(c["cov_idx"])) == 0, 99, c["cov_idx"]).astype(np.int32))
    L = lib()
    b = OrbdbQueryBatch(-1, 200, 6)
    assert L.orbdb_detect_reloc_device(db._h, C.byref(b), C.byref(OrbdbResult()), None) == -1 and "n_queries" in last_error()
    b = OrbdbQueryBatch(2, 200, 6)
    assert L.orbdb_detect_reloc_device(db._h, C.byref(b), C.byref(OrbdbResult()), None) == -1 and "null query BowVector" in last_error()
    empty = db.DetectRelocalizationCandidates(dict(q, frame=np.zeros(0, np.int32)))   # Q = 0 is fine and does nothing
    assert empty["cand"].shape == (0, 70)


def test_cpp_wrapper_compiles_links_and_refuses(tmp_path):
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parents[1]
    libso = root / "orb_slam2_refactored_amd" / "liborbslam2_amd.so"
    main = tmp_path / "main.cpp"
    main.write_text("int use_keyframe_db(); int main() { return use_keyframe_db(); }\n")
    exe = tmp_path / "w"
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", f"-I{root / 'include'}", str(root / "tests" / "native" / "keyframe_db_wrapper_use.cpp"),
                    str(main), "-o", str(exe), f"-L{libso.parent}", "-lorbslam2_amd", f"-Wl,-rpath,{libso.parent}"], check=True)
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
