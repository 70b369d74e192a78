"""Sim3Solver's argument checks: the library exports both entries, the host entry refuses bad offsets, octaves,
parameters and draws with a message in orb_last_error() before anything is copied, arrays shorter than the C-ABI
reads are refused in Python, and the C++ wrappers compile.  CPU only: no call reaches a device."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from orb_slam2_refactored_amd._lib import LIB_PATH, OrbError, lib
from orb_slam2_refactored_amd.sim3solver import Sim3SolverIterate, make_draws
from orb_slam2_refactored_amd.synth import make_sim3solver_batch

ROOT = Path(__file__).resolve().parents[1]


def _batch(**kw):
    return make_sim3solver_batch(1, n_corr=[12, 30], **kw)


def test_the_library_exports_both_entries():
    assert LIB_PATH.exists(), "library not built (run __graft_entry__.build())"
    raw = C.CDLL(str(LIB_PATH))
    for name in ("orb_sim3solver_iterate", "orb_sim3solver_iterate_device"):
        assert hasattr(raw, name), name


def _refused(b, match):
    with pytest.raises(OrbError, match=match):
        Sim3SolverIterate(b)
    assert lib().orb_last_error()   # the message is set


def test_bad_offsets_are_refused():
    b = _batch()
    b["kp1_begin"] = b["kp1_begin"].copy()
    b["kp1_begin"][1] = b["kp1_begin"][2] + 1
    _refused(b, "non-decreasing|kp1_begin")
    b = _batch()
    b["kp2_begin"] = b["kp2_begin"].copy()
    b["kp2_begin"][0] = 1
    _refused(b, "kp1_begin / kp2_begin")


@pytest.mark.parametrize("key", ["kp1_octave", "kp2_octave"])
@pytest.mark.parametrize("value", [-1, 8])
def test_bad_octaves_are_refused(key, value):
    b = _batch()
    b[key] = b[key].copy()
    b[key][3] = value
    _refused(b, key)


def test_bad_parameters_are_refused():
    _refused(dict(_batch(), min_inliers=2), "min_inliers")
    _refused(dict(_batch(), maxk=0), "maxk")
    _refused(dict(_batch(), max_iterations=0, draws=make_draws(2, 1)), "max_iterations")
    _refused(dict(_batch(), probability=1.0), "probability")
    b = _batch()
    b["match12"] = b["match12"].copy()
    b["match12"][2] = 10 ** 6
    _refused(b, "match12")


def test_draws_outside_the_generator_range_are_refused():
    b = _batch()
    b["draws"] = b["draws"].copy()
    b["draws"][1, 7, 2] = -1
    _refused(b, "draws")
    b = dict(_batch(), rand_max=32767)   # the table was made for glibc's RAND_MAX
    _refused(b, "draws")


@pytest.mark.parametrize("key", ["kp1_octave", "mp1_xw", "mp2_valid", "match12", "pose2", "camera1", "draws"])
def test_short_arrays_are_refused(key):
    b = _batch()
    b[key] = b[key].reshape(-1)[:-1]
    with pytest.raises(ValueError, match=key):
        Sim3SolverIterate(b)


def test_missing_array_is_refused():
    b = _batch()
    del b["draws"]
    with pytest.raises(ValueError, match="draws"):
        Sim3SolverIterate(b)


def test_cpp_wrapper_compiles_links_and_refuses(tmp_path):
    src = ROOT / "tests" / "native" / "sim3solver_wrapper_use.cpp"
    obj = tmp_path / "s.o"
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}", str(src), "-o", str(obj)], check=True)
    main = tmp_path / "main.cpp"
    main.write_text("int use_sim3solver_empty(); int main() { return use_sim3solver_empty(); }\n")
    exe = tmp_path / "s"
    subprocess.run(["g++", str(main), str(obj), "-o", str(exe), f"-L{LIB_PATH.parent}", "-lorbslam2_amd",
                    f"-Wl,-rpath,{LIB_PATH.parent}"], check=True)
    # an empty batch returns, and min_inliers = 2 is refused, before any device call: no GPU needed
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
