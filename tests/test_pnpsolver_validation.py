"""PnPsolver's argument checks: the library exports both entries, the host entry refuses bad parameters, offsets,
octaves and draws with a message in orb_last_error() before anything is copied, arrays shorter than the C-ABI reads
and wrong dtypes or devices are refused in Python, and the C++ wrapper compiles.  CPU only: no call reaches a device."""
import ctypes as C
import subprocess
from pathlib import Path

import numpy as np
import pytest

from orb_slam2_refactored_amd._lib import LIB_PATH, OrbError, lib
from orb_slam2_refactored_amd.pnpsolver import PnPsolverIterate, pnpsolver_iterate_device
from orb_slam2_refactored_amd.synth import make_pnp_batch

ROOT = Path(__file__).resolve().parents[1]


def _batch(**kw):
    b = make_pnp_batch(1, n_corr=[12, 30], n_draws=40)
    b.update(kw)
    return b


def test_the_library_exports_both_entries():
    assert LIB_PATH.exists(), "library not built (run __graft_entry__.build())"
    raw = C.CDLL(str(LIB_PATH))
    for name in ("orb_pnpsolver_iterate", "orb_pnpsolver_iterate_device"):
        assert hasattr(raw, name), name


def _refused(b, match):
    with pytest.raises(OrbError, match=match):
        PnPsolverIterate(b)
    assert lib().orb_last_error()


def test_bad_parameters_are_refused_with_the_field_named():
    _refused(_batch(min_set=5), "min_set")
    _refused(_batch(min_set=3), "min_set")
    _refused(_batch(min_inliers=5), "min_inliers")
    _refused(_batch(maxk=0), "maxk")
    _refused(_batch(max_iterations=0), "max_iterations")
    _refused(_batch(probability=1.0), "probability")
    _refused(_batch(epsilon=1.5), "epsilon")
    _refused(_batch(th2=0.0), "th2")


def test_bad_offsets_octaves_and_state_are_refused():
    b = _batch()
    b["kp_begin"] = b["kp_begin"].copy()
    b["kp_begin"][1] = b["kp_begin"][2] + 1
    _refused(b, "kp_begin")
    for v in (-1, 8):
        b = _batch()
        b["kp_octave"] = b["kp_octave"].copy()
        b["kp_octave"][3] = v
        _refused(b, "kp_octave")
    _refused(_batch(iterations=np.array([0, -1], np.int32)), "iterations")


def test_draws_outside_the_generator_range_and_a_short_table_are_refused():
    b = _batch()
    b["draws"] = b["draws"].copy()
    b["draws"][1, 7, 3] = -1
    _refused(b, "draws")
    _refused(_batch(rand_max=32767), "draws")   # the table was made for glibc's RAND_MAX
    _refused(_batch(draws=np.ascontiguousarray(_batch()["draws"][:, :10])), "n_draws")   # the cap of 30 correspondences is 35


@pytest.mark.parametrize("key", ["kp_xy", "kp_octave", "camera", "mp_valid", "mp_xw"])
def test_short_arrays_are_refused(key):
    b = _batch()
    b[key] = b[key].reshape(-1)[:-1]
    with pytest.raises(ValueError, match=key):
        PnPsolverIterate(b)


def test_missing_and_misshapen_draws_are_refused():
    b = _batch()
    del b["draws"]
    with pytest.raises(ValueError, match="draws"):
        PnPsolverIterate(b)
    with pytest.raises(ValueError, match="draws"):
        PnPsolverIterate(_batch(draws=_batch()["draws"][:, :, :3]))


def test_the_device_wrapper_refuses_host_arrays_and_wrong_dtypes():
    import torch
    b = _batch()
    with pytest.raises(ValueError, match="kp_begin"):
        pnpsolver_iterate_device(b)
    t = {k: torch.as_tensor(v) if isinstance(v, np.ndarray) and k != "level_sigma2" else v for k, v in b.items()}
    with pytest.raises(ValueError, match="kp_begin|GPU"):   # CPU tensors
        pnpsolver_iterate_device(t)
    t["kp_xy"] = t["kp_xy"].double()
    with pytest.raises(ValueError, match="kp_begin|kp_xy"):
        pnpsolver_iterate_device(t)


def test_cpp_wrapper_compiles_links_and_refuses(tmp_path):
    src = ROOT / "tests" / "native" / "pnpsolver_wrapper_use.cpp"
    obj = tmp_path / "p.o"
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}", str(src), "-o", str(obj)], check=True)
    main = tmp_path / "main.cpp"
    main.write_text("int use_pnpsolver_empty(); int main() { return use_pnpsolver_empty(); }\n")
    exe = tmp_path / "p"
    subprocess.run(["g++", str(main), str(obj), "-o", str(exe), f"-L{LIB_PATH.parent}", "-lorbslam2_amd",
                    f"-Wl,-rpath,{LIB_PATH.parent}"], check=True)
    # an empty batch returns, and min_set = 5 / min_inliers = 5 are refused, before any device call: no GPU needed
    assert subprocess.run([str(exe)], timeout=60).returncode == 0
