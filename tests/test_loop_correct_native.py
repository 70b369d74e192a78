"""csrc/lc_propagate.h on the CPU against tests/loop_correct_ref.py: tests/native/loop_correct_check.cpp is compiled
stand-alone twice, plainly at -O2 and under AddressSanitizer and UBSan, and run as a program on the generated maps, the
ones with entries outside their tables among them.  Every array is equal, floats as bits.  CPU only."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import loop_correct_cases as LC
import loop_correct_ref as LR
from test_map_maintenance_native import dump

ROOT = Path(__file__).resolve().parents[1]
COMPARED = LR.UPDATED + ("vertex_sim3", "edge_sim3", "point_ref")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("lc") / f"loop_correct_check_{request.param}"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", *flags,
                    "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"), "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "native" / "loop_correct_check.cpp"), "-o", str(out)], check=True)
    return out


def run(exe, tables):
    out = subprocess.run([str(exe)], input=dump(tables), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    got = {}
    for line in out.stdout.strip().split("\n"):
        name, n, *vals = line.split()
        got[name] = np.array(vals, np.int64).astype(np.int32)
        assert len(vals) == int(n)
    return got


def flat(a):
    a = np.ascontiguousarray(a)
    return (a.view(np.int32) if a.dtype == np.float32 else a.astype(np.int32)).reshape(-1)


@pytest.mark.parametrize("name,s", [("small", None), ("small", 1.7), ("wide", None), ("dirty", None), ("dirty_rows", None)])
def test_the_header_equals_the_restatement(exe, name, s):
    want = LC.expected_propagate(name, s)
    conn, n = LC.expected_connected(name)
    got = run(exe, dict(LC.after_update(name), scale=LC.SCALE, cur=np.array([LC.CUR[name]], np.int32), scw=LC.scw(name, s),
                        connected=conn))                      # the padded list
    for k in COMPARED:
        assert np.array_equal(got[k], flat(want[k])), k
    m = LC.after_update(name)
    assert (want["mp_xw"] != m["mp_xw"]).any() and (want["kf_pose"] != m["kf_pose"]).any(axis=1).sum() == n


def test_cpp_wrapper_compiles(tmp_path):
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "native" / "loop_correct_wrapper_use.cpp"), "-o", str(tmp_path / "w.o")], check=True)
