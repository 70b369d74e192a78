"""csrc/ba_window.h on the CPU against tests/local_ba_window_ref.py: tests/native/ba_window_check.cpp is compiled stand-alone
twice, plainly at -O2 and under AddressSanitizer and UBSan, and run as a program on the hand-built map, the generated maps and
the map with entries outside their tables.  Every list, count, index array and value array of the window and every table after
the write-back are equal, floats as bits.  CPU only."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import local_ba_map_cases as LC
import local_ba_window_ref as WR
from test_local_ba_window_ref import hand_map

ROOT = Path(__file__).resolve().parents[1]
MAPS = ["hand", "small", "large", "dirty"]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("baw") / f"ba_window_check_{request.param}"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *flags,
                    "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"),
                    str(ROOT / "tests" / "native" / "ba_window_check.cpp"), "-o", str(out)], check=True)
    return out


def the_map(name):
    return (hand_map(), 3) if name == "hand" else LC.dirty() if name == "dirty" else LC.case(name)


def words(v):
    v = np.ascontiguousarray(v)
    return v.view(np.int32) if v.dtype.itemsize > 1 and v.dtype != np.int32 else v.astype(np.int32)


def run(exe, mode, tables):
    text = "".join(f"{k} {words(v).size} " + " ".join(map(str, words(v).reshape(-1).tolist())) + "\n" for k, v in tables.items())
    out = subprocess.run([str(exe), mode], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    got = {}
    for line in out.stdout.strip().split("\n"):
        name, n, *vals = line.split()
        got[name] = np.array(vals, np.int64).astype(np.int32)
        assert len(vals) == int(n)
    return got


@pytest.mark.parametrize("name", MAPS)
def test_the_sequential_gather_equals_the_restatement(exe, name):
    t, cur = the_map(name)
    want = WR.gather(t, cur)
    full = (sum(want["counts"][:2]), want["counts"][2], want["counts"][3])
    got = run(exe, "gather", dict(t, cur=np.array([cur], np.int32), caps=np.array(full, np.int32)))
    assert tuple(got["counts"][:6]) == want["counts"] + (WR.OK, want["one_cam"])
    for k in WR.WINDOW_ARRAYS:
        assert np.array_equal(got[k], words(want[k]).reshape(-1)), k
    for short in range(3):                                   # one short: the status and the counts, nothing else
        caps = np.array([c - (i == short) for i, c in enumerate(full)], np.int32)
        got = run(exe, "gather", dict(t, cur=np.array([cur], np.int32), caps=caps))
        assert list(got) == ["counts"] and tuple(got["counts"][:5]) == want["counts"] + (WR.OVERFLOW,)


@pytest.mark.parametrize("name", ["hand", "small", "large"])
def test_the_sequential_write_back_equals_the_restatement(exe, name):
    t, cur = the_map(name)
    w = WR.gather(t, cur)
    rng = np.random.default_rng(11)
    P, N, E = sum(w["counts"][:2]), w["counts"][2], w["counts"][3]
    outlier = (rng.random(E) < 0.15).astype(np.uint8)
    if name == "hand":
        outlier[:] = 0
        outlier[[1, 2, 3, 6]] = 1
    R, tr, X = rng.normal(size=(P, 9)), rng.normal(size=(P, 3)), rng.normal(size=(N, 3)) * 10
    want = WR.apply(t, w, outlier, R, tr, X)
    assert want["mp_bad"].sum() > t["mp_bad"].sum()
    got = run(exe, "apply", dict(t, cur=np.array([cur], np.int32), outlier=outlier, pose_R=R, pose_t=tr, points=X))
    for k in WR.UPDATED:
        assert np.array_equal(got[k], words(want[k]).reshape(-1)), k


def test_cpp_wrapper_compiles(tmp_path):
    subprocess.run(["g++", "-std=c++14", "-Wall", "-Werror", "-c", f"-I{ROOT / 'include'}",
                    str(ROOT / "tests" / "native" / "local_ba_wrapper_use.cpp"), "-o", str(tmp_path / "w.o")], check=True)
