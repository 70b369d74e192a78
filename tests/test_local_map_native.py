"""csrc/tl_frustum.h on the CPU against tests/local_map_ref.py: tests/native/local_map_check.cpp is compiled stand-alone twice,
plainly at -O2 and under AddressSanitizer and UBSan, and run as a program on every (frame, local point) pair the "edges" case
projects, the hand-placed points among them.  The test a point leaves at, u, v, u - bf/z and viewCos (as float bits) and the
level are equal bit for bit.  CPU only."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import local_map_cases as LC
import local_map_ref as R

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("tl") / f"local_map_check_{request.param}"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *flags,
                    "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"),
                    str(ROOT / "tests" / "native" / "local_map_check.cpp"), "-o", str(out)], check=True)
    return out


def hx(a):
    return " ".join(float(x).hex() for x in np.asarray(a, np.float64).reshape(-1))


def bits(x):
    return int(np.float32(x).view(np.uint32))


def test_frustum_is_bit_equal_on_the_edges_points(exe):
    c = LC.case("edges")
    m, fr = c["map"], c["frames"]
    o = LC.expected("edges", 5)
    lines, want = [], []
    for f in range(5):
        for j in np.flatnonzero(o["fail"][f] >= 0):
            p = o["local_mp"][f, j]
            args = (fr["pose"][f], fr["camera"][f], fr["bounds"][f], m["mp_xw"][p], m["mp_normal"][p], m["mp_max_min"][p, 0],
                    m["mp_max_min"][p, 1], fr["min_view_cos"], fr["log_scale_factor"])
            lines.append(" ".join(hx(a) for a in args) + f" {fr['n_levels']}")
            r = R.frustum(*args, fr["n_levels"])
            assert r["fail"] == o["fail"][f, j]
            want.append([r["fail"], bits(r["u"]), bits(r["v"]), bits(r["ur"]), bits(r["view_cos"]), r["level"]])
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    got = [[int(x) for x in l.split()] for l in out.stdout.strip().split("\n")]
    assert got == want
    assert {w[0] for w in want} == {R.PASS, R.DEPTH, R.BOUNDS, R.DISTANCE, R.VIEW_COS} and len(want) > 1500
    assert {0, 7} <= {w[5] for w in want if w[0] == R.PASS}
