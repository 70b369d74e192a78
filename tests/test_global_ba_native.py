"""csrc/gba_update.h on the CPU against tests/global_ba_ref.py: tests/native/global_ba_check.cpp is compiled stand-alone
twice, plainly at -O2 and under AddressSanitizer and UBSan, and run as a program on every (child, parent) step and every
moved point of the big table; the results are equal as float bits.  CPU only."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import global_ba_cases as GC
import global_ba_ref as G

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("gba") / f"global_ba_check_{request.param}"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", *flags,
                    "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"),
                    str(ROOT / "tests" / "native" / "global_ba_check.cpp"), "-o", str(out)], check=True)
    return out


def hx(a):
    return " ".join(float(x).hex() for x in np.asarray(a, np.float64).reshape(-1))


def bits(v):
    return [int(x) for x in np.asarray(v, np.float32).view(np.uint32)]


def test_arithmetic_is_bit_equal_on_the_big_table(exe):
    m = GC.big_case()
    rng = np.random.default_rng(1)
    lines, want = [], []
    off, idx = m["kf_child_off"], m["kf_child_idx"]
    for k in range(len(off) - 1):
        for c in idx[off[k]:off[k + 1]]:
            args = (m["kf_pose"][c], m["kf_pose"][k], m["kf_pose_gba"][k])
            lines.append("C " + " ".join(hx(a) for a in args))
            want.append(bits(G.f_mul(G.f_mul(args[0], G.f_inverse(args[1])), args[2])))
    for p in range(300):
        a, b = rng.integers(0, 400, 2)
        args = (m["kf_pose_bef"][a], m["kf_pose"][b], m["mp_xw"][p])
        lines.append("P " + " ".join(hx(x) for x in args))
        want.append(bits(G.f_move_point(*args)))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    got = [[int(x) for x in l.split()] for l in out.stdout.strip().split("\n")]
    assert len(want) > 600 and got == want
