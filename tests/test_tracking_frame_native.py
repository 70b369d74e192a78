"""csrc/tf_frame.h on the CPU against tests/tracking_frame_ref.py: tests/native/tracking_frame_check.cpp is compiled stand-alone
twice, plainly at -O2 and under AddressSanitizer and UBSan, and run as a program.  The pose product with the motion, the
projection tests, the unprojection (uvZToWorld and UnprojectStereo) and the rank rule of the stereo point creation are equal
bit for bit.  CPU only."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import tracking_frame_cases as TC
import tracking_frame_ref as R
from orb_slam2_refactored_amd import tracking as T

ROOT = Path(__file__).resolve().parents[1]


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("tf") / f"tracking_frame_check_{request.param}"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", *flags,
                    "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"),
                    str(ROOT / "tests" / "native" / "tracking_frame_check.cpp"), "-o", str(out)], check=True)
    return out


def hx(a):
    return " ".join(float(x).hex() for x in np.asarray(a, np.float64).reshape(-1))


def bits(x):
    return int(np.float32(x).view(np.uint32))


def ask(exe, lines):
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    return [[int(x) for x in l.split()] for l in out.stdout.strip().split("\n")]


def test_pose_product_and_motion_are_bit_equal(exe):
    rng = np.random.default_rng(0)
    lines, want = [], []
    for k in range(200):
        V, L = rng.normal(0, 1, 12).astype(np.float32), rng.normal(0, 1, 12).astype(np.float32)
        if k % 7 == 0:
            V[rng.integers(0, 12, 4)] = [0.0, -0.0, 0.0, -0.0]   # s = 0; s += ... turns -0 products into +0
        base, mono = np.float32(rng.uniform(0, 1)), k % 3 == 0
        Cp = R.pose_product(V, L)
        lines.append(f"P {hx(V)} {hx(L)} {hx(base)} {int(mono)}")
        want.append([bits(x) for x in Cp] + [R.motion_of(L, Cp, base, mono)])
    assert ask(exe, lines) == want
    assert {w[-1] for w in want} == {0, 1, 2}


def test_the_projection_tests_are_bit_equal_on_a_generated_case(exe):
    c = TC.case("n1000")
    fr, m = c["frames"], c["map"]
    lines, want = [], []
    for i in np.flatnonzero(fr["frame_mappoint"][0] >= 0):
        args = (fr["pose"][0], fr["camera"][0], fr["bounds"][0], m["mp_xw"][fr["frame_mappoint"][0, i]])
        lines.append("J " + " ".join(hx(a) for a in args))
        v, u, w, ur = R.project(*args)
        want.append([v, bits(u), bits(w), bits(ur)])
    rng = np.random.default_rng(1)
    for _ in range(300):   # behind the camera and outside the image
        X = rng.uniform(-30, 30, 3).astype(np.float32)
        args = (fr["pose"][0], fr["camera"][0], fr["bounds"][0], X)
        lines.append("J " + " ".join(hx(a) for a in args))
        v, u, w, ur = R.project(*args)
        want.append([v, bits(u), bits(w), bits(ur)])
    assert ask(exe, lines) == want
    assert sum(w[0] for w in want) > 100 and sum(1 - w[0] for w in want) > 100


def test_the_unprojection_is_bit_equal_in_both_forms(exe):
    c = TC.case("n257")
    fr = c["frames"]
    lines, want = [], []
    for i in range(257):
        Z = fr["kp_depth"][0, i]
        if not Z > 0:
            continue
        for vo in (False, True):
            lines.append(f"U {hx(fr['pose'][0])} {hx(fr['camera'][0])} {hx(fr['kp_xy'][0, i])} {hx(Z)} {int(vo)}")
            want.append([bits(x) for x in R.unproject(fr["pose"][0], fr["camera"][0], fr["kp_xy"][0, i, 0], fr["kp_xy"][0, i, 1], Z, vo)])
    assert ask(exe, lines) == want and len(want) > 200


def rank_request(depth, th, mode):
    """(the request line, the answer the restatement gives) for one frame of depths with no map point at all."""
    n = len(depth)
    fr = dict(frame_n=np.array([n], np.int32), frame_mappoint=np.full((1, n), -1, np.int32), kp_depth=depth.reshape(1, n),
              pose=np.array([[1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]], np.float32), camera=np.array([[500, 500, 320, 240, 40]], np.float32),
              kp_xy=np.zeros((1, n, 2), np.float32))
    o = R.stereo_points(fr, dict(mp_nobs=np.zeros(0, np.int32)), mode, th)
    order = sorted((i for i in range(n) if depth[i] > 0), key=lambda i: (0.0 if mode == T.INIT else float(depth[i]), i))
    ranks = [-1] * n
    for r, i in enumerate(order):
        ranks[i] = r
    assert list(o["created_kp"][0, :o["n_created"][0]]) == order[:o["n_processed"][0]]   # every processed one is created here
    line = f"R {hx(np.float32(th))} {int(mode == T.INIT)} {n} " + " ".join(str(bits(z)) for z in depth)
    return line, [int(o["n_processed"][0])] + ranks


def test_the_rank_rule_is_equal(exe):
    rng = np.random.default_rng(2)
    lines, want = [], []
    for n, th in ((0, 5.0), (1, 5.0), (99, 50.0), (100, 50.0), (101, 50.0), (150, 5.0), (300, 5.0), (300, 0.5), (300, np.nan), (300, -1.0)):
        depth = rng.uniform(1, 20, n).astype(np.float32)
        if n >= 150:
            depth[rng.integers(0, n, 40)] = np.float32(5.0)
            for v in (0.0, -0.0, -3.0, np.nan, np.inf, 1e-42, 3e-39):
                depth[rng.integers(0, n, 5)] = np.float32(v)
        for mode in (T.KEYFRAME, T.INIT):
            line, w = rank_request(depth, th, mode)
            lines.append(line)
            want.append(w)
    assert ask(exe, lines) == want
