"""csrc/fr_undistort.h on the CPU against tests/frame_ref.py: tests/native/frame_check.cpp is compiled stand-alone twice,
plainly at -O2 and under AddressSanitizer and UBSan, and run as a program.  The undistortion (with the iteration count as an
argument), the k1 == 0 rule, the image bounds, the depth conversion with ComputeStereoFromRGBD's rule and the truncated pixel
are equal bit for bit; the library's two plain CPU functions, which are the same header, agree too.  CPU only."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import frame_ref as R

ROOT = Path(__file__).resolve().parents[1]
f32 = np.float32


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def exe(request, tmp_path_factory):
    out = tmp_path_factory.mktemp("fr") / f"frame_check_{request.param}"
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer"]
    subprocess.run(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-Wno-unknown-pragmas", *flags,
                    "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"),
                    str(ROOT / "tests" / "native" / "frame_check.cpp"), "-o", str(out)], check=True)
    return out


def hx(a):
    return " ".join(float(x).hex() for x in np.asarray(a, np.float64).reshape(-1))


def bits(x):
    return int(f32(x).view(np.uint32))


def ask(exe, lines):
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "runtime error" not in out.stderr, out.stderr[-2000:]
    return [[int(x) for x in l.split()] for l in out.stdout.strip().split("\n")]


CAMERAS = ((R.TUM1_CAMERA, R.TUM1_DIST), (R.TUM2_CAMERA, R.TUM2_DIST), (R.TUM1_CAMERA, np.append(R.TUM1_DIST[:4], f32(0))),
           (np.array([500, 500, 320, 240, 40], f32), np.array([-5.0, 0, 0, 0, 0], f32)))   # the last: icdist < 0 far out


def points():
    rng = np.random.default_rng(0)
    xs, ys = np.linspace(0, 640, 17), np.linspace(0, 480, 13)
    grid = np.stack(np.meshgrid(xs, ys), -1).reshape(-1, 2)
    return np.concatenate([grid, rng.uniform(-3, 643, (150, 2))]).astype(f32)


def test_the_undistortion_is_bit_equal_for_every_iteration_count(exe):
    xy = points()
    lines, want = [], []
    for cam, dist in CAMERAS:
        for iters in (0, 1, 5, 6, 10):
            ref = R.undistort(cam, dist, xy, iters)
            for p, r in zip(xy, ref):
                lines.append(f"U {hx(cam[:4])} {hx(dist)} {hx(p)} {iters}")
                want.append([bits(r[0]), bits(r[1])])
    assert ask(exe, lines) == want
    # the last camera does leave the loop for some points (they come back as the first guess) and not for others
    left = [np.array_equal(a, b) for a, b in zip(R.undistort(*CAMERAS[3], xy, 5), R.undistort(*CAMERAS[3], xy, 0))]
    assert 0 < sum(left) < len(xy)


def test_the_k1_rule_and_the_bounds_are_bit_equal(exe):
    xy = points()[::7]
    lines, want = [], []
    cases = list(CAMERAS) + [(R.TUM1_CAMERA, np.array([0.0, 0.3, 0.01, 0.02, 0.1], f32)), (R.TUM1_CAMERA, np.array([-0.0, 0, 0, 0, 0], f32))]
    for cam, dist in cases:
        ref = R.keypoint_xy(cam, dist, xy)
        for p, r in zip(xy, ref):
            lines.append(f"K {hx(cam[:4])} {hx(dist)} {hx(p)}")
            want.append([bits(r[0]), bits(r[1])])
        for rows, cols in ((480, 640), (375, 1242), (1, 1)):
            lines.append(f"B {rows} {cols} {hx(cam[:4])} {hx(dist)}")
            want.append([bits(v) for v in R.image_bounds(rows, cols, cam, dist)])
    assert ask(exe, lines) == want


def test_the_depth_rule_and_the_pixel_are_equal(exe):
    rng = np.random.default_rng(1)
    lines, want = [], []
    factor = f32(1.0 / 5000.0)
    for raw in (0, 1, 2, 4999, 5000, 65535):
        x = f32(rng.uniform(0, 640))
        lines.append(f"D 1 {raw} {hx(factor)} {hx(x)} {hx(f32(40))}")
        want.append([bits(v) for v in R.rgbd(R.depth_value(np.uint16(raw), factor), x, f32(40))])
    specials = [0.0, -0.0, -3.0, np.nan, np.inf, -np.inf, 1e-42, 3e-39, 1e-38, 0.5, 2.5, 80.0]
    for d in [f32(v) for v in specials] + list(rng.uniform(0.1, 20, 40).astype(f32)):
        for fac in (f32(1), factor, f32(0.5)):
            x = f32(rng.uniform(0, 640))
            lines.append(f"D 0 {bits(d)} {hx(fac)} {hx(x)} {hx(f32(386.1448))}")
            want.append([bits(v) for v in R.rgbd(R.depth_value(d, fac), x, f32(386.1448))])
    n_depth = len(lines)
    for x, y in ((3.99, 7.99), (639.99, 479.99), (-0.5, 0), (-1, 0), (640, 0), (0, 480), (0, -1.5), (np.nan, 5), (5, np.nan),
                 (np.inf, 0), (0, 0), (1e9, 3)):
        lines.append(f"P {hx(f32(x))} {hx(f32(y))} 480 640")
        p = R.pixel(x, y, 480, 640)
        want.append([0, -1, -1] if p is None else [1, p[0], p[1]])
    got = ask(exe, lines)
    assert got == want
    assert sum(w[1] == bits(-1) for w in want[:n_depth]) > 10 and sum(w[1] != bits(-1) for w in want[:n_depth]) > 50


def test_the_library_cpu_functions_are_the_same_arithmetic():
    from orb_slam2_refactored_amd import frame
    xy = points()
    for cam, dist in CAMERAS + ((R.TUM1_CAMERA, np.zeros(5, f32)),):
        assert np.array_equal(frame.undistort_points(cam, dist, xy).view(np.uint32), R.keypoint_xy(cam, dist, xy).view(np.uint32))
        assert np.array_equal(frame.image_bounds(480, 640, cam, dist).view(np.uint32), R.image_bounds(480, 640, cam, dist).view(np.uint32))
    assert np.array_equal(frame.undistort_points(R.TUM1_CAMERA, R.TUM1_DIST[:4], xy).view(np.uint32),
                          R.keypoint_xy(R.TUM1_CAMERA, R.TUM1_DIST[:4], xy).view(np.uint32))
