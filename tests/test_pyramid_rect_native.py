"""The pyramid kernels' rectangle model (csrc/orbx_pyr_rect.h) on the CPU.

pyramid_pair_kernel and pyramid_level_kernel read the rectangle a tile works on from the first and last
entries of the tile's rows of the resize tap tables; the host's capacity check (pyr_pair_plan) replays the
same function.  tests/native/pyr_rect_check.cpp runs that function over every tile of every level pair of
the 8-level, scale-1.2 pyramids of 640x480, 1280x720, 1242x375, 1920x1080, 64x48, 97x75, 333x251 and
770x500 (level 1 = 642 columns: a last tile 1-3 columns wide on several levels) and requires, by brute
force: every tap of every tile pixel inside the level-l rectangle, every tap of every rectangle pixel inside
the staged level-(l-1) rectangle, every LDS / table / pass capacity of the kernel's 64x64 tile, and the
written rectangles covering level l.  The same geometric properties are checked for a wider (128x32), a
flatter (64x32), a taller (32x128) and a smaller (80x48) tile, whose issued-slot ratios it prints.  Built
with AddressSanitizer and UBSan."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_rectangles_hold_every_tap_and_cover_the_level(tmp_path):
    exe = tmp_path / "pyr_rect_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"),
                    str(ROOT / "tests" / "native" / "pyr_rect_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "0 failures" in out.stdout and "runtime error" not in out.stderr, \
        out.stdout[-3000:] + out.stderr[-3000:]
