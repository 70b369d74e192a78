"""The projection searches' workspace layouts (csrc/orbp_layout.h) on the CPU.

tests/native/pj_layout_check.cpp carries the byte-count sums orbp.hip and its headers kept by hand beside
their carve sequences before the layouts replaced both, and requires each workspace's dry-run size (a
carve from a null base) to equal them: the grid / walk region alone, with the motion search's choice
array, with the projected-point block (relocalisation, Fuse, the Sim3 projection search), with
SearchForInitialization's candidate lists, and SearchBySim3's two side blocks, for the shapes (frames,
keypoints, points) = (1, 0, 0), (1, 1, 1), (3, 8192, 700) and (2, 100, 0).  Every workspace is then carved
from a malloc of exactly that size and the first and last element of each field written under
AddressSanitizer; field offsets must be multiples of 256, strictly increasing in the documented order and
free of overlap."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_layouts_match_the_former_byte_counts(tmp_path):
    exe = tmp_path / "pj_layout_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"), "-I", str(ROOT / "include"),
                    str(ROOT / "tests" / "native" / "pj_layout_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "0 failures" in out.stdout and "runtime error" not in out.stderr, \
        out.stdout + out.stderr
