"""The host entries' staging plan (csrc/host_mirror.h) on the CPU, without a GPU or the library.

tests/native/host_mirror_check.cpp drives Mirror with memcpy over a heap slab for arrays of 0, 1, 63 and 65 elements of
1, 4 and 12 bytes: null fields stay null and take no room, a zero-count field (a zero-length heap block) has an address
of its own and is never read, every address is 256-byte aligned inside the reserved size, in / out / in-out fields are
copied in exactly those directions, a shared host array is one device array copied once, and const T*& binds like T*&.
Built with AddressSanitizer and UBSan, so an out-of-bounds read is a reported error."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]


def test_host_mirror_plan_and_copies(tmp_path):
    exe = tmp_path / "host_mirror_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                    "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"),
                    str(ROOT / "tests" / "native" / "host_mirror_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "0 failures" in out.stdout and out.stderr == "", out.stdout + out.stderr
