"""LocalBA's helper thread (csrc/host_helper.h) on the CPU, without a GPU or the library.

tests/native/host_helper_check.cpp posts 1000 short jobs in sequence with post / wait and requires that
each ran exactly once and that its plain writes are visible when wait returns, and destroys a helper with
and without a job ever posted.  Built once with ThreadSanitizer (the job's writes against the caller's
reads after wait: a missing release / acquire pairing is a reported race) and once with AddressSanitizer."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("sanitizer", ["thread", "address,undefined"])
def test_host_helper_post_wait(tmp_path, sanitizer):
    exe = tmp_path / "host_helper_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", f"-fsanitize={sanitizer}", "-fno-omit-frame-pointer", "-pthread",
                    "-I", str(ROOT / "orb_slam2_refactored_amd" / "csrc"),
                    str(ROOT / "tests" / "native" / "host_helper_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "0 failures" in out.stdout and "WARNING: ThreadSanitizer" not in out.stderr, \
        out.stdout + out.stderr
