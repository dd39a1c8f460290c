"""The HIP-free half of the tiling read-ahead (simplepathtracer_amd/csrc/spt_readahead.h:
tile recognition, the frame / arming bookkeeping, the reader gate) driven on the CPU by
tests/cpp/readahead_check.cpp, a stand-alone program built with plain g++ and run under
ThreadSanitizer and under AddressSanitizer + UBSan (both linked into the executable)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", ["thread", "address,undefined"])
def test_readahead_state_under_sanitizers(tmp_path, sanitize):
    exe = tmp_path / "readahead_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", f"-fsanitize={sanitize}",
                    "-I", os.path.join(ROOT, "simplepathtracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "readahead_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
