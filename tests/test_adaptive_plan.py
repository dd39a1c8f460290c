"""Host check of adaptive sampling's tile plan (spt_adaptive.h): tests/cpp/adaptive_check.cpp,
a stand-alone program over the header's own arithmetic -- the code adaptive_plan_kernel runs
on the device -- run as built and under AddressSanitizer + UBSan linked into the executable."""
import subprocess

import pytest

from test_sampler_dealing import _hipcc_host


@pytest.mark.parametrize("sanitize", [None, "address,undefined"])
def test_adaptive_plan_rectangles(tmp_path, sanitize):
    exe = tmp_path / "adaptive_check"
    san = [f"-fsanitize={sanitize}", "-fno-sanitize-recover=undefined"] if sanitize else []
    _hipcc_host("adaptive_check.cpp", exe, san)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
