"""Host check of Normalize's range guard (spt_device.h normalize_slow_mask): the combined
min3 / max3 / |v|^2 predicate against the three-fold div_operand_ok conjunction, NaN
behaviour of v_min3_f32 / v_max3_f32 included.  tests/cpp/normalize_guard_check.cpp is a
stand-alone program (plain C++, no device code), run as built and under AddressSanitizer +
UBSan linked into the executable."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sanitize", [None, "address,undefined"])
def test_normalize_guard_equals_operand_tests(tmp_path, sanitize):
    exe = tmp_path / "normalize_guard_check"
    san = [f"-fsanitize={sanitize}", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Werror", *san,
                    os.path.join(ROOT, "tests", "cpp", "normalize_guard_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
