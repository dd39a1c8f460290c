"""Host check of the sampler's even dealing of helper lanes (spt::DealRule) with a 64-lane
model of coop_ball_vector against the oracle's sequential loop: tests/cpp/sampler_deal_check.cpp,
a stand-alone program over spt_internal.h (host code only), run as built and under
AddressSanitizer + UBSan linked into the executable."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simplepathtracer_amd", "csrc")


def _hipcc_host(src, exe, extra=()):
    subprocess.run(["hipcc", "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-ffp-contract=off", *extra,
                    "-I", CSRC, "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", src),
                    "-o", str(exe)], check=True)


@pytest.fixture(scope="module")
def oracle_lib():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    return os.path.join(ROOT, "oracle", "build")


@pytest.mark.parametrize("sanitize", [None, "address,undefined"])
def test_sampler_dealing_and_model(tmp_path, oracle_lib, sanitize):
    exe = tmp_path / "sampler_deal_check"
    san = [f"-fsanitize={sanitize}", "-fno-sanitize-recover=undefined"] if sanitize else []
    _hipcc_host("sampler_deal_check.cpp", exe, [*san, "-L", oracle_lib, "-lspt_oracle", f"-Wl,-rpath,{oracle_lib}"])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr

