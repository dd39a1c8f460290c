"""The fold's colour table arithmetic on the host (spt_codes.h): tests/cpp/ctab_check.cpp, a
stand-alone program built with plain g++, AddressSanitizer and UBSan linked into the
executable.  No GPU."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_colour_table_indexing_and_cap(tmp_path):
    exe = tmp_path / "ctab_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-I", os.path.join(ROOT, "simplepathtracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "ctab_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
