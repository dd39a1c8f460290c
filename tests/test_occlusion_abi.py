"""CPU tests of the occlusion-query entry points (spt_occluded_rays, spt_occluded_rays_async):
declared in include/spt_hip.h, exported by the library, bound by _native with the declared
argument types, and a null context is an argument error before any device is touched.  The
ABI version stays 11: the entry points are additions.  The blocking form's staging plan is
pinned by tests/cpp/occlude_plan_check.cpp.  (What they compute: tests/test_gpu_occlusion.py.)"""
import ctypes
import os
import re
import subprocess

NAMES = ("spt_occluded_rays_async", "spt_occluded_rays")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_occlusion_entry_points_are_declared_and_exported(native):
    declared = native.declared_symbols()
    L = native.lib()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.spt_abi_version() == native.ABI_VERSION == 11
    header = open(native.HEADER_PATH).read()
    assert re.search(r"^#define SPT_OCCLUDE_SEGMENTS 1u$", header, re.M)
    assert re.search(r"^#define SPT_ABI_VERSION 11$", header, re.M)
    assert native.OCCLUDE_SEGMENTS == 1


def test_native_binds_the_occlusion_signatures(native):
    L = native.lib()
    P, u32, f32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_float
    # (ctx, a4, b4, limits, n, flags, scale, occ[, stream])
    assert L.spt_occluded_rays_async.argtypes == [P, P, P, P, u32, u32, f32, P, P]
    assert L.spt_occluded_rays.argtypes == [P, P, P, P, u32, u32, f32, P]
    for name in NAMES:
        assert getattr(L, name).restype == ctypes.c_int
    # as the header declares them: pointers, then n and flags, the scale, the answer
    header = re.sub(r"/\*.*?\*/", "", open(native.HEADER_PATH).read(), flags=re.S)
    for name, tail in (("spt_occluded_rays_async", r"void \*d_occ , void \*stream"), ("spt_occluded_rays", r"uint8_t \*occ")):
        m = re.search(r"SPT_API int " + name + r"\(([^)]*)\)", header)
        assert m, name
        args = re.sub(r"\s+", " ", m.group(1))
        assert re.search(r"uint32_t n, uint32_t flags, float scale, " + tail + "$", args), args


def test_null_context_is_an_argument_error(native):
    L = native.lib()
    buf = (ctypes.c_float * 8)()
    occ = (ctypes.c_uint8 * 3)()
    for call in (lambda: L.spt_occluded_rays(None, buf, buf, None, 1, 0, 1.0, occ),
                 lambda: L.spt_occluded_rays_async(None, buf, buf, None, 1, 0, 1.0, occ, None),
                 lambda: L.spt_occluded_rays(None, buf, buf, None, 1, 1, 1.0, occ),
                 lambda: L.spt_occluded_rays(None, None, None, None, 0, 0, 1.0, None)):
        assert call() == 1
        assert b"null" in L.spt_last_error(None)
    assert list(occ) == [0, 0, 0]


def test_python_interface_has_the_occlusion_queries(native):
    from simplepathtracer_amd.renderer import Context
    for name in ("occluded", "visible", "occluded_async"):
        assert callable(getattr(Context, name)), name


def test_occlusion_staging_plan(tmp_path):
    """occluded_rays_plan (spt_staging.h) in tests/cpp/occlude_plan_check.cpp: plain g++, a
    program of its own, AddressSanitizer + UBSan linked into the executable."""
    exe = tmp_path / "occlude_plan_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-I", os.path.join(ROOT, "simplepathtracer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "occlude_plan_check.cpp"), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stdout + out.stderr
