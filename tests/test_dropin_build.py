"""The headless build of the reference's application against the drop-in shim (CPU side).

`make -C oracle ref` (run by build() where the reference's headers are present) compiles
the reference's unmodified Main.cpp (oracle/_ref/ref_dropin_main) and our driver around its
Renderer.hpp (oracle/_ref/ref_dropin_driver) behind the stand-ins of
oracle/ref_app_standins/ and oracle/ref_standins/, with include/dropin in front of the
reference's include directory, and links them against libspt_hip.so.  Here: that both were
built, and -- from the dependency files the compiler left beside them -- that the drop-in
headers really shadow the reference's two tracers.  Nothing of the reference is read: the
dependency files name its headers, no more.

The binaries are not run: without a device they end in abort() at spt_ctx_create.  The GPU
side is tests/test_gpu_dropin_reference.py; that ref_harness still builds and answers as
before is tests/test_reference_parity.py, unchanged.

Where neither the binaries nor the reference's headers exist the tests skip; where the
headers exist and a binary does not, they fail (the convention of test_reference_parity).
"""
import os

import pytest

BINARIES = ("ref_dropin_main", "ref_dropin_driver")


@pytest.fixture(scope="module")
def dropin(oracle):
    missing = [p for p in (oracle.DROPIN_MAIN, oracle.DROPIN_DRIVER) if not os.path.exists(p)]
    if missing:
        if os.path.isdir(oracle.REF_INCLUDE):
            pytest.fail(f"the reference's headers are in {oracle.REF_INCLUDE} but {missing} is not built")
        pytest.skip("neither the reference's headers nor oracle/_ref/ref_dropin_main and ref_dropin_driver are here")
    return oracle


def binary(oracle, name):
    return {"ref_dropin_main": oracle.DROPIN_MAIN, "ref_dropin_driver": oracle.DROPIN_DRIVER}[name]


def test_both_binaries_exist(dropin):
    assert dropin.dropin_available()
    for name in BINARIES:
        path = binary(dropin, name)
        assert os.access(path, os.X_OK), path
        assert os.path.exists(path + ".d"), f"no dependency file beside {path}"


@pytest.mark.parametrize("name", BINARIES)
def test_dropin_headers_shadow_the_reference_tracers(dropin, name):
    """The include graph holds the four drop-in headers and the reference's Renderer.hpp,
    Globals.hpp, Definitions.hpp, Math.hpp, IOHelpers.hpp and SceneGenerators.hpp, and none
    of the reference's SingleThreadPathTracer.hpp, TaskBasedPathTracer.hpp, Collision.hpp."""
    errors = dropin.dropin_shadowing_errors(binary(dropin, name))
    assert not errors, errors


def test_stand_in_layers(dropin):
    """Each binary saw the application stand-ins first and ref_standins/intrin.h behind
    them (whose macros the prelude must precede)."""
    here = os.path.dirname(os.path.abspath(dropin.__file__))
    for name in BINARIES:
        deps = dropin.dropin_deps(binary(dropin, name))
        for rel in ("ref_app_standins/intrin.h", "ref_standins/intrin.h", "ref_app_standins/GL.hpp",
                    "ref_app_standins/glbinding/gl46ext/gl.h", "ref_app_standins/glbinding/Binding.h",
                    "ref_app_standins/GLFW/glfw3.h", "ref_app_standins/stb_image_write.h"):
            assert os.path.join(here, rel) in deps, (name, rel)
        assert deps.index(os.path.join(here, "ref_app_standins/intrin.h")) < deps.index(
            os.path.join(here, "ref_standins/intrin.h"))
        for rel in ("ref_standins/GLFW/glfw3.h", "ref_standins/stb_image_write.h", "ref_standins/glbinding/gl46ext/gl.h"):
            assert os.path.join(here, rel) not in deps, (name, rel)


def test_sources(dropin):
    """ref_dropin_main's only source is the reference's Main.cpp, beside its include
    directory; the driver's is ours."""
    here = os.path.dirname(os.path.abspath(dropin.__file__))
    root = os.path.dirname(here)
    deps = dropin.dropin_deps(dropin.DROPIN_MAIN)
    sources = [p for p in deps if p.endswith((".cpp", ".cc", ".c", ".cxx"))]
    assert sources == [deps[0]] and os.path.basename(deps[0]) == "Main.cpp", sources
    assert not deps[0].startswith(root + os.sep), deps[0]
    ref_include = os.path.dirname(next(p for p in deps if os.path.basename(p) == "Renderer.hpp"))
    assert os.path.dirname(deps[0]) == os.path.dirname(ref_include), (deps[0], ref_include)
    deps = dropin.dropin_deps(dropin.DROPIN_DRIVER)
    sources = [p for p in deps if p.endswith((".cpp", ".cc", ".c", ".cxx"))]
    assert sources == [os.path.join(here, "ref_dropin_driver.cpp")], sources
