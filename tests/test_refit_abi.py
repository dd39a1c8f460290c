"""CPU tests of the scene-update entry points (include/spt_hip.h "scene updates", DESIGN.md
§4.16): spt_update_scene, spt_accel_refit_check and spt_prim_lists_read are declared, exported
and bound with the declared argument types, the ABI version stays 11, a null context is an
argument error before any device is touched; and the refit of the traversal tables itself,
through spt_accel_refit_check (host only): for every scene and move below the refit tables
pass the builder's own validation against the moved centres, keep every structure word, equal
the build byte for byte where the move is the identity, and refuse centres that are not
finite.  (What spt_update_scene computes on a device: tests/test_gpu_scene_update.py.)"""
import ctypes
import inspect
import re

import numpy as np
import pytest

NAMES = ("spt_update_scene", "spt_accel_refit_check", "spt_prim_lists_read")
F = np.float32
P = ctypes.c_void_p


def _p(a):
    return None if a is None else a.ctypes.data_as(P)


# ---------------------------------------------------------------- the ABI

def test_entry_points_are_declared_and_exported(native):
    declared = native.declared_symbols()
    L = native.lib()
    for name in NAMES:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.spt_abi_version() == native.ABI_VERSION == 11


def test_header_declares_the_signatures_bound(native):
    text = open(native.HEADER_PATH).read()
    kinds = {"uint32_t": ctypes.c_uint32, "int": ctypes.c_int}
    for name in NAMES:
        m = re.search(r"SPT_API int " + name + r"\(([^;]*)\);", text)
        assert m, name
        params = [re.sub(r"/\*.*?\*/", "", p).strip() for p in m.group(1).replace("\n", " ").split(",")]
        want = [P if "*" in p or "[" in p else kinds[p.split()[0]] for p in params]
        fn = getattr(native.lib(), name)
        assert fn.argtypes == want, (name, params)
        assert fn.restype == ctypes.c_int


def test_update_info_is_the_header_struct(native):
    text = open(native.HEADER_PATH).read()
    body = re.search(r"typedef struct spt_update_info \{(.*?)\} spt_update_info;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        words = decl.replace(",", " ").split()
        if words:
            fields += [(w, words[0]) for w in words[1:]]
    kinds = {"double": ctypes.c_double, "uint32_t": ctypes.c_uint32}
    assert [(n, kinds[t]) for n, t in fields] == list(native.UpdateInfo._fields_)
    assert [n for n, _ in fields][:6] == ["refit_ms", "lists_ms", "list_blocks", "list_entries", "lists_on_device", "refit"]
    assert ctypes.sizeof(native.UpdateInfo) == 40


def test_null_context_is_an_argument_error(native):
    L = native.lib()
    c, v, e = np.zeros((2, 4), F), np.eye(4, dtype=F).reshape(16), np.zeros(4, F)
    v[12:] = 0
    info = native.UpdateInfo()
    counts = np.zeros(4, np.uint32)
    for call in (lambda: L.spt_update_scene(None, _p(c), _p(v), _p(e), ctypes.byref(info)),
                 lambda: L.spt_update_scene(None, None, None, None, None),
                 lambda: L.spt_prim_lists_read(None, 0, None, None, None, None, 0, _p(counts)),
                 lambda: L.spt_prim_lists_read(None, 1, None, None, None, None, 0, None)):
        assert call() == 1
        assert b"null context" in L.spt_last_error(None)
    assert info.refit == 0 and info.lists_on_device == 0


def test_python_interface(native):
    import simplepathtracer_amd as spt
    par = lambda f: inspect.signature(f).parameters  # noqa: E731
    assert list(par(spt.Context.update_scene)) == ["self", "centers", "view", "eye"]
    assert all(par(spt.Context.update_scene)[k].default is None for k in ("centers", "view", "eye"))
    assert par(spt.TemporalAccumulator.__init__)["refit"].default is False
    assert par(spt.TemporalAccumulator.__init__)["resident"].default is False


# ---------------------------------------------------------------- the refit

def refit_check(native, a, b, radii, k, branching, refit=1):
    """(rc, tables) of spt_accel_refit_check: tables = dict(slots, orig, kpre, nodes, pre_cm, counts)."""
    L = native.lib()
    n = len(radii)
    a = np.ascontiguousarray(a, F)
    b = None if b is None else np.ascontiguousarray(b, F)
    r = np.ascontiguousarray(radii, F)
    counts = np.zeros(4, np.uint32)
    rc = L.spt_accel_refit_check(_p(a), _p(b), _p(r), n, k, branching, refit, _p(counts), None, None, None, None, None, 0, 0)
    if rc:
        return rc, None
    ns, nn = int(counts[0]), int(counts[1])
    t = dict(slots=np.zeros((ns, 4), F), orig=np.zeros(ns, np.uint32), kpre=np.zeros(ns, F),
             nodes=np.zeros((nn, 8), np.uint32), pre_cm=np.zeros(1, F), counts=counts)
    rc = L.spt_accel_refit_check(_p(a), _p(b), _p(r), n, k, branching, refit, _p(counts), _p(t["slots"]), _p(t["orig"]),
                                 _p(t["kpre"]), _p(t["nodes"]), _p(t["pre_cm"]), ns, nn)
    return rc, t


def same_bytes(x, y):
    return all(np.array_equal(x[k].view(np.uint8), y[k].view(np.uint8)) for k in ("slots", "orig", "kpre", "nodes", "pre_cm"))


def scenes(spt):
    """name -> (scene, cluster_k, branching): the default shape (8-member leaves, 4 children,
    3 above 512 spheres) and the flat list of 4-member clusters."""
    return {
        "spheres1": (spt.generate_spheres(1), 8, 4),
        "cornell3": (spt.cornell3(), 8, 4),
        "stress300": (spt.generate_stress(3, 300), 8, 4),
        "stress10000": (spt.generate_stress(1, 10000), 8, 3),
        "flat": (spt.generate_spheres(1), 4, 0),
    }


def moves(scene, seed=5):
    """name -> moved (n, 4) centres: a jitter of N(0, 0.05), a random permutation of the small
    spheres' centres (every small sphere jumps across the scene), one centre at 2e15."""
    rng = np.random.default_rng(seed)
    c = np.array(scene.centers, F, copy=True).reshape(scene.n, 4)
    small = np.flatnonzero(scene.radii <= 4 * np.median(scene.radii))
    jit = c.copy()
    jit[:, :3] += rng.normal(0.0, 0.05, (scene.n, 3)).astype(F)
    perm = c.copy()
    perm[small] = c[rng.permutation(small)]
    far = c.copy()
    far[small[len(small) // 2], 0] = F(2e15)
    return {"jitter": jit, "permutation": perm, "far": far}


SCENES = ("spheres1", "cornell3", "stress300", "stress10000", "flat")


@pytest.fixture(scope="module")
def built(native):
    """The build of every scene, once."""
    import simplepathtracer_amd as spt
    out = {}
    for name, (sc, k, br) in scenes(spt).items():
        a = np.array(sc.centers, F, copy=True).reshape(sc.n, 4)
        rc, t = refit_check(native, a, None, sc.radii, k, br, refit=0)
        assert rc == 0, native.lib().spt_last_error(None)
        out[name] = (sc, k, br, a, t)
    return out


@pytest.mark.parametrize("name", SCENES)
def test_identity_refit_equals_the_build_byte_for_byte(native, built, name):
    sc, k, br, a, t0 = built[name]
    rc, t = refit_check(native, a, a.copy(), sc.radii, k, br)
    assert rc == 0, native.lib().spt_last_error(None)
    assert same_bytes(t, t0) and np.array_equal(t["counts"], t0["counts"])
    if name in ("spheres1", "stress300", "stress10000"):
        assert t["counts"][2] > t["counts"][3] > 0  # a tree: inner nodes above the leaves
    if name == "flat":
        assert t["counts"][2] == t["counts"][3] > 0


@pytest.mark.parametrize("move", ("jitter", "permutation", "far"))
@pytest.mark.parametrize("name", SCENES)
def test_refit_validates_and_keeps_the_structure(native, built, name, move):
    sc, k, br, a, t0 = built[name]
    b = moves(sc)[move]
    assert not np.array_equal(a, b)
    rc, t = refit_check(native, a, b, sc.radii, k, br)  # runs validate_accel against b
    assert rc == 0, native.lib().spt_last_error(None)
    assert np.array_equal(t["orig"], t0["orig"])
    assert np.array_equal(t["nodes"][:, 4:6], t0["nodes"][:, 4:6])  # skip, slot
    real = t["orig"] != 0xFFFFFFFF
    assert np.array_equal(t["slots"][real, :3], b[t["orig"][real], :3])
    assert np.array_equal(t["slots"][:, 3].view(np.uint32), t0["slots"][:, 3].view(np.uint32))  # r*r stays
    if t["counts"][2] > 0:
        assert not same_bytes(t, t0)  # the bounds moved with the spheres
    if move == "far" and t["counts"][2] > 0:
        # past 1e15 the pretest and the node above the sphere never cull
        assert np.isinf(t["pre_cm"][0]) and (t["kpre"][real & (t["kpre"] != 0)] == -np.inf).all()
        assert np.isinf(t["nodes"][:, :4].view(F)).sum() > np.isinf(t0["nodes"][:, :4].view(F)).sum()  # beyond the pads


@pytest.mark.parametrize("name", ("spheres1", "flat", "cornell3"))
@pytest.mark.parametrize("bad", (np.nan, np.inf, -np.inf))
def test_a_centre_that_is_not_finite_is_refused(native, built, name, bad):
    sc, k, br, a, _ = built[name]
    b = a.copy()
    b[sc.n // 2, 1] = bad
    rc, _ = refit_check(native, a, b, sc.radii, k, br)
    assert rc == 1
    assert b"not finite" in native.lib().spt_last_error(None)
