"""ctypes binding of the CPU restatement (oracle/spt_oracle.c).

TEST INFRASTRUCTURE ONLY: imported by tests/, __graft_entry__.smoke() and
bench.py's cpu_baseline leg, never by the product package.  See spt_oracle.h for
what is pinned against the reference's own code and what is not.

The ref_* functions run the reference's own functions through oracle/_ref/ref_harness
(`make -C oracle ref`, built where the reference's headers are present), one process and
one request per call, under a time limit.  run_dropin_main / run_dropin_driver run the
reference's application against the drop-in shim (oracle/_ref/ref_dropin_main and
ref_dropin_driver, same target; they need a GPU), a fresh process per call.
"""
from __future__ import annotations

import ctypes
import os
import struct
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "build", "libspt_oracle.so")

REF_BIN = os.path.join(HERE, "_ref", "ref_harness")
# the reference's include/ directory on the build machine (the Makefile's default too)
REF_INCLUDE = os.environ.get("REF_INCLUDE", "/root/reference/include")
REF_TIMEOUT = 60.0
REF_WIDTH = REF_HEIGHT = 1440  # Globals.hpp: constexpr, as are 100 spp and 10 bounces
REF_SPP, REF_BOUNCES = 100, 10

SKYBOX, REFLECTIVE, REFRACTIVE, DIFFUSE = 0, 1, 2, 3
# spo_trace_ray's info: [specular events, cut at the cap] + the SPO_EV_* counters
EV = ("diffuse", "mirror", "glass_reflect", "refract_twice", "tir", "end_bounces", "end_sky", "cut")
TRACE_INFO = 2 + len(EV)


class Scene(ctypes.Structure):
    _fields_ = [
        ("n", ctypes.c_uint32),
        ("centers", ctypes.c_void_p),
        ("radii", ctypes.c_void_p),
        ("colors", ctypes.c_void_p),
        ("materials", ctypes.c_void_p),
        ("fuzz", ctypes.c_void_p),
    ]


class Frame(ctypes.Structure):
    _fields_ = [
        ("view", ctypes.c_float * 16),
        ("eye", ctypes.c_float * 4),
        ("sky", ctypes.c_float * 4),
        ("width", ctypes.c_uint32),
        ("height", ctypes.c_uint32),
        ("spp", ctypes.c_uint32),
        ("bounces", ctypes.c_uint32),
        ("seed", ctypes.c_uint64),
    ]


def build() -> None:
    subprocess.run(["make", "-s", "-C", HERE], check=True)


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            build()
        L = ctypes.CDLL(LIB_PATH)
        P = ctypes.c_void_p
        u32, u64, f32 = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_float
        L.spo_next_u32.argtypes = [P]; L.spo_next_u32.restype = u32
        L.spo_uniform.argtypes = [P, f32, f32]; L.spo_uniform.restype = f32
        L.spo_uniform_u32.argtypes = [u32, f32, f32]; L.spo_uniform_u32.restype = f32
        L.spo_sample_key.argtypes = [u64, u32, u32]; L.spo_sample_key.restype = u64
        L.spo_scene_state.argtypes = [u32]; L.spo_scene_state.restype = u64
        L.spo_ball_vector.argtypes = [P, P]; L.spo_ball_vector.restype = None
        L.spo_camera_basis.argtypes = [P, P, P, P]; L.spo_camera_basis.restype = None
        L.spo_find_closest.argtypes = [P, P, P]; L.spo_find_closest.restype = u32
        L.spo_write_pixel.argtypes = [P, P]; L.spo_write_pixel.restype = None
        L.spo_trace_sample.argtypes = [P, P, u32, u32, u32, ctypes.c_int, P]; L.spo_trace_sample.restype = u32
        L.spo_trace_sample_info.argtypes = [P, P, u32, u32, u32, ctypes.c_int, P, P]
        L.spo_trace_sample_info.restype = u32
        L.spo_probe_sphere.argtypes = [P, u32, P, P, P]; L.spo_probe_sphere.restype = ctypes.c_int
        L.spo_schlick_log.argtypes = [P, u32]; L.spo_schlick_log.restype = u32
        L.spo_primary_winners.argtypes = [P, P, P, u32, P]; L.spo_primary_winners.restype = None
        for fn in (L.spo_render_segment, L.spo_render_segment_task):
            fn.argtypes = [P, P, u32, u32, u32, u32, P, P]; fn.restype = u64
        L.spo_render_image_parallel.argtypes = [P, P, u32, ctypes.c_int, P, P]
        L.spo_render_image_parallel.restype = ctypes.c_int
        L.spo_primary_ray.argtypes = [P, u32, u32, P, P]; L.spo_primary_ray.restype = None
        L.spo_trace_ray.argtypes = [P, P, P, P, u32, P, P, P]; L.spo_trace_ray.restype = u32
        L.spo_render_segment_stream.argtypes = [P, P, u32, u32, u32, u32, P, P, P]
        L.spo_render_segment_stream.restype = u64
        L.spo_render_segment_task_stream.argtypes = [P, P, u32, u32, u32, u32, P, P, P, P]
        L.spo_render_segment_task_stream.restype = u64
        L.spo_generate_spheres.argtypes = [u32, u32, P, P, P, P, P]; L.spo_generate_spheres.restype = u32
        L.spo_init_spheres.argtypes = [u32, P, P, P, P, P]; L.spo_init_spheres.restype = u32
        L.spo_math_block.argtypes = [ctypes.c_int, u32, u64, P]; L.spo_math_block.restype = ctypes.c_int
        L.spo_math_digest.argtypes = [ctypes.c_int, u32, u64, P]; L.spo_math_digest.restype = ctypes.c_int
        _lib = L
    return _lib


def _p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


class OracleScene:
    """Keeps numpy arrays alive behind a spo_scene struct."""

    def __init__(self, centers, radii, colors, materials, fuzz):
        n = len(radii)
        self.centers = np.ascontiguousarray(np.asarray(centers, np.float32).reshape(n, 4))
        self.radii = np.ascontiguousarray(np.asarray(radii, np.float32).reshape(n))
        self.colors = np.ascontiguousarray(np.asarray(colors, np.float32).reshape(n, 4))
        self.materials = np.ascontiguousarray(np.asarray(materials, np.uint8).reshape(n))
        self.fuzz = np.ascontiguousarray(np.asarray(fuzz, np.float32).reshape(n))
        self.s = Scene(n, _p(self.centers), _p(self.radii), _p(self.colors), _p(self.materials), _p(self.fuzz))

    @property
    def ref(self):
        return ctypes.byref(self.s)


def make_frame(view, eye, sky, width, height, spp, bounces, seed) -> Frame:
    f = Frame()
    f.view[:] = [float(v) for v in np.asarray(view, np.float32).reshape(16)]
    f.eye[:] = [float(v) for v in np.asarray(eye, np.float32).reshape(4)]
    f.sky[:] = [float(v) for v in np.asarray(sky, np.float32).reshape(4)]
    f.width, f.height, f.spp, f.bounces, f.seed = width, height, spp, bounces, seed
    return f


def generate_spheres(seed: int, cap: int = 4096):
    c = np.zeros((cap, 4), np.float32); r = np.zeros(cap, np.float32); col = np.zeros((cap, 4), np.float32)
    m = np.zeros(cap, np.uint8); fz = np.zeros(cap, np.float32)
    n = lib().spo_generate_spheres(seed, cap, _p(c), _p(r), _p(col), _p(m), _p(fz))
    return OracleScene(c[:n], r[:n], col[:n], m[:n], fz[:n])


def init_spheres(seed: int):
    c = np.zeros((10, 4), np.float32); r = np.zeros(10, np.float32); col = np.zeros((10, 4), np.float32)
    m = np.zeros(10, np.uint8); fz = np.zeros(10, np.float32)
    n = lib().spo_init_spheres(seed, _p(c), _p(r), _p(col), _p(m), _p(fz))
    return OracleScene(c[:n], r[:n], col[:n], m[:n], fz[:n])


def camera_basis(eye, look_at, up):
    out = np.zeros(16, np.float32)
    e = np.asarray(eye, np.float32); l = np.asarray(look_at, np.float32); u = np.asarray(up, np.float32)
    lib().spo_camera_basis(_p(e), _p(l), _p(u), _p(out))
    return out


def render_segment(scene: OracleScene, frame: Frame, yB, yE, xB, xE, task=False, rgb8=None):
    rgba = np.zeros(((yE - yB) * (xE - xB), 4), np.float32)
    fn = lib().spo_render_segment_task if task else lib().spo_render_segment
    casts = fn(scene.ref, ctypes.byref(frame), yB, yE, xB, xE, _p(rgba), _p(rgb8) if rgb8 is not None else None)
    return rgba, casts


def render_image_parallel(scene: OracleScene, frame: Frame, thread_count: int, mode: int = 0, want_rgba=True):
    rgba = np.zeros((frame.height * frame.width, 4), np.float32) if want_rgba else None
    rgb8 = np.zeros(frame.width * frame.height * 3, np.uint8)
    rc = lib().spo_render_image_parallel(scene.ref, ctypes.byref(frame), thread_count, mode,
                                         _p(rgba) if rgba is not None else None, _p(rgb8))
    if rc != 0:
        raise RuntimeError("spo_render_image_parallel failed")
    return rgba, rgb8


def trace_sample(scene: OracleScene, frame: Frame, x, y, s, task=False):
    out = np.zeros(4, np.float32)
    casts = lib().spo_trace_sample(scene.ref, ctypes.byref(frame), x, y, s, int(task), _p(out))
    return out, casts


def trace_sample_info(scene: OracleScene, frame: Frame, x, y, s, task=False):
    """trace_sample, and the path's specular-event count and task-mode dropped flag."""
    out = np.zeros(4, np.float32)
    info = np.zeros(2, np.uint32)
    casts = lib().spo_trace_sample_info(scene.ref, ctypes.byref(frame), x, y, s, int(task), _p(out), _p(info))
    return out, casts, int(info[0]), bool(info[1])


def trace_region(scene: OracleScene, frame: Frame, yB, yE, xB, xE, task=False):
    """Every sample of a region: colours (pixels, spp, 4), and per sample the ray count,
    the specular-event count and the dropped flag (each (pixels, spp))."""
    n, spp = (yE - yB) * (xE - xB), frame.spp
    col = np.zeros((n, spp, 4), np.float32)
    casts = np.zeros((n, spp), np.uint32)
    info = np.zeros((n, spp, 2), np.uint32)
    fn, sc, fr = lib().spo_trace_sample_info, scene.ref, ctypes.byref(frame)
    f4, u4 = col.strides[1], info.strides[1]
    pc, pi = col.ctypes.data, info.ctypes.data
    for p in range(n):
        y, x = yB + p // (xE - xB), xB + p % (xE - xB)
        for s in range(spp):
            k = p * spp + s
            casts[p, s] = fn(sc, fr, x, y, s, int(task), pc + k * f4, pi + k * u4)
    return col, casts, info[:, :, 0], info[:, :, 1].astype(bool)


def probe_sphere(scene: OracleScene, i, d, o):
    """Sphere i alone on the ray (o, d): (RaySphereIntersection passes, squared distance
    find_closest would compare, contact ahead of the origin)."""
    d = np.ascontiguousarray(d, np.float32); o = np.ascontiguousarray(o, np.float32)
    out = np.zeros(2, np.float32)
    ok = lib().spo_probe_sphere(scene.ref, int(i), _p(d), _p(o), _p(out))
    return bool(ok), out[0], bool(out[1])


def find_closest(scene: OracleScene, d, o) -> int:
    d = np.ascontiguousarray(d, np.float32); o = np.ascontiguousarray(o, np.float32)
    return int(lib().spo_find_closest(scene.ref, _p(d), _p(o)))


def schlick_bases(fn, cap=1 << 20) -> np.ndarray:
    """The 1 - c arguments of every Schlick powf(1 - c, 5) the oracle evaluates while fn()
    runs on this thread."""
    buf = np.zeros(cap, np.float32)
    lib().spo_schlick_log(_p(buf), cap)
    try:
        fn()
    finally:
        n = lib().spo_schlick_log(None, 0)
    return buf[:min(n, cap)]


def primary_winners(scene: OracleScene, frame: Frame, xys) -> np.ndarray:
    """Closest sphere (index; scene.n = none) of the primary ray of each (x, y, s) row."""
    xys = np.ascontiguousarray(xys, np.uint32)
    out = np.zeros(len(xys), np.uint32)
    lib().spo_primary_winners(scene.ref, ctypes.byref(frame), _p(xys), len(xys), _p(out))
    return out


def scene_state(seed: int) -> int:
    """The state a reference thread's generator starts from when its clock reads `seed`."""
    return int(lib().spo_scene_state(seed & 0xFFFFFFFF))


def uniform_draws(seed: int, a: float, b: float, count: int) -> np.ndarray:
    st = ctypes.c_uint64(scene_state(seed))
    return np.array([lib().spo_uniform(ctypes.byref(st), a, b) for _ in range(count)], np.float32)


MATH_BLOCK = 1 << 20  # SPO_MATH_BLOCK


def math_block(op: int, first: int, count: int) -> np.ndarray:
    """Result bits of scalar primitive `op` (SPO_MATH_*) on the input patterns
    first ... first + count - 1 (mod 2^32)."""
    out = np.empty(count, np.uint32)
    if lib().spo_math_block(op, first, count, _p(out)) != 0:
        raise ValueError(f"spo_math_block({op}, {first:#x}, {count})")
    return out


def math_digest(op: int, first: int, count: int) -> np.ndarray:
    """One digest per block of 2^20 of those patterns (spt_oracle.h)."""
    out = np.empty((count + MATH_BLOCK - 1) // MATH_BLOCK, np.uint64)
    if lib().spo_math_digest(op, first, count, _p(out)) != 0:
        raise ValueError(f"spo_math_digest({op}, {first:#x}, {count})")
    return out


def primary_rays(frame: Frame, xy, seed: int) -> np.ndarray:
    """Directions (n, 4) of one primary ray per (x, y) row, the jitter drawn from one stream
    that starts at scene_state(seed)."""
    out = np.zeros((len(xy), 4), np.float32)
    st = ctypes.c_uint64(scene_state(seed))
    for i, (x, y) in enumerate(xy):
        lib().spo_primary_ray(ctypes.byref(frame), int(x), int(y), ctypes.byref(st), out.ctypes.data + 16 * i)
    return out


def trace_rays(scene: OracleScene, frame: Frame, d, o, bounces, seeds):
    """spo_trace_ray per row: path i starts from (o[i], d[i]) with bounces[i] and draws from
    the stream scene_state(seeds[i]).  Returns colours (n, 4) and info (n, TRACE_INFO)."""
    d = np.ascontiguousarray(d, np.float32); o = np.ascontiguousarray(o, np.float32)
    n = len(d)
    out = np.zeros((n, 4), np.float32)
    info = np.zeros((n, TRACE_INFO), np.uint32)
    fn, sc, fr = lib().spo_trace_ray, scene.ref, ctypes.byref(frame)
    st = ctypes.c_uint64(0)
    pst = ctypes.byref(st)
    for i in range(n):
        st.value = scene_state(int(seeds[i]))
        fn(sc, fr, d.ctypes.data + 16 * i, o.ctypes.data + 16 * i, int(bounces[i]), pst, out.ctypes.data + 16 * i,
           info.ctypes.data + 4 * TRACE_INFO * i)
    return out, info


def render_segment_stream(scene: OracleScene, frame: Frame, yB, yE, xB, xE, seed, task=False):
    """RenderSegment / RenderSegmentTask on one sequential stream that starts at
    scene_state(seed).  Returns (rgba of the region, the frame's g_data, samples dropped by
    the pass cap (task mode; else 0))."""
    rgba = np.zeros(((yE - yB) * (xE - xB), 4), np.float32)
    rgb8 = np.zeros(frame.width * frame.height * 3, np.uint8)
    st = ctypes.c_uint64(scene_state(seed))
    dropped = ctypes.c_uint64(0)
    if task:
        lib().spo_render_segment_task_stream(scene.ref, ctypes.byref(frame), yB, yE, xB, xE, ctypes.byref(st), _p(rgba),
                                             _p(rgb8), ctypes.byref(dropped))
    else:
        lib().spo_render_segment_stream(scene.ref, ctypes.byref(frame), yB, yE, xB, xE, ctypes.byref(st), _p(rgba),
                                        _p(rgb8))
    return rgba, rgb8, int(dropped.value)


# ---------------------------------------------------------------- the reference's own code

def ref_available() -> bool:
    return os.path.exists(REF_BIN)


def _ref_call(request: bytes) -> bytes:
    """One request to a fresh ref_harness process; raises on a non-zero exit or the time limit."""
    with tempfile.TemporaryDirectory(prefix="spt_ref_") as tmp:
        req, rsp = os.path.join(tmp, "request"), os.path.join(tmp, "response")
        with open(req, "wb") as f:
            f.write(request)
        r = subprocess.run([REF_BIN, req, rsp], capture_output=True, text=True, timeout=REF_TIMEOUT)
        if r.returncode != 0:
            raise RuntimeError(f"ref_harness exit {r.returncode}: {r.stderr.strip()}")
        with open(rsp, "rb") as f:
            return f.read()


def _scene_bytes(scene: OracleScene) -> bytes:
    c, col = scene.centers.copy(), scene.colors.copy()
    c[:, 3] = 0
    col[:, 3] = 0
    return (struct.pack("<I", scene.s.n) + c.tobytes() + scene.radii.tobytes() + col.tobytes()
            + scene.materials.tobytes() + scene.fuzz.tobytes())


def _scene_from(buf: bytes, at: int = 0):
    n = struct.unpack_from("<I", buf, at)[0]
    at += 4
    def take(dtype, count):
        nonlocal at
        a = np.frombuffer(buf, dtype, count, at).copy()
        at += a.nbytes
        return a
    c = take(np.float32, 4 * n).reshape(n, 4); r = take(np.float32, n); col = take(np.float32, 4 * n).reshape(n, 4)
    m = take(np.uint8, n); fz = take(np.float32, n)
    return OracleScene(c, r, col, m, fz), at


def ref_draws(seed: int, a: float, b: float, count: int) -> np.ndarray:
    """The first `count` random::GenerateUniformRealDist(a, b) of a fresh thread seeded `seed`."""
    return np.frombuffer(_ref_call(struct.pack("<IIffI", 1, seed, a, b, count)), np.float32).copy()


def ref_generate(seed: int, init: bool = False) -> OracleScene:
    """GenerateSpheres() (init: InitSpheres()) on a fresh thread seeded `seed`; fuzz = g_diffuses."""
    sc, _ = _scene_from(_ref_call(struct.pack("<III", 2, int(init), seed)))
    return sc


def ref_camera(eye, look_at, up) -> np.ndarray:
    """Transpose(CreateCameraBasisMatrix(eye, look_at, up)), 16 floats."""
    v = np.concatenate([np.asarray(a, np.float32)[:3] for a in (eye, look_at, up)])
    return np.frombuffer(_ref_call(struct.pack("<I", 3) + v.tobytes()), np.float32).copy()


def ref_geometry(scene: OracleScene, o, d, aim):
    """Per ray: FindClosestIntersectionSphere (uint32); for hits the ten floats
    ClosestContactPoint (4), its factor t, ContactNormal (4), LengthSquared(o - P) (zeros on
    a miss); RaySphereIntersection of sphere aim[i] (False where aim[i] < 0)."""
    o = np.ascontiguousarray(o, np.float32); d = np.ascontiguousarray(d, np.float32)
    aim = np.ascontiguousarray(aim, np.int32)
    n = len(o)
    buf = _ref_call(struct.pack("<I", 4) + _scene_bytes(scene) + struct.pack("<I", n) + o.tobytes() + d.tobytes()
                    + aim.tobytes())
    idx = np.frombuffer(buf, np.uint32, n, 0).copy()
    rec = np.frombuffer(buf, np.float32, 10 * n, 4 * n).reshape(n, 10).copy()
    rsi = np.frombuffer(buf, np.uint8, n, 44 * n).astype(bool)
    return idx, rec, rsi


def ref_trace(scene: OracleScene, d, o, bounces, seeds) -> np.ndarray:
    """TraceAndSampleColor(d[i], o[i], bounces[i]), each on a fresh thread seeded seeds[i]:
    colours (n, 4)."""
    d = np.ascontiguousarray(d, np.float32); o = np.ascontiguousarray(o, np.float32)
    n = len(d)
    rec = np.zeros(n, np.dtype([("d", "<f4", 4), ("o", "<f4", 4), ("b", "<u4"), ("s", "<u4")]))
    rec["d"], rec["o"], rec["b"], rec["s"] = d, o, bounces, seeds
    buf = _ref_call(struct.pack("<I", 5) + _scene_bytes(scene) + struct.pack("<I", n) + rec.tobytes())
    return np.frombuffer(buf, np.float32, 4 * n).reshape(n, 4).copy()


def ref_segment(scene: OracleScene, view, eye, yB, yE, xB, xE, seed, task=False):
    """RenderSegment (task: RenderSegmentTask) of the 1440 x 1440 frame at 100 spp and 10
    bounces on a fresh thread seeded `seed`.  Returns (indices, colours (k, 4)) as handed to
    io::WritePixel, in call order, and the whole g_data (zero before the call)."""
    req = (struct.pack("<I", 6) + _scene_bytes(scene) + np.asarray(view, np.float32).reshape(16).tobytes()
           + np.asarray(eye, np.float32).reshape(4).tobytes() + struct.pack("<IIIIII", int(task), seed, yB, yE, xB, xE))
    buf = _ref_call(req)
    k = struct.unpack_from("<I", buf, 0)[0]
    taps = np.frombuffer(buf, np.dtype([("index", "<u4"), ("color", "<f4", 4)]), k, 4)
    g = np.frombuffer(buf, np.uint8, REF_WIDTH * REF_HEIGHT * 3, 4 + 20 * k).copy()
    return taps["index"].copy(), taps["color"].copy(), g


# ------------------------------------------- the reference's application against the shim

# oracle/_ref/ref_dropin_main is the reference's Main.cpp itself, ref_dropin_driver our
# driver around its Renderer.hpp (oracle/ref_dropin_driver.cpp); both are built with
# include/dropin in front of the reference's headers and link libspt_hip.so: they need a GPU.
DROPIN_MAIN = os.path.join(HERE, "_ref", "ref_dropin_main")
DROPIN_DRIVER = os.path.join(HERE, "_ref", "ref_dropin_driver")
DROPIN_TIMEOUT = 300.0  # of tests/test_gpu_parity.py's shim test
HIP_ILLEGAL_ACCESS = "an illegal memory access was encountered"
# Set once a child has ended by a signal, run into the time limit or printed HIP's
# illegal-access error: the tests of tests/test_gpu_dropin_reference.py then skip, so that
# nothing more is started on a GPU that may have faulted.
dropin_fault = None


class DropinRun:
    """One child process: its exit status, what it printed, the recorded stbi_write_bmp
    arguments [(file name, w, h, comp), ...] and the dumped frames (uint8 arrays), in call
    order."""

    def __init__(self, returncode, output, saves, dumps):
        self.returncode, self.output, self.saves, self.dumps = returncode, output, saves, dumps


def dropin_available() -> bool:
    return os.path.exists(DROPIN_MAIN) and os.path.exists(DROPIN_DRIVER)


def dropin_deps(binary: str):
    """The prerequisites in the dependency file the compiler left beside a _ref/ binary, as
    absolute normalised paths; the first is the translation unit.  The file's relative
    paths are relative to oracle/, where make ran."""
    with open(binary + ".d") as f:
        text = f.read().replace("\\\n", " ")
    return [os.path.normpath(os.path.join(HERE, p)) for p in text.split(":", 1)[1].split()]


def dropin_shadowing_errors(binary: str):
    """What is wrong with a binary's include graph (an empty list: nothing): it must hold the
    four drop-in headers of this tree and the reference's Renderer.hpp, Globals.hpp,
    Definitions.hpp, Math.hpp, IOHelpers.hpp and SceneGenerators.hpp, all from one directory
    outside this tree, and nothing else named like the two tracers or Collision.hpp."""
    root = os.path.dirname(HERE)
    deps = dropin_deps(binary)
    errors = []
    for rel in ("include/dropin/SingleThreadPathTracer.hpp", "include/dropin/TaskBasedPathTracer.hpp",
                "include/spt/RenderSegmentShim.hpp", "include/spt_hip.h"):
        if os.path.join(root, rel) not in deps:
            errors.append(f"{rel} is not included")
    ref_dirs = {os.path.dirname(p) for p in deps if os.path.basename(p) == "Renderer.hpp"}
    if len(ref_dirs) != 1 or next(iter(ref_dirs)).startswith(root + os.sep):
        return errors + [f"Renderer.hpp comes from {sorted(ref_dirs)}"]
    ref_dir = next(iter(ref_dirs))
    for name in ("Globals.hpp", "Definitions.hpp", "Math.hpp", "IOHelpers.hpp", "SceneGenerators.hpp"):
        if os.path.join(ref_dir, name) not in deps:
            errors.append(f"the reference's {name} is not included")
    for name in ("SingleThreadPathTracer.hpp", "TaskBasedPathTracer.hpp", "Collision.hpp"):
        for p in deps:
            if os.path.basename(p) == name and not p.startswith(os.path.join(root, "include") + os.sep):
                errors.append(f"{p} is included: the reference's {name} is not shadowed")
    return errors


def _run_dropin(argv, seed, dump, env, tmp):
    global dropin_fault
    dump = dump or os.path.join(tmp, "g_data")
    e = dict(os.environ)
    e.update(env or {})
    e["SPT_REF_CLOCK_SEED"] = str(seed)
    e["SPT_REF_DUMP"] = dump
    try:
        # cwd: the reference opens shaders/ relative to it (absent: empty sources, as headless
        # GL does not care) and must find no stray file
        r = subprocess.run(argv, capture_output=True, text=True, errors="replace", timeout=DROPIN_TIMEOUT, env=e, cwd=tmp)
    except subprocess.TimeoutExpired:
        dropin_fault = f"{os.path.basename(argv[0])} ran into the {DROPIN_TIMEOUT:.0f} s limit"
        raise
    out = r.stdout + r.stderr
    if r.returncode < 0:
        dropin_fault = f"{os.path.basename(argv[0])} ended by signal {-r.returncode}"
    elif HIP_ILLEGAL_ACCESS in out:
        dropin_fault = f"{os.path.basename(argv[0])} printed HIP's illegal-access error"
    saves, dumps = [], []
    k = 1
    while os.path.exists(f"{dump}.{k}.args"):
        with open(f"{dump}.{k}.args") as f:
            name, w, h, comp = f.read().splitlines()
        saves.append((name, int(w), int(h), int(comp)))
        dumps.append(np.fromfile(f"{dump}.{k}", np.uint8))
        k += 1
    return DropinRun(r.returncode, out, saves, dumps)


def run_dropin_main(seed: int, dump=None, env=None) -> DropinRun:
    """The reference's Main.cpp in a fresh process, its clock reading `seed`.  dump: the path
    whose .<k> and .<k>.args files the saved frames are left in (default: not kept)."""
    with tempfile.TemporaryDirectory(prefix="spt_dropin_") as tmp:
        return _run_dropin([DROPIN_MAIN], seed, dump, env, tmp)


def run_dropin_driver(mode: str, scene: str = "random", seed: int = 1, dump=None, env=None, pixels=None, origins=None,
                      dirs=None):
    """ref_dropin_driver in a fresh process.  mode "image" or "frames" with scene "init" or
    "random": the DropinRun.  mode "pick" (the `random` scene): (run, PickSphere of every
    (x, y) row of pixels, FindClosestIntersectionSpheres of the rays), the two None where
    the process failed."""
    with tempfile.TemporaryDirectory(prefix="spt_dropin_") as tmp:
        if mode != "pick":
            return _run_dropin([DROPIN_DRIVER, mode, scene], seed, dump, env, tmp)
        xy = np.ascontiguousarray(pixels, "<u4").reshape(-1, 2)
        o = np.ascontiguousarray(origins, "<f4").reshape(-1, 4)
        d = np.ascontiguousarray(dirs, "<f4").reshape(-1, 4)
        assert len(o) == len(d)
        req, rsp = os.path.join(tmp, "request"), os.path.join(tmp, "response")
        with open(req, "wb") as f:
            f.write(struct.pack("<I", len(xy)) + xy.tobytes() + struct.pack("<I", len(o)) + o.tobytes() + d.tobytes())
        run = _run_dropin([DROPIN_DRIVER, "pick", req, rsp], seed, dump, env, tmp)
        if run.returncode != 0 or not os.path.exists(rsp):
            return run, None, None
        idx = np.fromfile(rsp, "<u4")
        assert idx.size == len(xy) + len(o), f"response of {idx.size} indices for {len(xy)} pixels and {len(o)} rays"
        return run, idx[:len(xy)].copy(), idx[len(xy):].copy()
