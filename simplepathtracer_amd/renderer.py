"""Host-side mirror of the reference's render entry points over the HIP C ABI.

Reference interface (all state in globals, Globals.hpp:8-37):

    void RenderSegment(RenderSegmentData)       SingleThreadPathTracer.hpp:114-137
    void RenderSegmentTask(RenderSegmentData)   TaskBasedPathTracer.hpp:54-206
    RenderImageParallelMain()                   Renderer.hpp:257-302 (tile dispatch)
    RenderImage()                               Renderer.hpp:304-308

Here the globals live in a `Globals` object that owns a device context; the two
entry points keep their names and argument meaning (a pixel rectangle) and write
the reference's g_data byte layout.  Errors raise SptError (the reference has no
error channel).
"""
from __future__ import annotations

import ctypes
import threading
from dataclasses import dataclass

import numpy as np

from . import _native
from .scene import INIT_COLOR, DEFAULT_EYE, DEFAULT_LOOK_AT, DEFAULT_UP, Scene, camera_basis


def _p(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p)


_PROGRESS_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_uint32)


@dataclass
class RenderSegmentData:
    """Definitions.hpp:15-21."""
    yBegin: int = 0
    yEnd: int = 0
    xBegin: int = 0
    xEnd: int = 0


def _fmix64(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def sample_state(seed, pixel, sample, draws=0):
    """The state of the render's keyed stream of (seed, pixel = y * width + x, sample) after
    `draws` draws (2 = past the primary ray's jitter), as trace_rays takes it: what
    spt_sample_state computes, in numpy.  pixel, sample and draws may be arrays (broadcast
    together): a uint64 array then, else an int."""
    px, sm, dr = np.broadcast_arrays(np.asarray(pixel, np.uint32), np.asarray(sample, np.uint32),
                                     np.asarray(draws, np.uint32))
    key = _fmix64(np.array([int(seed) & 0xFFFFFFFFFFFFFFFF], np.uint64))
    word = (px.astype(np.uint64) << np.uint64(32)) | sm.astype(np.uint64)
    out = _fmix64(np.atleast_1d(key ^ word)) + np.atleast_1d(dr.astype(np.uint64)) * np.uint64(0x9E3779B97F4A7C15)
    return out.reshape(px.shape) if px.ndim else int(out[0])


class Context:
    """One device context (spt_ctx) holding scene, camera and config."""

    def __init__(self, device: int = 0, devices=None):
        """One device, or with `devices` (a list of ordinals, repeats allowed) a
        multi-device context (spt_ctx_create_multi) whose member 0 is devices[0]."""
        L = _native.lib()
        h = ctypes.c_void_p()
        if devices is None:
            _native.check(L.spt_ctx_create(device, ctypes.byref(h)))
            self.devices = [device]
        else:
            devs = np.ascontiguousarray(np.asarray(devices, np.int32))
            _native.check(L.spt_ctx_create_multi(_p(devs), len(devs), ctypes.byref(h)))
            self.devices = [int(d) for d in devs]
        self._h = h
        self.device = self.devices[0]
        self._frame = None  # (width, height) after set_params

    @property
    def handle(self):
        return self._h

    def close(self) -> None:
        if self._h:
            _native.lib().spt_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, code: int) -> None:
        _native.check(code, self._h)

    def set_scene(self, scene: Scene) -> None:
        self._scene = scene  # keep arrays alive for the duration of the call
        self._check(_native.lib().spt_set_scene(self._h, _p(scene.centers), _p(scene.radii), _p(scene.colors),
                                                _p(scene.materials), _p(scene.fuzz), scene.n))

    def set_camera(self, view, eye=DEFAULT_EYE, sky=INIT_COLOR) -> None:
        v = np.ascontiguousarray(np.asarray(view, np.float32).reshape(16))
        e = np.ascontiguousarray(np.asarray(eye, np.float32).reshape(4))
        s = np.ascontiguousarray(np.asarray(sky, np.float32).reshape(4))
        self._check(_native.lib().spt_set_camera(self._h, _p(v), _p(e), _p(s)))

    def update_scene(self, centers=None, view=None, eye=None) -> dict:
        """Move the spheres and / or the camera without a rebuild (spt_update_scene): `centers`
        (n, 3) or (n, 4) floats in the scene's order (None: the spheres stay), `view` and `eye`
        together (None: the camera stays; the sky stays either way).  The traversal tables are
        refit and the primary-ray candidate lists built on the device; every later call
        computes what it computes after set_scene with the moved centres and set_camera, bit
        for bit.  Returns spt_update_info as a dict, with lists_reason as a word ('device',
        'off', 'camera', 'slots', 'unchanged')."""
        c4 = None
        if centers is not None:
            c = np.asarray(centers, np.float32)
            if c.ndim != 2 or c.shape[1] not in (3, 4):
                raise ValueError(f"centers: expected (n, 3) or (n, 4) floats, got shape {c.shape}")
            c4 = np.zeros((len(c), 4), np.float32)
            c4[:, :3] = c[:, :3]
            n = getattr(getattr(self, "_scene", None), "n", None)
            if n is not None and len(c4) != n:
                raise ValueError(f"centers: {len(c4)} spheres, the scene has {n}")
        if (view is None) != (eye is None):
            raise ValueError("update_scene: view and eye come together")
        v = None if view is None else _view16(view)
        e = None if eye is None else _eye4(eye)
        info = _native.UpdateInfo()
        self._check(_native.lib().spt_update_scene(self._h, None if c4 is None else _p(c4), None if v is None else _p(v),
                                                   None if e is None else _p(e), ctypes.byref(info)))
        d = {k: getattr(info, k) for k, _ in _native.UpdateInfo._fields_}
        d["lists_reason"] = _native.UPDATE_LISTS_REASONS.get(info.lists_reason, info.lists_reason)
        return d

    def prim_lists(self, which: int = 0):
        """The context's primary-ray candidate lists (spt_prim_lists_read): which = 0 those its
        device holds, which = 1 the host builder's for the current tables, camera and frame.
        Returns (b8, b4, ids, orig, on): (blocks, 2) uint32 {first, count} per 8x8 / 8x4
        block (count 0xFFFFFFFF: the block walks), the entries, the sphere of every slot."""
        L = _native.lib()
        w, h = self._frame
        bw = (w + 7) // 8
        b8 = np.zeros(2 * bw * ((h + 7) // 8), np.uint32)
        b4 = np.zeros(2 * bw * ((h + 3) // 4), np.uint32)
        counts = np.zeros(4, np.uint32)
        self._check(L.spt_prim_lists_read(self._h, which, None, None, None, None, 0, _p(counts)))
        cap = int(max(counts[0], counts[1], 1))
        ids, orig = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        self._check(L.spt_prim_lists_read(self._h, which, _p(b8), _p(b4), _p(ids), _p(orig), cap, _p(counts)))
        return b8.reshape(-1, 2), b4.reshape(-1, 2), ids[:counts[0]], orig[:counts[1]], bool(counts[3])

    def set_params(self, width: int, height: int, spp: int, bounces: int, seed: int = 1) -> None:
        self._check(_native.lib().spt_set_params(self._h, width, height, spp, bounces, seed))
        self._frame = (width, height)

    def set_cluster_size(self, k: int) -> None:
        """Culling cluster size (0 = brute force over every sphere); results identical."""
        self._check(_native.lib().spt_set_cluster_size(self._h, int(k)))

    def set_cluster_tree(self, branching: int) -> None:
        """Children per inner node of the cluster tree (0 = flat list,
        _native.TREE_AUTO = default heuristic); results identical."""
        self._check(_native.lib().spt_set_cluster_tree(self._h, int(branching)))

    def prepare_dropin(self) -> None:
        """spt_prepare_dropin (what the C++ shim does once after creating its context): create
        the drop-in's batch and read-ahead streams now, and arm the tiling read-ahead at a
        tiling's first call (SPT_READAHEAD_FIRST=0: only after a whole tiling)."""
        self._check(_native.lib().spt_prepare_dropin(self._h))

    def set_reserved_cus(self, n: int) -> None:
        """Keep n CUs free of launched renders (spt_set_reserved_cus: 32 = one per shader
        engine lets a whole-CU kernel on another stream start beside a render); results
        identical."""
        self._check(_native.lib().spt_set_reserved_cus(self._h, int(n)))

    def set_engine(self, engine: int) -> None:
        """_native.ENGINE_MEGAKERNEL (default) or _native.ENGINE_WAVEFRONT; results identical."""
        self._check(_native.lib().spt_set_engine(self._h, int(engine)))

    def set_workspace(self, nbytes: int) -> None:
        self._check(_native.lib().spt_set_workspace(self._h, int(nbytes)))

    def render_segment(self, yB, yE, xB, xE, g_data=None, task=False, rgba=True):
        """Returns region-local float4 pixels (None with rgba=False: g_data only, the C++
        drop-in's form, which the tiling read-ahead serves); writes g_data bytes of the
        region if given."""
        out = np.zeros((max(yE - yB, 0) * max(xE - xB, 0), 4), np.float32) if rgba else None
        fn = _native.lib().spt_render_segment_task if task else _native.lib().spt_render_segment
        gp = None
        if g_data is not None:
            assert g_data.dtype == np.uint8 and g_data.flags.c_contiguous
            gp = _p(g_data)
        self._check(fn(self._h, yB, yE, xB, xE, _p(out) if rgba else None, gp))
        return out

    def render_frame(self, g_data=None, task=False, rgba=True):
        """The whole frame over every member device (spt_render_frame): returns the
        row-major float4 frame (or None with rgba=False); writes g_data if given."""
        L = _native.lib()
        if self._frame is None:
            # SPT_ERR_STATE, as the library reports it to its own callers
            raise _native.SptError(2, "params not set (set_params)")
        w, h = self._frame
        out = np.zeros((w * h, 4), np.float32) if rgba else None
        gp = None
        if g_data is not None:
            assert g_data.dtype == np.uint8 and g_data.flags.c_contiguous and g_data.size == w * h * 3
            gp = _p(g_data)
        self._check(L.spt_render_frame(self._h, 1 if task else 0, _p(out) if rgba else None, gp))
        return out

    def pin_host(self, arr: np.ndarray) -> None:
        """Page-lock a host array (e.g. g_data) for direct device-to-host copies."""
        assert arr.flags.c_contiguous
        self._check(_native.lib().spt_pin_host(self._h, _p(arr), arr.nbytes))

    def unpin_host(self, arr: np.ndarray) -> None:
        self._check(_native.lib().spt_unpin_host(self._h, _p(arr)))

    def render_progressive(self, yB, yE, xB, xE, pass_spp: int, g_data=None, callback=None, task=False):
        """Progressive render in passes of pass_spp samples.  After each pass the returned
        float4 array (and g_data, if given) hold the render at the samples done so far
        (bit-identical to a render with that many samples) and callback(samples_done)
        runs; a truthy return stops the render."""
        rgba = np.zeros((max(yE - yB, 0) * max(xE - xB, 0), 4), np.float32)
        gp = None
        if g_data is not None:
            assert g_data.dtype == np.uint8 and g_data.flags.c_contiguous
            gp = _p(g_data)
        errors = []

        def tramp(_user, done):
            try:
                return 1 if (callback is not None and callback(int(done))) else 0
            except BaseException as e:  # stop the render, re-raise below
                errors.append(e)
                return 1

        cb = _PROGRESS_FN(tramp)
        self._check(_native.lib().spt_render_progressive(self._h, int(task), yB, yE, xB, xE, pass_spp, _p(rgba), gp,
                                                         ctypes.cast(cb, ctypes.c_void_p), None))
        if errors:
            raise errors[0]
        return rgba

    def render_samples(self, yB, yE, xB, xE, spp: int, task=False) -> np.ndarray:
        out = np.zeros(((yE - yB) * (xE - xB), spp, 4), np.float32)
        self._check(_native.lib().spt_render_samples(self._h, int(task), yB, yE, xB, xE, _p(out)))
        return out

    def render_rows_async(self, mode, yB, yE, strip, parts, part, xB, xE, d_rgba=0, d_rgb8=0, stream=0) -> None:
        """Device-resident launch; d_rgba/d_rgb8/stream are raw device pointers / hipStream_t."""
        self._check(_native.lib().spt_render_rows_async(self._h, mode, yB, yE, strip, parts, part, xB, xE,
                                                        ctypes.c_void_p(d_rgba or None),
                                                        ctypes.c_void_p(d_rgb8 or None),
                                                        ctypes.c_void_p(stream or None)))

    def assemble_rows_async(self, d_tiles, max_rows, yB, yE, strip, parts, xB, xE, d_frame=0, d_rgb8=0,
                            stream=0) -> None:
        self._check(_native.lib().spt_assemble_rows_async(self._h, ctypes.c_void_p(d_tiles), max_rows, yB, yE, strip,
                                                          parts, xB, xE, ctypes.c_void_p(d_frame or None),
                                                          ctypes.c_void_p(d_rgb8 or None),
                                                          ctypes.c_void_p(stream or None)))

    def render_task_range_async(self, i0, i1, d_rgba, stream=0) -> None:
        """Outputs [i0, i1) of RenderSegmentTask({0, H, 0, W}) on a non-square frame into
        d_rgba (spt_render_task_range_async: the rank-share form of its aliasing)."""
        self._check(_native.lib().spt_render_task_range_async(self._h, i0, i1, ctypes.c_void_p(d_rgba or None),
                                                              ctypes.c_void_p(stream or None)))

    @staticmethod
    def _rays4(a, what) -> np.ndarray:
        a = np.asarray(a, np.float32)
        if a.ndim != 2 or a.shape[1] not in (3, 4):
            raise ValueError(f"{what}: expected an (n, 3) or (n, 4) array, got shape {a.shape}")
        if a.shape[1] == 3:
            a = np.concatenate([a, np.zeros((len(a), 1), np.float32)], axis=1)
        return np.ascontiguousarray(a)

    def cast_rays(self, origins, dirs, hits=False):
        """cd::FindClosestIntersectionSphere (Collision.hpp:87-109) for n rays on the device
        (spt_cast_rays): origins and dirs are (n, 3) or (n, 4) float arrays (w ignored).
        Returns idx (uint32: the closest sphere's index, the sphere count on a miss), or with
        hits=True (idx, hit) where hit[i] = [[Px, Py, Pz, t], [nx, ny, nz, ds]]: contact
        point and parameter, contact normal and the squared distance compared; zeros on a
        miss."""
        o, d = self._rays4(origins, "origins"), self._rays4(dirs, "dirs")
        if len(o) != len(d):
            raise ValueError(f"{len(o)} origins for {len(d)} directions")
        idx = np.zeros(len(o), np.uint32)
        hit = np.zeros((len(o), 2, 4), np.float32) if hits else None
        self._check(_native.lib().spt_cast_rays(self._h, _p(o), _p(d), len(o), _p(idx), _p(hit) if hits else None))
        return (idx, hit) if hits else idx

    def cast_rays_async(self, d_origins, d_dirs, n, d_idx, d_hit=0, stream=0) -> None:
        """Device-resident cast_rays (spt_cast_rays_async): raw device pointers to n float4
        origins and directions, n uint32 indices and (optionally) 2 n float4 hit records,
        enqueued on `stream` (a hipStream_t; 0 = the default stream)."""
        self._check(_native.lib().spt_cast_rays_async(self._h, ctypes.c_void_p(d_origins or None),
                                                      ctypes.c_void_p(d_dirs or None), int(n),
                                                      ctypes.c_void_p(d_idx or None), ctypes.c_void_p(d_hit or None),
                                                      ctypes.c_void_p(stream or None)))

    def _occluded(self, a, b, limits, flags, scale) -> np.ndarray:
        occ = np.zeros(len(a), np.uint8)
        self._check(_native.lib().spt_occluded_rays(self._h, _p(a), _p(b), _p(limits) if limits is not None else None,
                                                    len(a), flags, float(scale), _p(occ)))
        return occ.astype(bool)

    def occluded(self, origins, dirs, limit_sq=None) -> np.ndarray:
        """Any-hit with a distance limit (spt_occluded_rays): for n rays, (n, 3) or (n, 4)
        float arrays (w ignored), whether cast_rays would hit a sphere with ds < limit_sq --
        a SQUARED distance, fp32, a scalar or an (n,) array; None: unbounded.  Returns an (n,)
        bool array.  NaN and <= 0 limits give False; the compare is strict."""
        o, d = self._rays4(origins, "origins"), self._rays4(dirs, "dirs")
        if len(o) != len(d):
            raise ValueError(f"{len(o)} origins for {len(d)} directions")
        lim = None
        if limit_sq is not None:
            lim = np.asarray(limit_sq, np.float32)
            if lim.ndim == 0:
                lim = np.full(len(o), lim, np.float32)
            lim = np.ascontiguousarray(lim.reshape(-1))
            if len(lim) != len(o):
                raise ValueError(f"{len(lim)} limits for {len(o)} rays")
        return self._occluded(o, d, lim, 0, 1.0)

    def visible(self, a, b, scale=1.0) -> np.ndarray:
        """Line of sight between the points a[i] and b[i], (n, 3) or (n, 4) float arrays:
        True where no sphere blocks the segment (spt_occluded_rays with
        SPT_OCCLUDE_SEGMENTS, negated): the ray from a along Normalize(b - a), limited to
        |b - a|^2 * scale.  A b on a sphere's surface lies at that sphere's own distance to
        within rounding: pass a scale slightly below 1 to leave the target out."""
        pa, pb = self._rays4(a, "a"), self._rays4(b, "b")
        if len(pa) != len(pb):
            raise ValueError(f"{len(pa)} points a for {len(pb)} points b")
        return ~self._occluded(pa, pb, None, _native.OCCLUDE_SEGMENTS, scale)

    def occluded_async(self, d_a, d_b, d_limits, n, d_occ, segments=False, scale=1.0, stream=0) -> None:
        """Device-resident occluded / visible (spt_occluded_rays_async): raw device pointers
        to n float4 origins and directions (segments=True: end points a and b), n fp32
        squared limits (0: unbounded; must be 0 with segments) and n answer bytes (1 =
        occluded), enqueued on `stream` (a hipStream_t; 0 = the default stream)."""
        self._check(_native.lib().spt_occluded_rays_async(
            self._h, ctypes.c_void_p(d_a or None), ctypes.c_void_p(d_b or None), ctypes.c_void_p(d_limits or None), int(n),
            _native.OCCLUDE_SEGMENTS if segments else 0, float(scale), ctypes.c_void_p(d_occ or None),
            ctypes.c_void_p(stream or None)))

    def primary_hits(self, xys, hits=False, dirs=False):
        """The closest sphere of the primary ray of sample s of pixel (x, y), for every
        (x, y, s) row of xys (spt_primary_hits; the render's own ray).  Returns idx, followed
        by hit (as cast_rays) with hits=True and by the (n, 4) directions with dirs=True."""
        t = np.ascontiguousarray(np.asarray(xys, np.uint32).reshape(-1, 3))
        idx = np.zeros(len(t), np.uint32)
        hit = np.zeros((len(t), 2, 4), np.float32) if hits else None
        dv = np.zeros((len(t), 4), np.float32) if dirs else None
        self._check(_native.lib().spt_primary_hits(self._h, _p(t), len(t), _p(idx), _p(hit) if hits else None,
                                                   _p(dv) if dirs else None))
        out = (idx,) + ((hit,) if hits else ()) + ((dv,) if dirs else ())
        return out if len(out) > 1 else idx

    def trace_rays(self, origins, dirs, bounces: int, states=None, seed: int = 0, info=False):
        """TraceAndSampleColor(d, o, bounces) (SingleThreadPathTracer.hpp:94-112) for n rays on
        the device (spt_trace_rays): origins and dirs are (n, 3) or (n, 4) float arrays (w
        ignored), states the raw splitmix state each ray draws from (uint64; None: ray i
        gets sample_state(seed, i, 0)).  Needs scene and camera (the sky).  Returns the
        colours (n, 4), w = 0, or with info=True (rgba, info) where info[i] = [casts,
        specular events | cut at the specular cap << 31]."""
        o, d = self._rays4(origins, "origins"), self._rays4(dirs, "dirs")
        if len(o) != len(d):
            raise ValueError(f"{len(o)} origins for {len(d)} directions")
        if states is None:
            st = sample_state(seed, np.arange(len(o), dtype=np.uint32), 0)
        else:
            st = np.ascontiguousarray(np.asarray(states, np.uint64).reshape(-1))
            if len(st) != len(o):
                raise ValueError(f"{len(st)} states for {len(o)} rays")
        rgba = np.zeros((len(o), 4), np.float32)
        inf = np.zeros((len(o), 2), np.uint32) if info else None
        self._check(_native.lib().spt_trace_rays(self._h, _p(o), _p(d), _p(st), len(o), int(bounces), _p(rgba),
                                                 _p(inf) if info else None))
        return (rgba, inf) if info else rgba

    def trace_rays_async(self, d_origins, d_dirs, d_states, n, bounces, d_rgba, d_info=0, stream=0) -> None:
        """Device-resident trace_rays (spt_trace_rays_async): raw device pointers to n float4
        origins and directions, n uint64 states, n float4 colours and (optionally) 2 n uint32
        info words, enqueued on `stream` (a hipStream_t; 0 = the default stream)."""
        self._check(_native.lib().spt_trace_rays_async(self._h, ctypes.c_void_p(d_origins or None),
                                                       ctypes.c_void_p(d_dirs or None), ctypes.c_void_p(d_states or None),
                                                       int(n), int(bounces), ctypes.c_void_p(d_rgba or None),
                                                       ctypes.c_void_p(d_info or None), ctypes.c_void_p(stream or None)))

    def id_buffer(self, s: int = 0) -> np.ndarray:
        """The picking / object-id buffer: an (H, W) uint32 image of the sphere sample s of
        every pixel sees first (the sphere count where it sees the sky)."""
        if self._frame is None:
            raise _native.SptError(2, "params not set (set_params)")
        w, h = self._frame
        ys, xs = np.mgrid[0:h, 0:w]
        xys = np.stack([xs.ravel(), ys.ravel(), np.full(w * h, s)], axis=1).astype(np.uint32)
        return self.primary_hits(xys).reshape(h, w)

    def render_features(self, yB, yE, xB, xE, ids=False):
        """Feature buffers of the rectangle [yB, yE) x [xB, xE) over the frame's own primary rays
        (spt_render_features): feat of shape (pixels, 2, 4), float32, per region-local pixel
        [[albedo r, g, b, coverage], [normal x, y, z, depth]], each the mean over the spp
        samples (the mean hit depth is depth / coverage); with ids=True (feat, ids), ids the
        sphere sample 0 sees first (uint32, the sphere count for the sky)."""
        n = max(yE - yB, 0) * max(xE - xB, 0)
        feat = np.zeros((n, 2, 4), np.float32)
        idx = np.zeros(n, np.uint32) if ids else None
        self._check(_native.lib().spt_render_features(self._h, yB, yE, xB, xE, _p(feat), _p(idx) if ids else None))
        return (feat, idx) if ids else feat

    def render_features_async(self, yB, yE, strip, parts, part, xB, xE, d_feat=0, d_ids=0, stream=0) -> None:
        """Device-resident render_features (spt_render_features_async) over the rows of
        render_rows_async's row map: raw device pointers to 8 floats and / or one uint32 per
        local pixel, enqueued on `stream` (a hipStream_t; 0 = the default stream)."""
        self._check(_native.lib().spt_render_features_async(self._h, yB, yE, strip, parts, part, xB, xE,
                                                            ctypes.c_void_p(d_feat or None),
                                                            ctypes.c_void_p(d_ids or None),
                                                            ctypes.c_void_p(stream or None)))

    def feature_buffers(self) -> dict:
        """The whole frame's feature buffers: albedo (H, W, 3), coverage (H, W), normal
        (H, W, 3), depth (H, W), all float32, and ids (H, W), uint32."""
        if self._frame is None:
            raise _native.SptError(2, "params not set (set_params)")
        w, h = self._frame
        feat, idx = self.render_features(0, h, 0, w, ids=True)
        feat = feat.reshape(h, w, 2, 4)
        return {"albedo": feat[:, :, 0, :3], "coverage": feat[:, :, 0, 3], "normal": feat[:, :, 1, :3],
                "depth": feat[:, :, 1, 3], "ids": idx.reshape(h, w)}

    def _denoise_inputs(self, rgba, feat):
        """(rgba, feat, w, h) of denoise's and denoise_variance's image arguments, as
        contiguous float32 arrays."""
        rgba = np.ascontiguousarray(rgba, np.float32)
        if rgba.ndim == 3 and rgba.shape[2] == 4:
            h, w = rgba.shape[:2]
        elif rgba.ndim == 2 and rgba.shape[1] == 4 and self._frame is not None and \
                rgba.shape[0] == self._frame[0] * self._frame[1]:
            w, h = self._frame
        else:
            raise ValueError(f"rgba: expected (H, W, 4), or (W * H, 4) of the current frame, got shape {rgba.shape}")
        if isinstance(feat, dict):
            feat = np.concatenate([np.asarray(feat["albedo"], np.float32).reshape(h, w, 3),
                                   np.asarray(feat["coverage"], np.float32).reshape(h, w, 1),
                                   np.asarray(feat["normal"], np.float32).reshape(h, w, 3),
                                   np.asarray(feat["depth"], np.float32).reshape(h, w, 1)], axis=2)
        feat = np.ascontiguousarray(feat, np.float32)
        if feat.size != w * h * 8:
            raise ValueError(f"feat: expected 8 floats for each of {w} x {h} pixels, got shape {feat.shape}")
        return rgba, feat, w, h

    def denoise(self, rgba, feat, sigma_color=30.0, sigma_albedo=0.1, sigma_normal=0.25, sigma_depth=0.5, levels=3,
                g_data=False):
        """The edge-avoiding a-trous filter of include/spt_hip.h "denoiser" on the device
        (spt_denoise).  rgba: an (H, W, 4) float array, colours on the renders' 0..255 scale,
        or the current frame as (W * H, 4) (what render_frame returns).  feat: what
        render_features returns for the same pixels ((pixels, 2, 4), or any shape of 8 floats
        per pixel), or the dict of feature_buffers().  Each sigma must be > 0 (inf switches
        its term off); levels is 1..8.  Returns the filtered image in rgba's shape, or with
        g_data=True (image, bytes): bytes the image as a g_data frame of its own W x H."""
        rgba, feat, w, h = self._denoise_inputs(rgba, feat)
        out = np.zeros_like(rgba)
        g = np.zeros(w * h * 3, np.uint8) if g_data else None
        self._check(_native.lib().spt_denoise(self._h, w, h, _p(rgba), _p(feat), sigma_color, sigma_albedo, sigma_normal,
                                              sigma_depth, int(levels), _p(out), _p(g) if g_data else None))
        return (out, g) if g_data else out

    def denoise_async(self, width, height, d_rgba, d_feat, sigma_color=30.0, sigma_albedo=0.1, sigma_normal=0.25,
                      sigma_depth=0.5, levels=3, d_out=0, d_rgb8=0, d_scratch=0, stream=0) -> None:
        """Device-resident denoise (spt_denoise_async): raw device pointers to width * height
        float4 colours, 8 floats of features per pixel, the float4 output and / or the
        width * height * 3 g_data bytes, and denoise_scratch_bytes(width, height, levels) bytes
        of scratch of the call's own; one launch per level on `stream` (a hipStream_t; 0 = the
        default stream)."""
        self._check(_native.lib().spt_denoise_async(self._h, int(width), int(height), ctypes.c_void_p(d_rgba or None),
                                                    ctypes.c_void_p(d_feat or None), sigma_color, sigma_albedo,
                                                    sigma_normal, sigma_depth, int(levels),
                                                    ctypes.c_void_p(d_out or None), ctypes.c_void_p(d_rgb8 or None),
                                                    ctypes.c_void_p(d_scratch or None), ctypes.c_void_p(stream or None)))

    def render_moments(self, yB, yE, xB, xE, g_data=None, rgba=True):
        """A segment-mode render of the rectangle that also returns its per-pixel sample
        moments (spt_render_moments): (rgba, mom), rgba what render_segment returns (None with
        rgba=False), mom of shape (pixels, 4), float32: the mean and the second moment of the
        samples' luminance, their population variance and the sample count.  Writes g_data
        bytes of the region if given.  The region's samples must fit the workspace at once."""
        n = max(yE - yB, 0) * max(xE - xB, 0)
        out = np.zeros((n, 4), np.float32) if rgba else None
        mom = np.zeros((n, 4), np.float32)
        gp = None
        if g_data is not None:
            assert g_data.dtype == np.uint8 and g_data.flags.c_contiguous
            gp = _p(g_data)
        self._check(_native.lib().spt_render_moments(self._h, yB, yE, xB, xE, _p(out) if rgba else None, gp, _p(mom)))
        return out, mom

    def render_moments_async(self, yB, yE, strip, parts, part, xB, xE, d_rgba=0, d_rgb8=0, d_mom=0, stream=0) -> None:
        """Device-resident render_moments (spt_render_moments_async) over the rows of
        render_rows_async's row map: raw device pointers to the float4 colours and / or the
        frame's g_data bytes, and to one float4 of moments per local pixel, enqueued on
        `stream` (a hipStream_t; 0 = the default stream)."""
        self._check(_native.lib().spt_render_moments_async(self._h, yB, yE, strip, parts, part, xB, xE,
                                                           ctypes.c_void_p(d_rgba or None),
                                                           ctypes.c_void_p(d_rgb8 or None),
                                                           ctypes.c_void_p(d_mom or None),
                                                           ctypes.c_void_p(stream or None)))

    def denoise_variance(self, rgba, feat, mom, sigma_color=4.0, sigma_albedo=0.1, sigma_normal=0.25, sigma_depth=0.5,
                         var_floor=1.0, levels=3, g_data=False, variance=False):
        """The variance-guided a-trous filter of include/spt_hip.h "variance-guided denoiser"
        on the device (spt_denoise_var): denoise's arguments, mom what render_moments returns
        for the same pixels (4 floats per pixel), and var_floor, finite and > 0, added to the
        variances that normalise the colour term; sigma_color counts standard deviations.
        Returns the filtered image in rgba's shape; with g_data and / or variance a tuple
        (image[, bytes][, var]), var the filtered variance of the pixel means, (H, W)."""
        rgba, feat, w, h = self._denoise_inputs(rgba, feat)
        mom = np.ascontiguousarray(mom, np.float32)
        if mom.size != w * h * 4:
            raise ValueError(f"mom: expected 4 floats for each of {w} x {h} pixels, got shape {mom.shape}")
        out = np.zeros_like(rgba)
        g = np.zeros(w * h * 3, np.uint8) if g_data else None
        var = np.zeros((h, w), np.float32) if variance else None
        self._check(_native.lib().spt_denoise_var(self._h, w, h, _p(rgba), _p(feat), _p(mom), sigma_color, sigma_albedo,
                                                  sigma_normal, sigma_depth, var_floor, int(levels), _p(out),
                                                  _p(g) if g_data else None, _p(var) if variance else None))
        res = (out,) + ((g,) if g_data else ()) + ((var,) if variance else ())
        return res if len(res) > 1 else out

    def denoise_variance_async(self, width, height, d_rgba, d_feat, d_mom, sigma_color=4.0, sigma_albedo=0.1,
                               sigma_normal=0.25, sigma_depth=0.5, var_floor=1.0, levels=3, d_out=0, d_rgb8=0, d_out_var=0,
                               d_scratch=0, stream=0) -> None:
        """Device-resident denoise_variance (spt_denoise_var_async): denoise_async's pointers,
        d_mom (one float4 per pixel) and d_out_var (one float per pixel, optional)."""
        self._check(_native.lib().spt_denoise_var_async(
            self._h, int(width), int(height), ctypes.c_void_p(d_rgba or None), ctypes.c_void_p(d_feat or None),
            ctypes.c_void_p(d_mom or None), sigma_color, sigma_albedo, sigma_normal, sigma_depth, var_floor, int(levels),
            ctypes.c_void_p(d_out or None), ctypes.c_void_p(d_rgb8 or None), ctypes.c_void_p(d_out_var or None),
            ctypes.c_void_p(d_scratch or None), ctypes.c_void_p(stream or None)))

    def render_adaptive(self, yB, yE, xB, xE, base_spp=8, step_spp=8, max_spp=64, tol=0.08, lum_floor=1.0, g_data=None):
        """An adaptively sampled segment-mode render of the rectangle (spt_render_adaptive):
        every 8x8 tile of it gets base_spp samples, then step_spp more per pass while any of
        its pixels' mean is still noisier than tol (relative to its luminance + lum_floor), up
        to max_spp.  Returns (rgba, mom, info): rgba of shape (pixels, 4), each pixel what
        render_segment gives at its own sample count; mom of shape (pixels, 4) as
        render_moments', mom[:, 3] the per-pixel sample count; info a dict with the samples
        rendered and the passes run.  Writes g_data bytes of the region if given.  The
        context's own spp is not read."""
        n = max(yE - yB, 0) * max(xE - xB, 0)
        out = np.zeros((n, 4), np.float32)
        mom = np.zeros((n, 4), np.float32)
        info = np.zeros(2, np.uint64)
        gp = None
        if g_data is not None:
            assert g_data.dtype == np.uint8 and g_data.flags.c_contiguous
            gp = _p(g_data)
        self._check(_native.lib().spt_render_adaptive(self._h, yB, yE, xB, xE, int(base_spp), int(step_spp), int(max_spp),
                                                      tol, lum_floor, _p(out), gp, _p(mom), _p(info)))
        return out, mom, {"samples": int(info[0]), "passes": int(info[1])}

    def render_adaptive_dev(self, yB, yE, xB, xE, base_spp=8, step_spp=8, max_spp=64, tol=0.08, lum_floor=1.0, rgba=None,
                            rgb8=None, mom=None, stream=0) -> dict:
        """render_adaptive into torch tensors on the context's device (spt_render_adaptive_dev):
        rgba and mom float32 with 4 floats per region pixel, rgb8 the full frame's g_data
        bytes (uint8), each optional; on `stream` (a hipStream_t; 0 = the default stream).
        The host waits on the stream once per pass, and the call returns with the last pass's
        fold enqueued: synchronise the stream before reading the tensors.  Returns info."""
        n = max(yE - yB, 0) * max(xE - xB, 0)
        for t, what, count in ((rgba, "rgba", n * 4), (mom, "mom", n * 4)):
            if t is not None and not (t.is_cuda and t.is_contiguous() and t.dtype.is_floating_point and
                                      t.element_size() == 4 and t.numel() == count):
                raise ValueError(f"{what}: expected a contiguous float32 device tensor of {count} elements")
        if rgb8 is not None and not (rgb8.is_cuda and rgb8.is_contiguous() and rgb8.element_size() == 1 and
                                     self._frame is not None and rgb8.numel() == self._frame[0] * self._frame[1] * 3):
            raise ValueError("rgb8: expected a contiguous uint8 device tensor of the frame's W * H * 3 bytes")
        info = np.zeros(2, np.uint64)
        ptr = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else None)  # noqa: E731
        self._check(_native.lib().spt_render_adaptive_dev(self._h, yB, yE, xB, xE, int(base_spp), int(step_spp),
                                                          int(max_spp), tol, lum_floor, ptr(rgba), ptr(rgb8), ptr(mom),
                                                          _p(info), ctypes.c_void_p(stream or None)))
        return {"samples": int(info[0]), "passes": int(info[1])}

    def temporal(self, rgba, mom, feat, ids, view, eye, history=None, prev_view=None, prev_eye=None, tol_normal=0.25,
                 tol_depth=0.1, max_history=64.0, motion=None):
        """Temporal accumulation of include/spt_hip.h "temporal accumulation" on the device
        (spt_temporal): this frame's rgba ((H, W, 4), or the current frame as (W * H, 4)), mom
        (what render_moments or render_adaptive returns), feat and ids (what
        render_features(ids=True) returns) and its camera, blended with `history`, the tuple
        (rgba, mom, feat, ids) of the previous frame (rgba and mom: the previous call's
        outputs, or a first frame's own), seen through prev_view from prev_eye.  Without a
        history the outputs are copies.  Returns (out_rgba, out_mom) in rgba's and mom's
        shapes; keep them with feat, ids and the camera as the next frame's history.
        With `motion`, the (n, 8) table of sphere_motion(scene, prev_scene), the history
        follows the spheres that moved between the two frames (spt_temporal_motion)."""
        rgba, feat, w, h = self._denoise_inputs(rgba, feat)
        n = w * h

        def arr(a, dtype, per, what):
            a = np.ascontiguousarray(a, dtype)
            if a.size != n * per:
                raise ValueError(f"{what}: expected {per} value(s) for each of {w} x {h} pixels, got shape {a.shape}")
            return a

        mom = arr(mom, np.float32, 4, "mom")
        ids = arr(ids, np.uint32, 1, "ids")
        cam = [_view16(view), _eye4(eye), None, None]
        hist = [None] * 4
        if history is not None:
            if prev_view is None or prev_eye is None:
                raise ValueError("history needs prev_view and prev_eye")
            h_rgba, h_mom, h_feat, h_ids = history
            hist = [arr(h_rgba, np.float32, 4, "history rgba"), arr(h_mom, np.float32, 4, "history mom"),
                    arr(h_feat, np.float32, 8, "history feat"), arr(h_ids, np.uint32, 1, "history ids")]
            cam[2:] = [_view16(prev_view), _eye4(prev_eye)]
        out, out_mom = np.zeros_like(rgba), np.zeros_like(mom)
        ptr = lambda a: None if a is None else _p(a)  # noqa: E731
        args = [self._h, w, h, _p(rgba), _p(mom), _p(feat), _p(ids), _p(cam[0]), _p(cam[1]), ptr(hist[0]), ptr(hist[1]),
                ptr(hist[2]), ptr(hist[3]), ptr(cam[2]), ptr(cam[3])]
        if motion is None:
            self._check(_native.lib().spt_temporal(*args, tol_normal, tol_depth, max_history, _p(out), _p(out_mom)))
            return out, out_mom
        motion = _motion_table(motion)
        self._check(_native.lib().spt_temporal_motion(*args, _p(motion) if len(motion) else None, len(motion), tol_normal,
                                                      tol_depth, max_history, _p(out), _p(out_mom)))
        return out, out_mom

    def temporal_async(self, width, height, d_rgba, d_mom, d_feat, d_ids, view, eye, d_hist=None, prev_view=None,
                       prev_eye=None, tol_normal=0.25, tol_depth=0.1, max_history=64.0, d_out_rgba=0, d_out_mom=0,
                       stream=0, d_motion=0, n_spheres=0) -> None:
        """Device-resident temporal (spt_temporal_async): raw device pointers to this frame's
        width * height float4 colours, float4 moments, 8 floats of features and uint32 ids per
        pixel, d_hist the tuple of the previous frame's four pointers (or None), and the two
        float4 outputs; the cameras are host arrays, read before the call returns.  One launch
        on `stream` (a hipStream_t; 0 = the default stream).  With d_motion, a device pointer to
        the n_spheres records of sphere_motion's table, spt_temporal_motion_async instead."""
        cam = [_view16(view), _eye4(eye), None if prev_view is None else _view16(prev_view),
               None if prev_eye is None else _eye4(prev_eye)]
        dh = tuple(d_hist) if d_hist is not None else (0, 0, 0, 0)
        ptr = lambda a: None if a is None else _p(a)  # noqa: E731
        args = [self._h, int(width), int(height), ctypes.c_void_p(d_rgba or None), ctypes.c_void_p(d_mom or None),
                ctypes.c_void_p(d_feat or None), ctypes.c_void_p(d_ids or None), ptr(cam[0]), ptr(cam[1]),
                ctypes.c_void_p(dh[0] or None), ctypes.c_void_p(dh[1] or None), ctypes.c_void_p(dh[2] or None),
                ctypes.c_void_p(dh[3] or None), ptr(cam[2]), ptr(cam[3])]
        tail = [tol_normal, tol_depth, max_history, ctypes.c_void_p(d_out_rgba or None), ctypes.c_void_p(d_out_mom or None),
                ctypes.c_void_p(stream or None)]
        if not d_motion and not n_spheres:
            self._check(_native.lib().spt_temporal_async(*args, *tail))
        else:
            self._check(_native.lib().spt_temporal_motion_async(*args, ctypes.c_void_p(d_motion or None), int(n_spheres),
                                                                *tail))

    def render_denoised(self, variance=False, adaptive=None, **sigmas) -> np.ndarray:
        """The current frame rendered, its feature buffers, and the frame filtered by denoise
        (whose keyword arguments `sigmas` takes): render_frame + feature_buffers + denoise.
        Returns the (H, W, 4) float image, or what denoise returns with g_data=True.
        With variance=True the variance-guided filter instead: render_moments of the whole
        frame + feature_buffers + denoise_variance (whose keyword arguments `sigmas` takes).
        With adaptive=dict(...) as well (render_adaptive's keyword arguments; variance=True
        only), render_adaptive of the whole frame takes render_moments' place: its per-pixel
        sample counts in mom give the filter each pixel's own variance of the mean."""
        if self._frame is None:
            raise _native.SptError(2, "params not set (set_params)")
        w, h = self._frame
        if adaptive is not None:
            if not variance:
                raise ValueError("adaptive=... needs variance=True (the filter reads the per-pixel sample counts)")
            rgba, mom, _ = self.render_adaptive(0, h, 0, w, **adaptive)
            return self.denoise_variance(rgba.reshape(h, w, 4), self.feature_buffers(), mom, **sigmas)
        if variance:
            rgba, mom = self.render_moments(0, h, 0, w)
            return self.denoise_variance(rgba.reshape(h, w, 4), self.feature_buffers(), mom, **sigmas)
        return self.denoise(self.render_frame().reshape(h, w, 4), self.feature_buffers(), **sigmas)

    def synchronize(self) -> None:
        self._check(_native.lib().spt_synchronize(self._h))

    def service_start(self) -> None:
        """Render through the resident render service (spt_service_start): consecutive
        renders run as jobs of one persistent launch, without a ramp and tail each."""
        self._check(_native.lib().spt_service_start(self._h))

    def service_set_full_grid(self, full: bool) -> None:
        """Sessions on every block slot (True) or one per CU left free (False, the default)."""
        self._check(_native.lib().spt_service_set_full_grid(self._h, 1 if full else 0))

    def service_stop(self) -> None:
        """Drain and end the service session; renders launch per call again."""
        self._check(_native.lib().spt_service_stop(self._h))

    def stats(self) -> dict:
        s = _native.Stats()
        self._check(_native.lib().spt_get_stats(self._h, ctypes.byref(s)))
        d = {k: getattr(s, k) for k, _ in _native.Stats._fields_}
        d["diag"] = list(s.diag)
        return d

    def reset_stats(self) -> None:
        self._check(_native.lib().spt_reset_stats(self._h))

    def selftest_numerics(self, a, b, bits) -> np.ndarray:
        a = np.ascontiguousarray(a, np.float32)
        b = np.ascontiguousarray(b, np.float32)
        bits = np.ascontiguousarray(bits, np.uint32)
        out = np.zeros((len(a), _native.SELFTEST_COLS), np.float32)
        self._check(_native.lib().spt_selftest_numerics(self._h, _p(a), _p(b), _p(bits), len(a), _p(out)))
        return out


def task_range(width, height, parts, part) -> tuple[int, int]:
    """Part `part` of `parts`'s outputs [i0, i1) of a non-square task-mode frame (spt_task_range)."""
    a, b = ctypes.c_uint32(), ctypes.c_uint32()
    _native.check(_native.lib().spt_task_range(width, height, parts, part, ctypes.byref(a), ctypes.byref(b)))
    return a.value, b.value


def denoise_scratch_bytes(width, height, levels) -> int:
    """Bytes of scratch a denoise_async call of this shape needs (spt_denoise_scratch_bytes)."""
    b = ctypes.c_uint64(0)
    _native.check(_native.lib().spt_denoise_scratch_bytes(int(width), int(height), int(levels), ctypes.byref(b)))
    return b.value


def rows_count(yB, yE, strip, parts, part) -> int:
    r = ctypes.c_uint32(0)
    _native.check(_native.lib().spt_rows_count(yB, yE, strip, parts, part, ctypes.byref(r)))
    return r.value


def _view16(view) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(view, np.float32).reshape(16))


def _eye4(eye) -> np.ndarray:
    """An eye of 3 or 4 floats as the 4 the C ABI reads."""
    e = np.asarray(eye, np.float32).reshape(-1)
    if e.size not in (3, 4):
        raise ValueError(f"eye: expected 3 or 4 floats, got {e.size}")
    return np.ascontiguousarray(np.concatenate([e[:3], np.zeros(1, np.float32)]))


def _motion_table(motion) -> np.ndarray:
    """A motion table as the C ABI reads it: (n, 8) float32, contiguous."""
    m = np.ascontiguousarray(motion, np.float32)
    if m.size % 8:
        raise ValueError(f"motion: expected 8 floats per sphere, got shape {m.shape}")
    return m.reshape(-1, 8)


def sphere_motion(scene: Scene, prev_scene: Scene) -> np.ndarray:
    """The (n, 8) float32 motion table of Context.temporal(motion=...): per sphere {C.xyz, r}
    of `scene`, this frame's, then {Cp.xyz, rp} of `prev_scene`, the previous frame's.  The
    two scenes hold the same spheres in the same order; ValueError when their counts differ."""
    if scene.n != prev_scene.n:
        raise ValueError(f"sphere_motion: {scene.n} spheres now, {prev_scene.n} in the previous scene")
    out = np.zeros((scene.n, 8), np.float32)
    out[:, 0:3], out[:, 3] = scene.centers[:, :3], scene.radii
    out[:, 4:7], out[:, 7] = prev_scene.centers[:, :3], prev_scene.radii
    return out


def temporal_inverse(view) -> np.ndarray:
    """The (3, 3) float32 inverse of view's upper-left 3x3 as Context.temporal uses it for the
    previous camera (spt_temporal_inverse): computed in double, rounded once per entry."""
    v = _view16(view)
    out = np.zeros((3, 3), np.float32)
    _native.check(_native.lib().spt_temporal_inverse(_p(v), _p(out)))
    return out


class TemporalAccumulator:
    """A preview that keeps its samples while the camera and the spheres move: every
    frame(view, eye) renders width x height at spp samples with a seed of its own, accumulates
    it against the stored history (Context.temporal, whose keyword arguments `temporal_kwargs`
    takes) and stores the accumulated, unfiltered result as the next frame's history.  The
    context's scene must be set, by the caller or by frame(scene=...); camera and params are
    set by every frame.

    With resident=True the frame's colour, moments, features and ids and the history (a
    ping-pong pair) live in torch tensors on the context's device, and a frame is the
    device-pointer forms enqueued on one stream of the accumulator's own, then one copy of the
    returned image to the host: the history never crosses the host link.  The images are the
    non-resident accumulator's, bit for bit.

    With refit=True the frames after the first move the spheres and the camera through
    Context.update_scene (the traversal tables refit, the candidate lists built on the device)
    in place of set_scene and set_camera, while the scene's sphere count, radii, colours,
    materials and fuzz stay as they were; a frame that changes any of them falls back to
    set_scene.  The images are those of refit=False, bit for bit."""

    def __init__(self, ctx: Context, width, height, spp, bounces, seed=1, sky=INIT_COLOR, resident=False,
                 refit=False, **temporal_kwargs):
        self.ctx, self.width, self.height, self.spp, self.bounces = ctx, int(width), int(height), int(spp), int(bounces)
        self.seed, self.sky, self.kwargs = int(seed), sky, temporal_kwargs
        self.resident = bool(resident)
        self.refit = bool(refit)
        self._dev = None  # the resident tensors, made by the first resident frame
        self.reset()

    def reset(self) -> None:
        """Forget the history and start the seeds again: the next frame passes through."""
        self.frame_index = 0
        self._history = None  # ((rgba, mom, feat, ids), view, eye); resident: (slot, view, eye)
        self._spheres = None  # (n, 4): {C.xyz, r} of the last frame(scene=...)'s scene
        self._fixed = None    # refit: (radii, colors, materials, fuzz) of the scene the context's tables were built for
        self._cam_set = False  # refit: this accumulator has set the camera (and with it the sky)

    def _set_scene(self, scene, view, eye):
        """set_scene for frame(scene=...) (refit: update_scene with the frame's camera, where
        only the centres changed); returns the motion table against the previous frame's scene,
        or None where there is none to follow, and whether the camera was moved as well."""
        now = np.concatenate([scene.centers[:, :3], scene.radii[:, None]], axis=1).astype(np.float32)
        motion = None
        if self._spheres is not None:
            if len(now) != len(self._spheres):
                raise ValueError(f"frame: {len(now)} spheres now, {len(self._spheres)} in the previous frame's scene")
            if self._history is not None:
                motion = np.ascontiguousarray(np.concatenate([now, self._spheres], axis=1))
        fixed = (scene.radii, scene.colors, scene.materials, scene.fuzz)
        moved_camera = False
        if self.refit and self._fixed is not None and all(np.array_equal(a, b) for a, b in zip(fixed, self._fixed)):
            if self._cam_set:
                self.ctx.update_scene(scene.centers, view, _eye4(eye))
                moved_camera = True
            else:
                self.ctx.update_scene(scene.centers)
        else:
            self.ctx.set_scene(scene)
            self._fixed = tuple(np.array(a, copy=True) for a in fixed) if self.refit else None
        self._spheres = now
        return motion, moved_camera

    def frame(self, view, eye, denoise=None, scene=None) -> np.ndarray:
        """The accumulated (H, W, 4) image of the next frame seen through `view` from `eye`;
        with denoise=dict(...) (denoise_variance's keyword arguments, {} for its defaults)
        that filter's result on the accumulated colour and moments instead.  The history
        kept is the unfiltered one either way.  With scene=..., that scene is set first
        (Context.set_scene) and the history follows its spheres from where the previous
        frame's scene had them (sphere_motion; the same spheres in the same order: ValueError
        when the counts differ); the first scene given has none to follow."""
        c, w, h = self.ctx, self.width, self.height
        motion, moved_camera = self._set_scene(scene, view, eye) if scene is not None else (None, False)
        if not moved_camera:
            if self.refit and self._cam_set:
                c.update_scene(None, view, _eye4(eye))
            else:
                c.set_camera(view, _eye4(eye), self.sky)
                self._cam_set = True
        c.set_params(w, h, self.spp, self.bounces, self.seed + self.frame_index)
        kw = dict(self.kwargs) if motion is None else dict(self.kwargs, motion=motion)
        if self.resident:
            return self._resident_frame(view, eye, denoise, kw)
        rgba, mom = c.render_moments(0, h, 0, w)
        feat, ids = c.render_features(0, h, 0, w, ids=True)
        hist, pv, pe = self._history if self._history is not None else (None, None, None)
        out, out_mom = c.temporal(rgba.reshape(h, w, 4), mom, feat, ids, view, eye, hist, pv, pe, **kw)
        self._history = ((out, out_mom, feat, ids), _view16(view).copy(), _eye4(eye))
        self.frame_index += 1
        if denoise is not None:
            return c.denoise_variance(out, feat, out_mom, **denoise)
        return out

    def _resident_frame(self, view, eye, denoise, kw):
        import torch
        c, w, h, n = self.ctx, self.width, self.height, self.width * self.height
        if self._dev is None:
            dev = torch.device("cuda", c.device)
            f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)  # noqa: E731
            slot = lambda: dict(rgba=f32(n, 4), mom=f32(n, 4), feat=f32(n, 8),  # noqa: E731
                                ids=torch.zeros(n, dtype=torch.int32, device=dev))
            self._dev = dict(device=dev, stream=torch.cuda.Stream(device=dev), raw_rgba=f32(n, 4), raw_mom=f32(n, 4),
                             slots=(slot(), slot()), filtered=None, scratch=None, table=None)
            torch.cuda.synchronize(dev)  # the tensors are zeroed before the stream below writes them
        d = self._dev
        stream, s = d["stream"], d["stream"].cuda_stream
        cur = d["slots"][self.frame_index & 1]
        c.synchronize()  # the scene, camera and params are in place
        c.render_moments_async(0, h, 1, 1, 0, 0, w, d_rgba=d["raw_rgba"].data_ptr(), d_mom=d["raw_mom"].data_ptr(), stream=s)
        c.render_features_async(0, h, 1, 1, 0, 0, w, cur["feat"].data_ptr(), cur["ids"].data_ptr(), s)
        d_hist = pv = pe = None
        if self._history is not None:
            prev, pv, pe = self._history
            d_hist = tuple(prev[k].data_ptr() for k in ("rgba", "mom", "feat", "ids"))
        motion = kw.pop("motion", None)
        if motion is not None:
            if d["table"] is None or d["table"].numel() != motion.size:
                d["table"] = torch.zeros(motion.size, dtype=torch.float32, device=d["device"])
                torch.cuda.synchronize(d["device"])
            with torch.cuda.stream(stream):
                d["table"].copy_(torch.from_numpy(motion.reshape(-1)), non_blocking=True)
            kw.update(d_motion=d["table"].data_ptr(), n_spheres=len(motion))
        c.temporal_async(w, h, d["raw_rgba"].data_ptr(), d["raw_mom"].data_ptr(), cur["feat"].data_ptr(),
                         cur["ids"].data_ptr(), view, eye, d_hist, pv, pe, d_out_rgba=cur["rgba"].data_ptr(),
                         d_out_mom=cur["mom"].data_ptr(), stream=s, **kw)
        result = cur["rgba"]
        if denoise is not None:
            if "g_data" in denoise or "variance" in denoise:
                raise ValueError("a resident frame returns the filtered image alone: no g_data or variance")
            levels = int(denoise.get("levels", 3))
            need = denoise_scratch_bytes(w, h, levels)
            if d["filtered"] is None or d["scratch"].numel() < need:
                d["filtered"] = torch.zeros((n, 4), dtype=torch.float32, device=d["device"])
                d["scratch"] = torch.zeros(max(need, 16), dtype=torch.uint8, device=d["device"])
                torch.cuda.synchronize(d["device"])
            c.denoise_variance_async(w, h, cur["rgba"].data_ptr(), cur["feat"].data_ptr(), cur["mom"].data_ptr(),
                                     d_out=d["filtered"].data_ptr(), d_scratch=d["scratch"].data_ptr(), stream=s, **denoise)
            result = d["filtered"]
        with torch.cuda.stream(stream):
            host = result.to("cpu")  # the one copy of the frame that crosses the host link
        stream.synchronize()
        self._history = (cur, _view16(view).copy(), _eye4(eye))
        self.frame_index += 1
        return host.numpy().reshape(h, w, 4)


class Globals:
    """The reference's global state (Globals.hpp:8-37) bound to a device context.

    g_width/g_height/g_samples/g_bounces, the scene SoA, viewMatrix/eyePos/
    initColor and the g_data framebuffer (RGB8, g_width*g_height*3 bytes).
    """

    def __init__(self, scene: Scene, width=1440, height=1440, samples=100, bounces=10, seed=1, eye=DEFAULT_EYE,
                 look_at=DEFAULT_LOOK_AT, up=DEFAULT_UP, init_color=INIT_COLOR, device=0, context=None,
                 devices=None):
        self.g_width, self.g_height, self.g_samples, self.g_bounces = width, height, samples, bounces
        self.g_stride = 3
        self.g_size = width * height * 3
        self.g_data = np.zeros(self.g_size, np.uint8)
        self.eyePos, self.lookAt, self.upDir, self.initColor = eye, look_at, up, init_color
        self.viewMatrix = camera_basis(eye, look_at, up)
        self.scene = scene
        self.seed = seed
        self.ctx = context or Context(device, devices=devices)
        self._lock = threading.Lock()
        self.sync()

    def sync(self) -> None:
        """Push the current globals to the device context."""
        self.ctx.set_scene(self.scene)
        self.ctx.set_camera(self.viewMatrix, self.eyePos, self.initColor)
        self.ctx.set_params(self.g_width, self.g_height, self.g_samples, self.g_bounces, self.seed)


def SaveImage(g: Globals, directory: str = ".") -> str:
    """io::SaveImage (IOHelpers.hpp:24-27): g_data as a 24-bit BMP named
    output{g_samples}s{g_bounces}b.bmp, in stbi_write_bmp's layout; returns the path."""
    import os
    path = os.path.join(directory, f"output{g.g_samples}s{g.g_bounces}b.bmp")
    data = np.ascontiguousarray(g.g_data, np.uint8)
    _native.check(_native.lib().spt_save_bmp(path.encode(), g.g_width, g.g_height, g.g_stride, _p(data)))
    return path


def RenderSegment(segment: RenderSegmentData, g: Globals) -> np.ndarray:
    """SingleThreadPathTracer.hpp:114-137: render the rectangle into g.g_data.
    Returns the float pixel colours (region-local, the value io::WritePixel gets)."""
    return g.ctx.render_segment(segment.yBegin, segment.yEnd, segment.xBegin, segment.xEnd, g.g_data, task=False)


def RenderSegmentTask(segment: RenderSegmentData, g: Globals) -> np.ndarray:
    """TaskBasedPathTracer.hpp:54-206 semantics (10-pass cap, count-weighted
    resolve), including the colorIndex stride of non-square tiles (lines 103, 186:
    rows strided by segmentHeight, so pixels alias and some indices stay empty)."""
    return g.ctx.render_segment(segment.yBegin, segment.yEnd, segment.xBegin, segment.xEnd, g.g_data, task=True)


def MakeRenderSegmentData(i, j, segment_width, segment_height, g: Globals) -> RenderSegmentData:
    """Renderer.hpp:232-240."""
    yB = segment_height * j
    yE = g.g_height if yB + segment_height > g.g_height else yB + segment_height
    xB = segment_width * i
    xE = g.g_width if xB + segment_width > g.g_width else xB + segment_width
    return RenderSegmentData(yB, yE, xB, xE)


def RenderImageParallelMain(g: Globals, thread_count: int = 4, task: bool = False) -> None:
    """Renderer.hpp:257-302: a thread_count x thread_count tile grid, at most
    thread_count RenderJob threads in flight, each calling the drop-in entry point
    concurrently on the shared context."""
    tc = thread_count + (thread_count % 2)
    sw, sh = g.g_width // tc, g.g_height // tc
    segments = [MakeRenderSegmentData(i, j, sw, sh, g) for j in range(tc) for i in range(tc)]
    fn = RenderSegmentTask if task else RenderSegment
    errors = []
    sem = threading.Semaphore(tc)

    def job(seg):
        try:
            fn(seg, g)
        except Exception as e:  # surfaced after join
            errors.append(e)
        finally:
            sem.release()

    threads = []
    for seg in segments:
        sem.acquire()
        t = threading.Thread(target=job, args=(seg,))
        t.start()
        threads.append(t)
    for t in threads:
        t.join()
    if errors:
        raise errors[0]


def RenderImage(g: Globals) -> None:
    """Renderer.hpp:304-308: RenderSegmentTask over the full frame."""
    RenderSegmentTask(RenderSegmentData(0, g.g_height, 0, g.g_width), g)
