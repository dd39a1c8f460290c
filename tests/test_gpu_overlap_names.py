"""Which overlap an argument error names must not depend on what lies beside a buffer.

spt_temporal refuses an output that overlaps an input or the other output and names the pair.
An output that overlaps one buffer by its first or last bytes runs on into whatever the
allocator placed next to it, so several overlaps can hold at once; tests/test_gpu_temporal.py
asks for the intended pair by name with buffers from numpy's allocator, whose neighbours vary
from run to run.  Here the neighbours are chosen: every buffer is a view into one arena, laid
out so that the stray overlap exists, and the intended pair must still be the one named --
the buffer the output begins in.
"""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p
W, H = 33, 18
N = W * H * 16  # bytes of a float4 plane


@pytest.fixture(scope="module")
def spt():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import simplepathtracer_amd as m
    m.lib()
    return m


def test_temporal_names_the_buffer_an_output_begins_in(spt):
    L = spt._native.lib()
    # one arena, the planes back to back: ... ids | out | hist_feat ...
    order = (("gap", N), ("rgba", N), ("mom", N), ("feat", 2 * N), ("h_rgba", N), ("h_mom", N), ("ids", N // 4), ("out", N),
             ("h_feat", 2 * N), ("h_ids", N // 4), ("out_mom", N))
    arena = np.zeros(sum(s for _, s in order) + 64, np.uint8)
    base = (arena.ctypes.data + 63) & ~63
    at, off = {}, 0
    for name, size in order:
        at[name] = base + off
        off += size
    view = np.eye(4, dtype=np.float32).reshape(16)
    eye = np.zeros(4, np.float32)
    vp, ep = view.ctypes.data_as(P), eye.ctypes.data_as(P)
    c = spt.Context(0)
    try:
        h = c.handle

        def call(fn, o, m):
            a = [P(at[k]) for k in ("rgba", "mom", "feat", "ids")] + [vp, ep] + \
                [P(at[k]) for k in ("h_rgba", "h_mom", "h_feat", "h_ids")] + [vp, ep]
            if fn == "async":
                return L.spt_temporal_async(h, W, H, *a, 0.25, 0.1, 64.0, P(o), P(m), None)
            return L.spt_temporal(h, W, H, *a, 0.25, 0.1, 64.0, P(o), P(m))

        for fn in ("blocking", "async"):
            # out_mom begins in out_rgba's last bytes; its tail lies in hist_feat
            assert call(fn, at["out"], at["out"] + N - 4) == 1
            assert L.spt_last_error(h) == b"out_rgba overlaps out_mom", fn
            # out_mom begins in ids' last bytes; its tail lies in out_rgba
            assert call(fn, at["out"], at["ids"] + N // 4 - 4) == 1
            assert L.spt_last_error(h) == b"out_mom overlaps ids", fn
            # out_rgba begins in hist_mom's last bytes; its tail covers ids and reaches out_mom
            assert call(fn, at["h_mom"] + N - 4, at["out"]) == 1
            assert L.spt_last_error(h) == b"out_rgba overlaps hist_mom", fn
            # an output whose tail alone reaches an input is still refused
            assert call(fn, at["out"], at["gap"] + 16) == 1
            assert L.spt_last_error(h) == b"out_mom overlaps rgba", fn
        assert not arena.any(), "a refused call wrote"
        # and buffers that only touch are accepted
        assert call("blocking", at["out"], at["out_mom"]) == 0, L.spt_last_error(h)
    finally:
        c.close()
