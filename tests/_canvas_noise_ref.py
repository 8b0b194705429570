"""numpy mirror of the canvas-keyed noise stream (include/avdiff_hip.h, "canvas-keyed noise"), built on ``_noise_ref.normals``: draw the
per-sample stream for every canvas position, [P, outer*inner], and gather it into window layout.  Shared by
tests/test_canvas_noise_cpu.py and tests/test_gpu_canvas_noise.py."""
import numpy as np

from _consensus_ref import dims
from _noise_ref import normals


def canvas_draw(seed, t, P, per, p0=0):
    """float64 [P, per]: canvas positions p0 .. p0 + P - 1 at one timestep t, row p = sample p of the per-sample stream."""
    return normals(seed, p0, np.full(P, t, dtype=np.int64), per)


def canvas_normals(seed, t_now, shape, hop, window_offset=0):
    """float64 array of ``shape`` (a window batch [N,C,T,H,W] or [N,Ca,F]): window b's element (o, l, i) takes the per-sample
    stream's value for sample p = (window_offset + b)*hop + l, timestep t_now[b], element o*inner + i."""
    shape = tuple(int(s) for s in shape)
    N = shape[0]
    outer, L, inner = dims(shape)
    t_now = np.asarray(t_now, dtype=np.int64)
    assert t_now.shape == (N,)
    out = np.empty((N, outer, L, inner), dtype=np.float64)
    for b in range(N):
        p0 = (window_offset + b) * hop
        rows = canvas_draw(seed, int(t_now[b]), L, outer * inner, p0)          # [L, outer*inner]
        out[b] = rows.reshape(L, outer, inner).transpose(1, 0, 2)
    return out.reshape(shape)


def gather_windows(draw, shape, hop, window_offset=0):
    """window layout of a full draw [P, outer*inner] (any dtype; one timestep for all windows): out[b, o, l, i] = draw[(window_offset
    + b)*hop + l, o*inner + i].  The same gather serves a GPU draw from ``gaussian_noise``."""
    shape = tuple(int(s) for s in shape)
    N = shape[0]
    outer, L, inner = dims(shape)
    out = np.empty((N, outer, L, inner), dtype=draw.dtype)
    for b in range(N):
        p0 = (window_offset + b) * hop
        out[b] = draw[p0:p0 + L].reshape(L, outer, inner).transpose(1, 0, 2)
    return out.reshape(shape)
