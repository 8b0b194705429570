"""numpy mirror of the canvas-keyed latent guide (include/avdiff_hip.h, "canvas-keyed known noise"), built on ``_guide_ref`` and
``_canvas_noise_ref``: the known normals of the per-sample guide stream for every canvas position, [P, outer*inner], gathered into
window layout — which is the contract's definition.  Shared by tests/test_canvas_guide_cpu.py and tests/test_gpu_canvas_guide.py."""
import numpy as np

from _canvas_noise_ref import gather_windows
from _consensus_ref import dims
from _guide_ref import abar_at, known_normals


def canvas_known_normals(seed, shape, hop, window_offset=0):
    """float64 array of ``shape`` (a window batch [N,C,T,H,W] or [N,Ca,F]): window b's element (o, l, i) takes the per-sample guide
    stream's value for sample p = (window_offset + b)*hop + l and element o*inner + i.  The draw starts at the first window's
    position, so a window offset next to 2^32 costs nothing."""
    shape = tuple(int(s) for s in shape)
    outer, L, inner = dims(shape)
    P = (shape[0] - 1) * hop + L
    draw = known_normals(seed, window_offset * hop, P, outer * inner)
    return gather_windows(draw, shape, hop)


def q_f64(known, tau, abar, seed, hop, window_offset=0):
    """q(tau[b]) = A x_k + S n_k(p) for every window of known in float64 (x_k itself where a == 1)."""
    k = np.asarray(known, dtype=np.float64)
    a = abar_at(abar, tau).reshape((k.shape[0],) + (1,) * (k.ndim - 1))
    n = canvas_known_normals(seed, k.shape, hop, window_offset)
    return np.where(a == 1.0, k, np.sqrt(a) * k + np.sqrt(np.maximum(1.0 - a, 0.0)) * n)
