"""numpy fp32 mirror of the latent window consensus (contract in include/avdiff_hip.h, avd_window_consensus_f32).

``consensus_f32`` follows the contract operation by operation with ``np.float32`` arrays: numpy rounds every multiply, add and divide
to fp32 and contracts nothing, and the sums run over the covering windows in increasing order from 0 — the kernel's order, so a GPU
result is compared bit for bit.  ``consensus_f64`` is the same map in fp64 (linearity checks)."""
import numpy as np


def window_range(p, L, hop, N):
    """(lo, hi): the windows k with 0 <= p - k*hop < L, as ``window_range`` in csrc/stitch.hip."""
    hi = min(p // hop, N - 1)
    q = p - L + 1
    lo = 0 if q <= 0 else (q + hop - 1) // hop
    return lo, hi


def dims(shape):
    """(outer, L, inner) of a window batch: video [N,C,T,H,W] slides along T, audio [N,Ca,F] along F."""
    if len(shape) == 5:
        return shape[1], shape[2], shape[3] * shape[4]
    if len(shape) == 3:
        return shape[1], shape[2], 1
    raise ValueError(shape)


def _consensus(z, hop, weights, dtype):
    z = np.array(z, dtype=dtype)                       # a copy: the caller's array stays
    N = z.shape[0]
    outer, L, inner = dims(z.shape)
    w = np.ones(L, dtype=dtype) if weights is None else np.asarray(weights, dtype=dtype)
    assert w.shape == (L,) and (w > 0).all()
    v = z.reshape(N, outer, L, inner)                  # a view: writes land in z
    for p in range((N - 1) * hop + L):
        lo, hi = window_range(p, L, hop, N)
        if lo >= hi:
            continue                                   # one window (or, with hop > L, none): not touched
        acc = np.zeros((outer, inner), dtype=dtype)
        nrm = dtype(0)
        for k in range(lo, hi + 1):
            q = p - k * hop
            acc = acc + w[q] * v[k, :, q, :]           # product rounded, then the sum rounded
            nrm = nrm + w[q]
        m = acc / nrm
        for k in range(lo, hi + 1):
            v[k, :, p - k * hop, :] = m
    return z


def consensus_f32(z, hop, weights=None):
    return _consensus(z, hop, weights, np.float32)


def consensus_f64(z, hop, weights=None):
    return _consensus(z, hop, weights, np.float64)


def windows_from_canvas(canvas, L, hop):
    """[C, P, ...] -> [N, C, L, ...] with P = (N-1)*hop + L."""
    P = canvas.shape[1]
    assert (P - L) % hop == 0
    return np.stack([canvas[:, k * hop:k * hop + L] for k in range((P - L) // hop + 1)], 0)


def overlaps_agree(z, hop):
    """every canvas position holds the same bits in all the windows that cover it"""
    N = z.shape[0]
    outer, L, inner = dims(z.shape)
    v = np.ascontiguousarray(z).reshape(N, outer, L, inner)
    for p in range((N - 1) * hop + L):
        lo, hi = window_range(p, L, hop, N)
        for k in range(lo + 1, hi + 1):
            if not np.array_equal(v[k, :, p - k * hop, :], v[lo, :, p - lo * hop, :]):
                return False
    return True
