"""numpy reference of the renoise of RePaint resampling (include/avdiff_hip.h, "renoise") in float64: the renoise stream (the seeded
stream's Philox4x32-10 + Box-Muller with the domain word TAG_R and the visit in the timestep's place), the forward jump, the guide's
blend at t_to, and the canvas keying of both.  Built on ``_noise_ref`` (through ``_guide_ref.known_normals``), ``_guide_ref`` and the
canvas gathers.  Shared by tests/test_resample_cpu.py and tests/test_gpu_resample.py."""
import numpy as np

import _canvas_guide_ref as CG
import _guide_ref as G
from _canvas_noise_ref import gather_windows
from _consensus_ref import dims

TAG_R = 0x52504E31


def renoise_normals(seed, sample_offset, B, per_sample, visit):
    """float64 [B, per_sample]: row b = n_r of sample sample_offset + b, counter (e >> 2, s, visit, TAG_R)"""
    return G.known_normals(seed, sample_offset, B, per_sample, tag=TAG_R, t=visit)


def canvas_renoise_normals(seed, shape, hop, visit, window_offset=0):
    """float64 array of ``shape`` (a window batch): element (o, l, i) of window b takes n_r of sample p = (window_offset + b)*hop + l,
    element o*inner + i"""
    shape = tuple(int(s) for s in shape)
    outer, L, inner = dims(shape)
    P = (shape[0] - 1) * hop + L
    return gather_windows(renoise_normals(seed, window_offset * hop, P, outer * inner, visit), shape, hop)


def coef(abar, t_from, t_to):
    """(identity [B] bool, A [B], S [B]) from the fp32 table: the identity case is !(a_t < a_f)"""
    af, at = G.abar_at(abar, t_from), G.abar_at(abar, t_to)
    same = ~(at < af)
    rho = np.where(same, 1.0, at / np.where(af == 0, 1.0, af))
    return same, np.sqrt(rho), np.sqrt(np.maximum(1.0 - rho, 0.0))


def _jump(z, n, abar, t_from, t_to):
    z = np.asarray(z, dtype=np.float64)
    bshape = (z.shape[0],) + (1,) * (z.ndim - 1)
    same, A, S = (v.reshape(bshape) for v in coef(abar, t_from, t_to))
    return np.where(same, z, A * z + S * n)


def renoise_f64(z, t_from, t_to, abar, seed, visit, sample_offset=0, known=None, mask=None, guide_seed=0, guide_offset=None):
    """the per-sample entry: out[b] = the jump of z[b]; with ``known`` the guide's blend(mask, q(t_to), out) (mask None = 1)"""
    z = np.asarray(z, dtype=np.float64)
    n = renoise_normals(seed, sample_offset, z.shape[0], z[0].size, visit).reshape(z.shape)
    out = _jump(z, n, abar, t_from, t_to)
    if known is not None:
        q = G.q_f64(known, t_to, abar, guide_seed, sample_offset if guide_offset is None else guide_offset)
        out = G.blend_f64(1.0 if mask is None else mask, q, out)
    return out


def renoise_canvas_f64(z, t_from, t_to, abar, seed, visit, hop, window_offset=0, known=None, mask=None, guide_seed=0):
    """the canvas entry: renoise stream and known noise keyed by canvas position, one window offset for both"""
    z = np.asarray(z, dtype=np.float64)
    out = _jump(z, canvas_renoise_normals(seed, z.shape, hop, visit, window_offset), abar, t_from, t_to)
    if known is not None:
        q = CG.q_f64(known, t_to, abar, guide_seed, hop, window_offset)
        out = G.blend_f64(1.0 if mask is None else mask, q, out)
    return out
