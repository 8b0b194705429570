"""numpy mirror of the CFG control (include/avdiff_hip.h, avd_cfg_control): the per-sample combine in fp32, the rescale factor s_b
from fp64 moments, and r(e) in fp32.  Shared by tests/test_cfg_rescale_cpu.py and tests/test_gpu_cfg_rescale.py."""
import numpy as np


def _per_sample(v, B, ndim, dtype=np.float32):
    return np.broadcast_to(np.asarray(v, dtype=dtype).reshape(-1), (B,)).reshape((B,) + (1,) * (ndim - 1))


def combine_f32(e_cond, e_null, g):
    """null + g_b (cond - null) per sample, in fp32 with one rounding per operation (as cfg_combine)."""
    c, n = np.asarray(e_cond, np.float32), np.asarray(e_null, np.float32)
    gb = _per_sample(g, c.shape[0], c.ndim)
    return n + gb * (c - n)


def sigma_f64(v):
    """per-sample unbiased std in fp64 from the moment sums: sqrt((S2 - S1^2 / n) / (n - 1)); NaN where the variance rounds below 0."""
    v = np.asarray(v, np.float64).reshape(np.shape(v)[0], -1)
    n = float(v.shape[1])
    s1, s2 = v.sum(axis=1), (v * v).sum(axis=1)
    with np.errstate(invalid="ignore"):
        return np.sqrt((s2 - s1 * s1 / n) / (n - 1.0))


def scale(c, y):
    """s_b = (float)(sigma_c / sigma_y), rounded once; 1 where sigma_y == 0 or the result is not finite.  c, y: [B, ...]."""
    sc, sy = sigma_f64(c), sigma_f64(y)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = (sc / sy).astype(np.float32)
    return np.where((sy == 0.0) | ~np.isfinite(r), np.float32(1.0), r).astype(np.float32)


def rescale_f32(e, phi, s):
    """r(e) per sample: e at phi 0, e s at phi 1, else phi (e s) + (1 - phi) e, every operation rounded to fp32."""
    e = np.asarray(e, np.float32)
    p, sb = _per_sample(phi, e.shape[0], e.ndim), _per_sample(s, e.shape[0], e.ndim)
    es = e * sb
    blend = p * es + (np.float32(1.0) - p) * e
    return np.where(p == 0, e, np.where(p == 1, es, blend)).astype(np.float32)


def cfg_rescale(c, y, phi):
    """r(y) with s_b from (c, y): what functional.cfg_rescale computes on latent-layout tensors."""
    return rescale_f32(y, phi, scale(c, y))


def ulps(a, b):
    """fp32 ulp distance, elementwise (same-sign finite values)"""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)
