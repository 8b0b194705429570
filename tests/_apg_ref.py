"""numpy mirror of adaptive projected guidance (include/avdiff_hip.h, "adaptive projected guidance"): the direction with momentum in
fp32, the three moments in fp64, the coefficients rounded once to fp32, and the combine in fp32 with one rounding per operation.
Shared by tests/test_apg_cpu.py and tests/test_gpu_apg.py; the per-sample helpers are those of _cfg_ref."""
import numpy as np

from _cfg_ref import _per_sample, ulps  # noqa: F401  (ulps: re-exported for the tests)

F32 = np.float32


def direction(c, u, beta=0.0, m_prev=None):
    """d = (c - u) + beta m_prev in fp32, one rounding per operation; beta == 0 (no buffer) is c - u itself (item 2)"""
    d0 = np.asarray(c, F32) - np.asarray(u, F32)
    if beta == 0.0:
        assert m_prev is None
        return d0
    return d0 + F32(beta) * np.asarray(m_prev, F32)


def moments(c, d):
    """(S_dd, S_dc, S_cc) per sample in fp64 (item 3; the device sums 1024-element chunks, then the chunks: another order)"""
    c = np.asarray(c, np.float64).reshape(np.shape(c)[0], -1)
    d = np.asarray(d, np.float64).reshape(np.shape(d)[0], -1)
    return (d * d).sum(axis=1), (d * c).sum(axis=1), (c * c).sum(axis=1)


def coefficients(c, d, g, r=0.0, eta_p=0.0):
    """(s_b, k_b, w_b) of item 4, fp32 [B] each"""
    sdd, sdc, scc = moments(c, d)
    B = sdd.shape[0]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        s = np.minimum(1.0, np.float64(F32(r)) / np.sqrt(sdd)).astype(F32)
        k = ((1.0 - np.float64(F32(eta_p))) * sdc / scc).astype(F32)
    s = np.where((F32(r) == 0) | (sdd == 0.0) | ~np.isfinite(s), F32(1.0), s).astype(F32)
    k = np.where((scc == 0.0) | ~np.isfinite(k), F32(0.0), k).astype(F32)
    gb = np.broadcast_to(np.asarray(g, F32).reshape(-1), (B,))
    w = ((gb - F32(1.0)) * s).astype(F32)
    return s, k, w


def combine_f32(c, d, w, k):
    """e = c + w_b (d - k_b c) in fp32, in that order, one rounding per operation (item 5)"""
    c, d = np.asarray(c, F32), np.asarray(d, F32)
    wb, kb = _per_sample(w, c.shape[0], c.ndim), _per_sample(k, c.shape[0], c.ndim)
    return (c + wb * (d - kb * c)).astype(F32)


def apg(c, u, g, r=0.0, eta_p=0.0, beta=0.0, m_prev=None):
    """(e, d, (s, k, w)): what functional.apg_guidance computes on latent-layout tensors; d is the momentum buffer's new content"""
    d = direction(c, u, beta, m_prev)
    s, k, w = coefficients(c, d, g, r, eta_p)
    return combine_f32(c, d, w, k), d, (s, k, w)


def cancellation_free(c, d, floor=0.05):
    """the coefficient checks' input condition: |S_dc| >= floor sqrt(S_dd S_cc) for every sample, so that cancellation in S_dc cannot
    turn the fp64 summation order into fp32 ulps of k_b"""
    sdd, sdc, scc = moments(c, d)
    return bool((np.abs(sdc) >= floor * np.sqrt(sdd * scc)).all())
