"""numpy reference of the latent guide (include/avdiff_hip.h, avd_latent_guide): the known-noise stream (the seeded stream's
Philox4x32-10 + Box-Muller with the domain word TAG_K and no timestep), q(tau) and the blend, in float64.  Shared by
tests/test_latent_guide_cpu.py and tests/test_gpu_latent_guide.py."""
import numpy as np

from _noise_ref import box_muller, philox4x32_10

TAG_K = 0x4B4E5731


def known_normals(seed: int, sample_offset: int, B: int, per_sample: int, tag: int = TAG_K, t: int = 0) -> np.ndarray:
    """float64 [B, per_sample]: row b = the known-noise normals of sample sample_offset + b (counter (e >> 2, s, t, tag))."""
    n4 = (per_sample + 3) // 4
    e4 = np.arange(n4, dtype=np.uint64).astype(np.uint32)[None, :]
    s = ((sample_offset + np.arange(B, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint32)[:, None]
    key = (np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32))
    x0, x1, x2, x3 = philox4x32_10((np.broadcast_to(e4, (B, n4)), np.broadcast_to(s, (B, n4)), np.uint32(t), np.uint32(tag)), key)
    n0, n1 = box_muller(x0, x1)
    n2, n3 = box_muller(x2, x3)
    return np.stack([n0, n1, n2, n3], axis=-1).reshape(B, 4 * n4)[:, :per_sample]


def abar_at(abar, tau):
    """a(tau) per sample: alpha_bar[clamp(tau, 0, T-1)] for tau >= 0, 1 for tau < 0."""
    abar = np.asarray(abar, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.int64)
    return np.where(tau < 0, 1.0, abar[np.clip(tau, 0, abar.shape[0] - 1)])


def q_f64(known, tau, abar, seed, sample_offset=0):
    """q(tau[b]) for every sample of known [B, ...] in float64."""
    k = np.asarray(known, dtype=np.float64)
    B = k.shape[0]
    a = abar_at(abar, tau).reshape((B,) + (1,) * (k.ndim - 1))
    n = known_normals(seed, sample_offset, B, k[0].size).reshape(k.shape)
    return np.sqrt(a) * k + np.sqrt(np.maximum(1.0 - a, 0.0)) * n


def blend_f64(m, q, z):
    m = np.broadcast_to(np.asarray(m, dtype=np.float64), np.shape(z))
    return np.where(m == 0, z, np.where(m == 1, q, (1.0 - m) * z + m * q))
