"""numpy reference of the seeded normal stream (include/avdiff_hip.h, avd_noise_key): Philox4x32-10 with the Random123 constants,
then Box-Muller in float64.  Shared by tests/test_noise_cpu.py and tests/test_gpu_seeded_noise.py."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
DOMAIN = 0x44444D31
_MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: 4 uint32 arrays (broadcastable), key: 2 uint32 arrays -> 4 uint32 arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint32) for c in ctr)
    k0, k1 = (np.asarray(k, dtype=np.uint32) for k in key)
    with np.errstate(over="ignore"):
        for r in range(10):
            if r:
                k0, k1 = k0 + W0, k1 + W1
            p0 = M0 * c0.astype(np.uint64)
            p1 = M1 * c2.astype(np.uint64)
            hi0, lo0 = (p0 >> np.uint64(32)).astype(np.uint32), (p0 & _MASK).astype(np.uint32)
            hi1, lo1 = (p1 >> np.uint64(32)).astype(np.uint32), (p1 & _MASK).astype(np.uint32)
            c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
    return c0, c1, c2, c3


def box_muller(xa, xb):
    """(xa, xb) uint32 -> (n_even, n_odd) float64, as the stream's contract writes it."""
    u = ((np.asarray(xa, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) + 1.0) * 2.0 ** -24
    v = (np.asarray(xb, dtype=np.uint32) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24
    r = np.sqrt(-2.0 * np.log(u))
    return r * np.cos(2.0 * np.pi * v), r * np.sin(2.0 * np.pi * v)


def normals(seed: int, sample_offset: int, t_now, per_sample: int) -> np.ndarray:
    """float64 [B, per_sample]: row b = sample sample_offset + b at timestep t_now[b]."""
    t_now = np.asarray(t_now, dtype=np.int64)
    B = t_now.shape[0]
    n4 = (per_sample + 3) // 4
    e4 = np.arange(n4, dtype=np.uint64).astype(np.uint32)[None, :]
    s = ((sample_offset + np.arange(B, dtype=np.int64)) & 0xFFFFFFFF).astype(np.uint32)[:, None]
    t = (t_now & 0xFFFFFFFF).astype(np.uint32)[:, None]
    key = (np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32))
    x0, x1, x2, x3 = philox4x32_10((np.broadcast_to(e4, (B, n4)), np.broadcast_to(s, (B, n4)), np.broadcast_to(t, (B, n4)),
                                    np.uint32(DOMAIN)), key)
    n0, n1 = box_muller(x0, x1)
    n2, n3 = box_muller(x2, x3)
    return np.stack([n0, n1, n2, n3], axis=-1).reshape(B, 4 * n4)[:, :per_sample]
