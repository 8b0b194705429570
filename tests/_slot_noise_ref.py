"""numpy reference of the clip-keyed slot noise (include/avdiff_hip.h, "clip-keyed slot noise"): the per-sample stream's Philox4x32-10
and Box-Muller (tests/_noise_ref.py) under the domain word "SLOT", keyed by the clip position an element sits on.  Shared by
tests/test_slot_noise_cpu.py and the GPU tests of the slot entries at eta > 0."""
import numpy as np

import _noise_ref as NR

TAG = 0x534C4F54


def position_normals(seed: int, p, t, per: int) -> np.ndarray:
    """float64 [len(p), per]: row k = the normals of clip position p[k] (any Python ints, taken mod 2^32) at timestep t[k],
    elements e' = 0 .. per - 1"""
    p = np.array([int(v) % 2 ** 32 for v in p], dtype=np.uint64).astype(np.uint32)[:, None]
    t = np.array([int(v) % 2 ** 32 for v in t], dtype=np.uint64).astype(np.uint32)[:, None]
    n4 = (per + 3) // 4
    e4 = np.arange(n4, dtype=np.uint64).astype(np.uint32)[None, :]
    shape = (p.shape[0], n4)
    key = (np.uint32(seed & 0xFFFFFFFF), np.uint32(seed >> 32))
    x0, x1, x2, x3 = NR.philox4x32_10((np.broadcast_to(e4, shape), np.broadcast_to(p, shape), np.broadcast_to(t, shape), np.uint32(TAG)),
                                      key)
    n0, n1 = NR.box_muller(x0, x1)
    n2, n3 = NR.box_muller(x2, x3)
    return np.stack([n0, n1, n2, n3], axis=-1).reshape(p.shape[0], 4 * n4)[:, :per]


def clip_position(first: int, b: int, stride: int, slot_len: int, l: int, cursor: int = 0) -> int:
    """the contract's p, in exact integers"""
    return ((first + max(cursor, 0) + b * stride) * slot_len + l) % 2 ** 32


def normals(seed: int, t_now, shape, slot_len: int, first: int = 0, stride=None, cursor: int = 0) -> np.ndarray:
    """float64 array of ``shape`` = (B, outer, L, *inner): element (b, o, l, i) = the normal of its clip position at t_now[b, s], s =
    min(l // slot_len, S - 1), element e' = o * inner + i of the position's slice.  t_now: int [B, S]."""
    t_now = np.asarray(t_now, dtype=np.int64)
    B, S = t_now.shape
    stride = S if stride is None else stride
    outer, L_ = shape[1], shape[2]
    inner = int(np.prod(shape[3:], dtype=np.int64))
    ps, ts = [], []
    for b in range(B):
        for l in range(L_):
            ps.append(clip_position(first, b, stride, slot_len, l, cursor))
            ts.append(int(t_now[b, min(l // slot_len, S - 1)]))
    rows = position_normals(seed, ps, ts, outer * inner)                      # [B * L, outer * inner]
    return rows.reshape(B, L_, outer, inner).transpose(0, 2, 1, 3).reshape(shape)
