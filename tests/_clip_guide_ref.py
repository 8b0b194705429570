"""numpy reference of the clip-keyed latent guide (include/avdiff_hip.h, "clip-keyed latent guide"), in float64: the clip position of
"clip-keyed slot noise" (tests/_slot_noise_ref.py) taken signed and unwrapped, the known noise of the latent guide's stream
(tests/_guide_ref.py) keyed by that position, q(tau) and the blend per slot.  Shared by tests/test_clip_guide_cpu.py and the GPU tests
of the guided slot entries."""
import numpy as np

import _guide_ref as GR
import _slot_noise_ref as SN

LEAVE = -2 ** 63


def position(first: int, b: int, stride: int, slot_len: int, l: int, cursor: int = 0) -> int:
    """the contract's p in exact integers: signed, not wrapped.  Inside [0, 2^32) it is the slot noise's position."""
    p = (first + max(cursor, 0) + b * stride) * slot_len + l
    if 0 <= p < 2 ** 32:
        assert p == SN.clip_position(first, b, stride, slot_len, l, cursor)
    return p


def in_canvas(p: int, P: int) -> bool:
    """the out-of-canvas rule: an element is guided exactly when 0 <= p < P"""
    return 0 <= p < P


def clip_guide_slots(known, mask, tau, abar, z, seed, slot_len, first=0, stride=None, cursor=0, everywhere=False) -> np.ndarray:
    """float64 array of z's shape: blend(m(p), q_p(tau[b, s]), z) per element, z where p is outside the canvas or the slot's tau is
    LEAVE.  known / mask: [outer, P, *inner] (mask None = 1 everywhere); z: [B, outer, L, *inner]; tau: int [B, S]."""
    z = np.asarray(z, dtype=np.float64)
    known = np.asarray(known, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.int64)
    B, S = tau.shape
    stride = S if stride is None else stride
    outer, L_ = z.shape[1], z.shape[2]
    P = known.shape[1]
    per = outer * int(np.prod(z.shape[3:], dtype=np.int64))
    m_all = None if (mask is None or everywhere) else np.asarray(mask, dtype=np.float64)
    out = z.copy()
    for b in range(B):
        for l in range(L_):
            t = int(tau[b, min(l // slot_len, S - 1)])
            p = position(first, b, stride, slot_len, l, cursor)
            if t == LEAVE or not in_canvas(p, P):
                continue
            a = float(GR.abar_at(abar, [t])[0])
            n = GR.known_normals(seed, p, 1, per)[0].reshape(known[:, p].shape)
            q = known[:, p] if a == 1.0 else np.sqrt(a) * known[:, p] + np.sqrt(max(1.0 - a, 0.0)) * n
            out[b, :, l] = GR.blend_f64(1.0 if m_all is None else m_all[:, p], q, z[b, :, l])
    return out
