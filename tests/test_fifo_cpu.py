"""CPU tests of FIFO diagonal denoising: the plan's timestep tables, the driver's prompt-window indexing, and the bindings of the
slot-timestep and queue-shift entries."""
import re
from pathlib import Path

import pytest
import torch

from _slot_ref import tables

ROOT = Path(__file__).resolve().parent.parent
NEW = ("avd_denoise_step_slots_f32", "avd_embed_cfg_pair_slots_f32", "avd_cfg_unpatch_ddim_slots_f32",
       "avd_cfg_untoken_ddim_audio_slots_f32", "avd_fifo_shift_f32")


def _sched(n):
    """s_0 > ... > s_n = -1"""
    return torch.linspace(999, -1, n + 1).round().long()


# ------------------------------------------------------------------------------------------------- fifo_plan
@pytest.mark.parametrize("n,S", [(4, 2), (6, 3), (4, 4), (3, 1)])
def test_fifo_plan_every_slot_takes_every_step_in_order(n, S):
    from multimodal_diffusion_amd import schedule_utils as su
    s = _sched(n).tolist()
    rn, rp, sn, sp = su.fifo_plan(_sched(n), S)
    B = n // S
    assert rn.shape == rp.shape == (n - 1, B, S) and sn.shape == sp.shape == (B, S)
    assert all(t.dtype == torch.long for t in (rn, rp, sn, sp))
    rn, rp, sn, sp = rn.view(n - 1, n), rp.view(n - 1, n), sn.view(n), sp.view(n)       # queue slot q = sample q // S, slot q % S
    for K in (1, n, n + 3):
        for c in range(K):
            pairs = []
            if c < n:                                   # in the initial queue at slot c: the whole ramp, no shift
                pairs += [(int(rn[r, c]), int(rp[r, c])) for r in range(n - 1)]
            # steady iteration m: clip slot c sits at queue slot c - m (it enters at the tail after the shift of iteration c - n)
            pairs += [(int(sn[c - m]), int(sp[c - m])) for m in range(max(0, c - n + 1), c + 1)]
            steps = [p for p in pairs if p[0] != p[1]]
            assert steps == [(s[i], s[i + 1]) for i in range(n)], (K, c, pairs)
            assert all(p == (s[0], s[0]) for p in pairs if p[0] == p[1])
            assert pairs[-1][1] == -1                   # it leaves finished, in steady iteration c
    for row in list(rn) + [sn]:                         # cleaner towards the head at every iteration
        assert all(int(a) <= int(b) for a, b in zip(row[:-1], row[1:]))
    # after the ramp every slot stands where the steady state picks it up
    level = torch.full((n,), s[0])
    for r in range(n - 1):
        assert torch.equal(rn[r], level)
        level = rp[r].clone()
    assert torch.equal(level, sn)


def test_fifo_plan_refuses_what_it_cannot_plan():
    from multimodal_diffusion_amd import schedule_utils as su
    with pytest.raises(ValueError, match="multiple"):
        su.fifo_plan(_sched(5), 2)
    with pytest.raises(ValueError, match="strictly decreasing"):
        su.fifo_plan(torch.tensor([900, 500, 700, 100, -1]), 2)            # an up-jump
    with pytest.raises(ValueError, match="strictly decreasing"):
        su.fifo_plan(torch.tensor([900, 500, 500, 100, -1]), 2)            # equal neighbours
    with pytest.raises(ValueError, match="ends in -1"):
        su.fifo_plan(torch.tensor([900, 500, 100, 0]), 1)
    with pytest.raises(ValueError):
        su.fifo_plan(_sched(4), 0)


# ------------------------------------------------------------------------------------------------- prompt windows
def test_fifo_prompt_windows_slices_and_zero_pads():
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_windows
    B, S, hop, Lp = 2, 2, 3, 8
    audio = torch.arange(1, 2 * 17 + 1, dtype=torch.float32).view(2, 17)                   # [Ca, P]
    video = torch.arange(1, 2 * 17 * 6 + 1, dtype=torch.float32).view(2, 17, 2, 3)         # [C, P, H, W]
    for canvas in (audio, video):
        for m in (0, 1, 4):
            w = fifo_prompt_windows(canvas, m, B, S, hop, Lp)
            assert w.shape == (B, 2, Lp) + tuple(canvas.shape[2:])
            for k in range(B):
                p0 = (m + k * S) * hop
                n = max(0, min(Lp, 17 - p0))
                assert torch.equal(w[k, :, :n], canvas[:, p0:p0 + n])
                assert (w[k, :, n:] == 0).all()
    assert (fifo_prompt_windows(audio, 4, B, S, hop, Lp)[1] == 0).all()                    # wholly past the end: the null prompt
    assert (fifo_prompt_windows(audio, 0, B, S, hop, Lp)[0] != 0).all()
    with pytest.raises(ValueError):
        fifo_prompt_windows(torch.zeros(2, 3, 4), 0, B, S, hop, Lp)
    with pytest.raises(ValueError):
        fifo_prompt_windows(audio, -1, B, S, hop, Lp)


# ------------------------------------------------------------------------------------------------- bindings
def test_slot_entries_declared_exported_and_bound():
    from multimodal_diffusion_amd import _lib as L
    import multimodal_diffusion_amd as A
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    lib = L.lib()
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.avd_abi_version() == L.ABI_VERSION == 7
    assert "slot timesteps" in header and "FIFO queue shift" in header
    assert callable(A.fifo_denoise) and hasattr(A.DenoiseEngine, "step_slots")
    assert isinstance(A.DenoiseEngine.slots, property) and isinstance(A.DenoiseEngine.slot_len, property)


def test_slot_entries_refuse_before_any_launch():
    """argument checks run before any HIP call, so a CPU-only machine sees them"""
    import ctypes as C
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    p = 4096                                             # a non-null, 16-byte aligned stand-in: nothing is dereferenced
    # the fused updates: slots must be the geometry's S, audio chunks must not overlap
    assert lib.avd_cfg_unpatch_ddim_slots_f32(p, p, p, p, p, 1000, 2.0, 3, 2 * p, 2, 8, 4, 16, 32, 2, 4, 4, None) == L.EINVAL
    assert b"slots 3" in lib.avd_last_error()
    assert lib.avd_cfg_untoken_ddim_audio_slots_f32(p, p, p, p, p, 1000, 2.0, 19, 2 * p, 2, 8, 40, 4, 2, None) == L.EUNSUPPORTED
    assert b"non-overlapping" in lib.avd_last_error()
    assert lib.avd_cfg_untoken_ddim_audio_slots_f32(p, p, p, p, p, 1000, 2.0, 9, 2 * p, 2, 8, 40, 4, 4, None) == L.EINVAL
    # the shift: overlap, range of c, null key
    key = L.NoiseKey(7, 0)
    big = 1 << 30
    assert lib.avd_fifo_shift_f32(C.byref(key), 999, 4, p, p, big, 2, 8, 2, 2, 256, None) == L.EINVAL
    assert b"overlap" in lib.avd_last_error()
    assert lib.avd_fifo_shift_f32(C.byref(key), 999, 4, p, 2 * big, p + 64, 2, 8, 2, 2, 256, None) == L.EINVAL
    assert b"popped" in lib.avd_last_error()
    assert lib.avd_fifo_shift_f32(C.byref(key), 999, 2 ** 31, p, 2 * big, 3 * big, 2, 8, 2, 2, 256, None) == L.EINVAL
    assert b"2^32" in lib.avd_last_error()
    assert lib.avd_fifo_shift_f32(C.byref(key), 999, -1, p, 2 * big, 3 * big, 2, 8, 2, 2, 256, None) == L.EINVAL
    assert lib.avd_fifo_shift_f32(None, 999, 0, p, 2 * big, 3 * big, 2, 8, 2, 2, 256, None) == L.EINVAL


def test_reference_tables_cover_the_cases():
    for B, S in ((2, 2), (1, 4), (3, 2), (2, 10)):
        tn, tp = tables(B, S, seed=B * 16 + S)
        assert tn.shape == tp.shape == (B, S) and tn.dtype == torch.long
        assert ((tp < tn) | (tp == tn)).all()
