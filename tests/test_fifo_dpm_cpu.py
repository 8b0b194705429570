"""CPU tests of FIFO diagonal denoising with DPM-Solver++(2M): the plan's t_last tables, a toy queue in numpy that shows the history
staying with its slot, and the bindings of the slot DPM entries and of the queue shift with history."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import _dpm_ref as D
import _slot_dpm_ref as SD
import _slot_ref as SR

ROOT = Path(__file__).resolve().parent.parent
NEW = ("avd_cfg_unpatch_dpmpp_2m_slots_f32", "avd_cfg_untoken_dpmpp_2m_audio_slots_f32", "avd_denoise_step_slots_dpmpp_2m_f32",
       "avd_fifo_shift_hist_f32")


def _sched(n):
    """s_0 > ... > s_n = -1"""
    return torch.linspace(999, -1, n + 1).round().long()


def _seen(plan, last, n, c):
    """every (t_last, t_now, t_prev) clip slot c meets on its way through a queue of n slots"""
    rn, rp, rl = (t.reshape(n - 1, n) for t in (plan[0], plan[1], last[0]))          # queue slot q = sample q // S, slot q % S
    sn, sp, sl = (t.reshape(n) for t in (plan[2], plan[3], last[1]))
    seen = []
    if c < n:                                   # in the initial queue at slot c: the whole ramp, no shift
        seen += [(int(rl[r, c]), int(rn[r, c]), int(rp[r, c])) for r in range(n - 1)]
    # steady iteration m: clip slot c sits at queue slot c - m (it enters at the tail after the shift of iteration c - n)
    seen += [(int(sl[c - m]), int(sn[c - m]), int(sp[c - m])) for m in range(max(0, c - n + 1), c + 1)]
    return seen


# ------------------------------------------------------------------------------------------------- fifo_plan_last
@pytest.mark.parametrize("n,S", [(4, 2), (6, 3), (4, 4), (3, 1)])
def test_every_slot_sees_its_own_triples_in_order(n, S):
    from multimodal_diffusion_amd import schedule_utils as su
    s = _sched(n).tolist()
    plan, last = su.fifo_plan(_sched(n), S), su.fifo_plan_last(_sched(n), S)
    assert last[0].shape == (n - 1, n // S, S) and last[1].shape == (n // S, S) and all(t.dtype == torch.long for t in last)
    want = [(([-1] + s)[i], s[i], s[i + 1]) for i in range(n)]          # (s_{i-1}, s_i, s_{i+1}), s_{-1} = -1
    for K in (max(1, n - 2), n, n + 3):                                 # clips shorter than, equal to and longer than the queue
        for c in range(K):
            seen = _seen(plan, last, n, c)
            assert [t for t in seen if t[1] != t[2]] == want, (K, c, seen)
            assert all(t == (-1, s[0], s[0]) for t in seen if t[1] == t[2]), (K, c, seen)      # otherwise only holds


def test_fifo_plan_last_refuses_what_fifo_plan_refuses():
    from multimodal_diffusion_amd import schedule_utils as su
    with pytest.raises(ValueError, match="multiple"):
        su.fifo_plan_last(_sched(5), 2)
    with pytest.raises(ValueError, match="strictly decreasing"):
        su.fifo_plan_last(torch.tensor([900, 500, 700, 100, -1]), 2)
    with pytest.raises(ValueError, match="strictly decreasing"):
        su.fifo_plan_last(torch.tensor([900, 500, 500, 100, -1]), 2)
    with pytest.raises(ValueError, match="ends in -1"):
        su.fifo_plan_last(torch.tensor([900, 500, 100, 0]), 1)
    with pytest.raises(ValueError):
        su.fifo_plan_last(_sched(4), 0)


# ------------------------------------------------------------------------------------------------- a toy queue
def _eps(z, t):
    """a local model: eps of an element depends on that element and its timestep alone"""
    return 0.1 * z * (1.0 + np.asarray(t, dtype=np.float64) / 1000.0)


@pytest.mark.parametrize("n,S,slot_len", [(4, 2, 2), (6, 3, 1), (4, 4, 1), (3, 1, 2)])
def test_toy_queue_keeps_every_history_with_its_slot(n, S, slot_len):
    """A queue in numpy, fp64: the update is _dpm_ref.step_f64 per slot, the shift _slot_ref.shift on z and on the history (zero tail),
    the tables fifo_plan + fifo_plan_last.  Every finished slot must be its own independent 2M trajectory: were a history to stay
    behind when its slot moves, or a waiting slot to pick one up, the second-order steps would read a neighbour's x0."""
    from multimodal_diffusion_amd import schedule_utils as su
    sched = _sched(n)
    s = sched.tolist()
    B, K, C = n // S, n + 3, 3
    noise = lambda c: torch.randn(C, slot_len, 2, generator=torch.Generator().manual_seed(100 + c), dtype=torch.float64)

    def alone(x):                      # clip slot on its own: n steps of the fp64 solver as one sample
        x, h = x.numpy()[None], np.zeros((1, C, slot_len, 2))
        for i in range(n):
            x, h = D.step_f64(x, _eps(x, s[i]), h, SD.ABAR, [([-1] + s)[i]], [s[i]], [s[i + 1]])
        return x[0]

    rn, rp, sn, sp = su.fifo_plan(sched, S)
    rl, sl = su.fifo_plan_last(sched, S)
    z = torch.stack([torch.cat([noise(b * S + k) for k in range(S)], 1) for b in range(B)])          # [B, C, S * slot_len, 2]
    h = torch.full_like(z, float("nan"))             # no initialisation needed: every slot's first step is first order

    def step(z, h, tl, tn, tp):
        t_el = SR.per_position(tn, z.shape[2], slot_len, z).numpy()
        out, x0 = SD.step_slots_np(D.step_f64, z.numpy(), _eps(z.numpy(), t_el), h.numpy(), tl, tn, tp, slot_len)
        return torch.from_numpy(np.ascontiguousarray(out)), torch.from_numpy(np.ascontiguousarray(x0))

    for r in range(n - 1):
        z, h = step(z, h, rl[r], rn[r], rp[r])
    for m in range(K):
        z, h = step(z, h, sl, sn, sp)
        z, popped = SR.shift(z, noise(n + m), slot_len)
        h, _ = SR.shift(h, torch.zeros(C, slot_len, 2, dtype=torch.float64), slot_len)
        ref = alone(noise(m))
        assert np.isfinite(popped.numpy()).all()
        assert np.allclose(popped.numpy(), ref, rtol=1e-12, atol=1e-13), (m, float(np.abs(popped.numpy() - ref).max()))
    if n >= 3:      # the second-order steps are live: a first-order trajectory is something else
        x, hh = noise(0).numpy()[None], np.zeros((1, C, slot_len, 2))
        for i in range(n):
            x, hh = D.step_f64(x, _eps(x, s[i]), hh, SD.ABAR, [-1], [s[i]], [s[i + 1]])
        assert not np.allclose(x[0], alone(noise(0)), rtol=1e-6)


# ------------------------------------------------------------------------------------------------- bindings
def test_slot_dpm_entries_declared_exported_and_bound():
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn, schedule_utils as su
    import multimodal_diffusion_amd as A
    import inspect
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    lib = L.lib()
    for name in NEW:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.avd_abi_version() == L.ABI_VERSION == 7
    assert "FIFO queue shift with history" in header
    assert callable(Fn.dpmpp_2m_step_slots) and callable(su.fifo_plan_last) and callable(A.DenoiseEngine.fifo_shift)
    assert "t_last" in inspect.signature(A.DenoiseEngine.step_slots).parameters
    assert "t_last" in inspect.signature(Fn.slot_tables).parameters and "hist" in inspect.signature(Fn.fifo_shift).parameters


def test_slot_dpm_entries_refuse_before_any_launch():
    """argument checks run before any HIP call, so a CPU-only machine sees them"""
    import ctypes as C
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    p, big = 4096, 1 << 30                               # non-null, 16-byte aligned stand-ins: nothing is dereferenced
    video = (2, 8, 4, 16, 32, 2, 4, 4, None)
    # x0_hist: aligned (video), apart from z and z_out, and present
    assert lib.avd_cfg_unpatch_dpmpp_2m_slots_f32(p, 2 * big, p, p, p, p, 1000, 2.0, 2, 4 * big + 4, 3 * big, *video) == L.EUNSUPPORTED
    assert b"x0_hist" in lib.avd_last_error()
    assert lib.avd_cfg_unpatch_dpmpp_2m_slots_f32(p, 2 * big, p, p, p, p, 1000, 2.0, 2, 2 * big + 64, 3 * big, *video) == L.EINVAL
    assert b"x0_hist" in lib.avd_last_error()
    assert lib.avd_cfg_unpatch_dpmpp_2m_slots_f32(p, 2 * big, p, p, p, p, 1000, 2.0, 2, 3 * big + 64, 3 * big, *video) == L.EINVAL
    assert lib.avd_cfg_unpatch_dpmpp_2m_slots_f32(p, 2 * big, p, p, p, p, 1000, 2.0, 2, None, 3 * big, *video) == L.EINVAL
    assert lib.avd_cfg_unpatch_dpmpp_2m_slots_f32(p, 2 * big, None, p, p, p, 1000, 2.0, 2, 4 * big, 3 * big, *video) == L.EINVAL
    assert lib.avd_cfg_unpatch_dpmpp_2m_slots_f32(p, 2 * big, p, p, p, p, 1000, 2.0, 3, 4 * big, 3 * big, *video) == L.EINVAL
    assert b"slots 3" in lib.avd_last_error()
    audio = (p, 2 * big, p, p, p, p, 1000, 2.0)
    assert lib.avd_cfg_untoken_dpmpp_2m_audio_slots_f32(*audio, 19, 4 * big, 3 * big, 2, 8, 40, 4, 2, None) == L.EUNSUPPORTED
    assert b"non-overlapping" in lib.avd_last_error()
    assert lib.avd_cfg_untoken_dpmpp_2m_audio_slots_f32(*audio, 9, 4 * big, 3 * big, 2, 8, 40, 4, 4, None) == L.EINVAL
    # the shift with history: five buffers, pairwise apart
    key = L.NoiseKey(7, 0)
    dims = (2, 8, 2, 2, 256, None)
    bufs = [p, 2 * big, 3 * big, 4 * big, 5 * big]       # z_in, z_out, popped, hist_in, hist_out
    for i, j in ((0, 1), (0, 3), (0, 4), (1, 3), (1, 4), (3, 4), (2, 0), (2, 1), (2, 3), (2, 4)):
        b = list(bufs)
        b[i] = b[j] + 64
        assert lib.avd_fifo_shift_hist_f32(C.byref(key), 999, 4, *b, *dims) == L.EINVAL, (i, j)
        assert b"overlap" in lib.avd_last_error(), (i, j)
    assert lib.avd_fifo_shift_hist_f32(C.byref(key), 999, 4, p, 2 * big, 3 * big, None, 5 * big, *dims) == L.EINVAL
    assert lib.avd_fifo_shift_hist_f32(C.byref(key), 999, 2 ** 31, *bufs, *dims) == L.EINVAL
    assert b"2^32" in lib.avd_last_error()


def test_reference_tables_cover_the_cases():
    for B, S in ((2, 2), (2, 4), (3, 2), (2, 10)):
        tl, tn, tp = SD.tables3(B, S, seed=B * 16 + S)
        assert tl.shape == tn.shape == tp.shape == (B, S) and tl.dtype == torch.long
