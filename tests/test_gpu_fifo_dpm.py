"""FIFO diagonal denoising with DPM-Solver++(2M) on the GPU: the queue shift with history against its torch restatement, an elementwise
toy queue on the device against every slot's own fp32-mirror trajectory, and the driver on either solver against a loop written here
from its parts — everything bit for bit."""
import ctypes as C

import numpy as np
import pytest
import torch

import _dpm_ref as D
import _slot_dpm_ref as SD
import _slot_ref as SR
from _kit import ABAR, dev, engine, model  # noqa: F401  (dev, model are fixtures)

pytestmark = pytest.mark.gpu

GS = 3.5
SEED = 0x5EED0F1F0
SCHED4 = torch.tensor([999, 749, 499, 249, -1])


# ------------------------------------------------------------------------------------------------- fifo_shift with a history
@pytest.mark.parametrize("shape,slot_len", [((2, 8, 4, 16, 16), 2), ((2, 8, 40), 4), ((3, 8, 4, 16, 16), 1)])
def test_fifo_shift_with_history_equals_two_rolls(dev, shape, slot_len):
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(len(shape) + slot_len)
    z, hist = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
    c, t = 11, 999
    ref_z, ref_popped = Fn.fifo_shift(z, c, SEED, t, slot_len)
    out, popped, hist_out = Fn.fifo_shift(z, c, SEED, t, slot_len, hist=hist)
    assert torch.equal(out, ref_z) and torch.equal(popped, ref_popped)
    ref_h, _ = SR.shift(hist, torch.zeros((shape[1], slot_len) + tuple(shape[3:]), device=dev), slot_len)
    assert torch.equal(hist_out, ref_h)
    assert hist_out.data_ptr() != hist.data_ptr() and torch.isfinite(hist_out).all()
    # misaligned views take the one-element lanes: same bits (every buffer in turn on the video shapes; audio runs them anyway)
    B, L_ = shape[0], shape[2]
    inner = int(np.prod(shape[3:]))
    key = C.byref(Fn.noise_key(SEED, 0))

    def off(x):
        v = torch.empty(x.numel() + 1, device=dev)[1:].view(x.shape).copy_(x)
        assert v.data_ptr() % 16 != 0
        return v

    for which in ("z", "hist", "hist_out"):
        zi, hi = (off(z) if which == "z" else z), (off(hist) if which == "hist" else hist)
        o2, p2 = torch.empty_like(z), torch.empty_like(popped)
        h2 = off(hist) if which == "hist_out" else torch.empty_like(hist)
        L.check(L.lib().avd_fifo_shift_hist_f32(key, t, c, zi.data_ptr(), o2.data_ptr(), p2.data_ptr(), hi.data_ptr(), h2.data_ptr(), B,
                                                shape[1], L_ // slot_len, slot_len, inner, L.stream_ptr(dev)))
        assert torch.equal(o2, out) and torch.equal(p2, popped) and torch.equal(h2, hist_out), which


def test_fifo_shift_with_history_refuses_overlapping_buffers(dev):
    from multimodal_diffusion_amd import functional as Fn
    z, hist = torch.randn(2, 8, 40, device=dev), torch.randn(2, 8, 40, device=dev)
    with pytest.raises(ValueError, match="overlap"):
        Fn.fifo_shift(z, 0, SEED, 999, 4, hist=hist, hist_out=hist)              # in place
    with pytest.raises(ValueError, match="overlap"):
        Fn.fifo_shift(z, 0, SEED, 999, 4, hist=z)                                 # the history is the queue
    with pytest.raises(ValueError, match="overlap"):
        Fn.fifo_shift(z, 0, SEED, 999, 4, hist=hist, hist_out=z)
    both = torch.randn(2 * z.numel() - 8, device=dev)                             # two buffers sharing their last / first slot
    a, b = both[:z.numel()].view_as(z), both[z.numel() - 8:].view_as(z)
    with pytest.raises(ValueError, match="overlap"):
        Fn.fifo_shift(z, 0, SEED, 999, 4, hist=a, hist_out=b)
    with pytest.raises(ValueError, match="shape"):
        Fn.fifo_shift(z, 0, SEED, 999, 4, hist=hist[:, :, :36].contiguous())
    with pytest.raises(ValueError, match="hist_out goes with hist"):
        Fn.fifo_shift(z, 0, SEED, 999, 4, hist_out=hist)


# ------------------------------------------------------------------------------------------------- a toy queue on the device
@pytest.mark.parametrize("shape,slot_len", [((2, 4, 4, 4, 4), 2), ((3, 4, 8), 4)])
def test_toy_queue_on_the_device_keeps_every_history_with_its_slot(dev, shape, slot_len):
    """dpmpp_2m_step_slots + fifo_shift(hist=) with the local model eps = 0.1 z computed in torch: every finished slot equals its own
    trajectory through the numpy fp32 mirror, bit for bit — its history moved with it and no waiting slot picked one up"""
    from multimodal_diffusion_amd import functional as Fn, schedule_utils as su
    B, S = shape[0], shape[2] // slot_len
    n = B * S
    sched = torch.linspace(999, -1, n + 1).round().long()
    s = sched.tolist()
    rn, rp, sn, sp = su.fifo_plan(sched, S)
    rl, sl = su.fifo_plan_last(sched, S)
    z = Fn.canvas_noise(SEED, torch.full((B,), s[0]), shape, shape[2])
    h = torch.full(shape, float("nan"), device=dev)             # never read before it is written: every first step is first order
    tenth = np.float32(0.1)

    def alone(x):                                               # [C, slot_len, ...] -> its own n steps, one sample of the fp32 mirror
        x, hh = x.cpu().numpy()[None], np.zeros((1,) + tuple(x.shape), np.float32)
        for i in range(n):
            x, hh = D.step_f32(x, tenth * x, hh, SD.ABAR, [([-1] + s)[i]], [s[i]], [s[i + 1]])
        return torch.from_numpy(x[0])

    starts = [z[q // S][:, (q % S) * slot_len:(q % S + 1) * slot_len].clone() for q in range(n)]
    for r in range(n - 1):
        z = Fn.dpmpp_2m_step_slots(z, 0.1 * z, h, rl[r], rn[r], rp[r], ABAR, slot_len)
    for m in range(n + 2):
        z = Fn.dpmpp_2m_step_slots(z, 0.1 * z, h, sl, sn, sp, ABAR, slot_len)
        z, popped, h = Fn.fifo_shift(z, n + m, SEED, s[0], slot_len, hist=h)
        starts.append(z[B - 1][:, (S - 1) * slot_len:].clone())          # the slot that just entered
        assert torch.equal(popped.cpu(), alone(starts[m])), m
    assert torch.isfinite(z).all()


# ------------------------------------------------------------------------------------------------- fifo_denoise
def _setup(dev, mods, target, solver):
    """as test_gpu_fifo._setup: a queue of n = 4 slots (B = 2, S = 2), either target"""
    g = torch.Generator().manual_seed(17)
    if target == "video":
        eng = engine(mods, "video", (2, 8, 4, 16, 16), 10, guidance=GS, solver=solver)
        return eng, torch.randn(8, 150, generator=g).to(dev), 20
    eng = engine(mods, "audio", (2, 8, 8), 8, guidance=GS, solver=solver)
    return eng, torch.randn(8, 14, 8, 8, generator=g).to(dev), 2


def _loop(eng, canvas_p, hop, sched, K, seed):
    """fifo_denoise restated from its parts: the plan's tables, step_slots, the torch shift of z (and of engine.x0_hist), set_prompt"""
    from multimodal_diffusion_amd import functional as Fn, schedule_utils as su
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_len, fifo_prompt_windows
    B, S, sl = eng.embed.B, eng.slots, eng.slot_len
    rn, rp, sn, sp = su.fifo_plan(sched, S)
    dpm = eng.solver == "dpmpp_2m"
    rl, last = su.fifo_plan_last(sched, S) if dpm else (None, None)
    n = B * S
    L_ = eng.latent_shape[2]
    Lp = fifo_prompt_len(eng, canvas_p)
    z = Fn.canvas_noise(seed, torch.full((B,), int(sched[0])), eng.latent_shape, L_)
    eng.set_prompt(fifo_prompt_windows(canvas_p, 0, B, S, hop, Lp))
    for r in range(n - 1):
        z = eng.step_slots(z, rn[r], rp[r], t_last=rl[r] if dpm else None)
    done = []
    for m in range(K):
        eng.set_prompt(fifo_prompt_windows(canvas_p, m, B, S, hop, Lp))
        z = eng.step_slots(z, sn, sp, t_last=last)
        one_slot = (1, z.shape[1], sl) + tuple(z.shape[3:])
        tail = Fn.canvas_noise(seed, torch.tensor([int(sched[0])]), one_slot, sl, window_offset=n + m)[0]
        z, popped = SR.shift(z, tail, sl)
        if dpm:
            eng.x0_hist.copy_(SR.shift(eng.x0_hist, torch.zeros_like(tail), sl)[0])
        done.append(popped)
    return torch.cat(done, 1)


@pytest.mark.parametrize("target", ["video", "audio"])
def test_fifo_denoise_dpmpp_2m_equals_the_loop_of_its_parts(dev, model, target):
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop = _setup(dev, model[1], target, "dpmpp_2m")
    gen0 = eng._generation
    out3 = A.fifo_denoise(eng, canvas_p, hop, SCHED4, 3, SEED)
    assert eng._generation > gen0 and "x0_hist" in eng._stale_reason          # the shift moved an address a captured graph holds
    ref3 = _loop(eng, canvas_p, hop, SCHED4, 3, SEED)
    sl = eng.slot_len
    assert out3.shape == (8, 3 * sl) + tuple(eng.latent_shape[3:]) and torch.isfinite(out3).all()
    assert torch.equal(out3, ref3), float((out3 - ref3).abs().max())
    # a longer clip leaves the slots already out unchanged
    out5, out2 = A.fifo_denoise(eng, canvas_p, hop, SCHED4, 5, SEED), A.fifo_denoise(eng, canvas_p, hop, SCHED4, 2, SEED)
    assert torch.equal(out5[:, :2 * sl], out2) and torch.equal(out5[:, :3 * sl], out3)
    assert float(out3.std()) > 0
    # the second-order steps are live: the ddim engine gives another clip from the same seed
    ddim, _, _ = _setup(dev, model[1], target, "ddim")
    assert not torch.equal(A.fifo_denoise(ddim, canvas_p, hop, SCHED4, 3, SEED), out3)


@pytest.mark.parametrize("target", ["video", "audio"])
def test_fifo_denoise_ddim_still_equals_its_loop(dev, model, target):
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop = _setup(dev, model[1], target, "ddim")
    out3 = A.fifo_denoise(eng, canvas_p, hop, SCHED4, 3, SEED)
    assert torch.isfinite(out3).all() and torch.equal(out3, _loop(eng, canvas_p, hop, SCHED4, 3, SEED))
    assert eng.x0_hist is None


def test_engine_fifo_shift(dev, model):
    from multimodal_diffusion_amd import functional as Fn
    z = torch.randn(2, 8, 4, 16, 16, device=dev)
    ddim = engine(model[1], "video", tuple(z.shape), 10, guidance=GS)
    with pytest.raises(ValueError, match="seed"):
        ddim.fifo_shift(z, 4, 999)
    gen = ddim._generation
    a, b = ddim.fifo_shift(z, 4, 999, seed=SEED), Fn.fifo_shift(z, 4, SEED, 999, 2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and ddim._generation == gen
    eng = engine(model[1], "video", tuple(z.shape), 10, guidance=GS, solver="dpmpp_2m", noise_seed=SEED)
    h0 = torch.randn_like(z)
    eng.x0_hist.copy_(h0)
    first, gen = eng.x0_hist, eng._generation
    zo, popped = eng.fifo_shift(z, 4, 999)
    assert torch.equal(zo, b[0]) and torch.equal(popped, b[1])
    assert torch.equal(eng.x0_hist, Fn.fifo_shift(z, 4, SEED, 999, 2, hist=h0)[2])
    assert eng.x0_hist is not first and eng._generation == gen + 1
    eng.fifo_shift(zo, 5, 999)
    assert eng.x0_hist is first                                               # two engine-owned buffers, used in turn
