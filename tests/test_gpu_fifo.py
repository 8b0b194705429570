"""FIFO diagonal denoising on the GPU: the queue shift kernel against its torch restatement, and the driver against a loop written
here from its parts — everything bit for bit."""
import pytest
import torch

import _slot_ref as SR
from _kit import audio_case, dev, engine, model, video_case  # noqa: F401  (dev, model are fixtures)

pytestmark = pytest.mark.gpu

GS = 3.5
SEED = 0x5EED0F1F0


# ------------------------------------------------------------------------------------------------- fifo_shift
@pytest.mark.parametrize("shape,slot_len", [((2, 8, 4, 16, 16), 2), ((2, 8, 40), 4), ((3, 8, 4, 16, 16), 1)])
def test_fifo_shift_equals_roll_and_canvas_noise(dev, shape, slot_len):
    from multimodal_diffusion_amd import functional as Fn
    z = torch.randn(shape, generator=torch.Generator().manual_seed(len(shape))).to(dev)
    c, t = 11, 999
    one_slot = (1, shape[1], slot_len) + tuple(shape[3:])
    tail = Fn.canvas_noise(SEED, torch.tensor([t]), one_slot, slot_len, window_offset=c)[0]
    ref, ref_popped = SR.shift(z, tail, slot_len)
    out, popped = Fn.fifo_shift(z, c, SEED, t, slot_len)
    assert torch.equal(out, ref) and torch.equal(popped, ref_popped)
    assert popped.shape == one_slot[1:] and torch.isfinite(out).all()
    # the tail is clip slot c of a queue initialised as the driver does: the same normals whatever the clip length
    B, L_ = shape[0], shape[2]
    S = L_ // slot_len
    init = Fn.canvas_noise(SEED, torch.full((c // S + 1,), t), (c // S + 1,) + tuple(shape[1:]), L_)
    assert torch.equal(init[c // S][:, (c % S) * slot_len:(c % S + 1) * slot_len], tail)
    # a misaligned view takes the one-element lanes: same bits
    if len(shape) == 5:
        buf = torch.empty(z.numel() + 1, device=dev)
        zu = buf[1:].view(shape).copy_(z)
        assert zu.data_ptr() % 16 != 0
        from multimodal_diffusion_amd import _lib as L
        import ctypes as C
        o2, p2 = torch.empty_like(z), torch.empty_like(popped)
        L.check(L.lib().avd_fifo_shift_f32(C.byref(Fn.noise_key(SEED, 0)), t, c, zu.data_ptr(), o2.data_ptr(), p2.data_ptr(), B, shape[1], S,
                                           slot_len, shape[3] * shape[4], L.stream_ptr(dev)))
        assert torch.equal(o2, out) and torch.equal(p2, popped)


def test_fifo_shift_refusals(dev):
    from multimodal_diffusion_amd import functional as Fn
    z = torch.zeros(2, 8, 40, device=dev)
    with pytest.raises(ValueError, match="divides"):
        Fn.fifo_shift(z, 0, SEED, 999, 3)
    with pytest.raises(ValueError, match="2\\*\\*32"):
        Fn.fifo_shift(z, 2 ** 30, SEED, 999, 4)
    with pytest.raises(ValueError):
        Fn.fifo_shift(z, -1, SEED, 999, 4)


# ------------------------------------------------------------------------------------------------- fifo_denoise
def _setup(dev, mods, target):
    """(engine, prompt canvas, prompt_hop) of a queue of n = 4 slots (B = 2, S = 2).  Video [2, 8, 4, 16, 16], tube 2 x 4 x 4, under
    an audio prompt of 10 chunks = 40 frames per sample, 20 per target slot; audio [2, 8, 8], chunk 4 / 4, under a video prompt of 8
    tubes = 4 frames per sample, 2 per target slot."""
    g = torch.Generator().manual_seed(17)
    if target == "video":
        eng = engine(mods, "video", (2, 8, 4, 16, 16), 10, guidance=GS)
        return eng, torch.randn(8, 150, generator=g).to(dev), 20
    eng = engine(mods, "audio", (2, 8, 8), 8, guidance=GS)
    return eng, torch.randn(8, 14, 8, 8, generator=g).to(dev), 2


def _loop(eng, canvas_p, hop, sched, K, seed):
    """fifo_denoise restated from its parts: fifo_plan's tables, step_slots, the torch shift, set_prompt"""
    from multimodal_diffusion_amd import functional as Fn, schedule_utils as su
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_len, fifo_prompt_windows
    B, S, sl = eng.embed.B, eng.slots, eng.slot_len
    rn, rp, sn, sp = su.fifo_plan(sched, S)
    n = B * S
    L_ = eng.latent_shape[2]
    Lp = fifo_prompt_len(eng, canvas_p)
    z = Fn.canvas_noise(seed, torch.full((B,), int(sched[0])), eng.latent_shape, L_)
    eng.set_prompt(fifo_prompt_windows(canvas_p, 0, B, S, hop, Lp))
    for r in range(n - 1):
        z = eng.step_slots(z, rn[r], rp[r])
    done = []
    for m in range(K):
        eng.set_prompt(fifo_prompt_windows(canvas_p, m, B, S, hop, Lp))
        z = eng.step_slots(z, sn, sp)
        one_slot = (1, z.shape[1], sl) + tuple(z.shape[3:])
        tail = Fn.canvas_noise(seed, torch.tensor([int(sched[0])]), one_slot, sl, window_offset=n + m)[0]
        z, popped = SR.shift(z, tail, sl)
        done.append(popped)
    return torch.cat(done, 1)


@pytest.mark.parametrize("target", ["video", "audio"])
def test_fifo_denoise_equals_the_loop_of_its_parts(dev, model, target):
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop = _setup(dev, model[1], target)
    sched = torch.tensor([999, 749, 499, 249, -1])
    out3 = A.fifo_denoise(eng, canvas_p, hop, sched, 3, SEED)
    ref3 = _loop(eng, canvas_p, hop, sched, 3, SEED)
    sl = eng.slot_len
    assert out3.shape == (8, 3 * sl) + tuple(eng.latent_shape[3:]) and torch.isfinite(out3).all()
    assert torch.equal(out3, ref3), float((out3 - ref3).abs().max())
    # a longer clip leaves the slots already out unchanged
    out4, out2 = A.fifo_denoise(eng, canvas_p, hop, sched, 4, SEED), A.fifo_denoise(eng, canvas_p, hop, sched, 2, SEED)
    assert torch.equal(out4[:, :2 * sl], out2) and torch.equal(out4[:, :3 * sl], out3)
    # and another seed is another clip
    other = A.fifo_denoise(eng, canvas_p, hop, sched, 2, SEED + 1)
    assert not torch.equal(other, out2)
    # finished slots are clean latents, not the noise they started from: every slot took all n steps
    assert float(out3.std()) > 0


def test_fifo_denoise_refuses_a_mismatched_queue(dev, model):
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop = _setup(dev, model[1], "video")
    with pytest.raises(ValueError, match="queue"):
        A.fifo_denoise(eng, canvas_p, hop, torch.tensor([999, 499, -1]), 2, SEED)             # n = 2, the queue holds 4
    with pytest.raises(ValueError, match="n_slots"):
        A.fifo_denoise(eng, canvas_p, hop, torch.tensor([999, 749, 499, 249, -1]), 0, SEED)
    with pytest.raises(ValueError, match="audio prompt canvas"):
        A.fifo_denoise(eng, torch.zeros(8, 14, 8, 8, device=dev), hop, torch.tensor([999, 749, 499, 249, -1]), 1, SEED)


@pytest.mark.parametrize("target", ["video", "audio"])
def test_every_driver_refuses_a_bad_queue_before_anything_runs(dev, model, target, monkeypatch):
    """the argument and geometry faults every driver checks — eager, graph=True, lookahead=1 and the clip batch of K = 2 — are
    ValueErrors raised before the first set_prompt or step_slots, and leave no control or guide on the engine"""
    import re
    import multimodal_diffusion_amd as A
    sched = torch.tensor([999, 749, 499, 249, -1])
    eng2, canvas_p, hop = _setup(dev, model[1], target)                                   # B = 2: n = B * S = 4
    eng4 = engine(model[1], target, (4,) + tuple(eng2.latent_shape[1:]), eng2.embed.Np, guidance=GS)      # lookahead 1: n = B * (S - 1);
    sl = eng2.slot_len                                                                    # clips: n = (B / 2) * S
    drivers = {"eager": (eng2, lambda e, hop, sched, K, **kw: A.fifo_denoise(e, canvas_p, hop, sched, K, SEED, graph=False, **kw)),
               "graph": (eng2, lambda e, hop, sched, K, **kw: A.fifo_denoise(e, canvas_p, hop, sched, K, SEED, graph=True, **kw)),
               "lookahead": (eng4, lambda e, hop, sched, K, **kw: A.fifo_denoise(e, canvas_p, hop, sched, K, SEED, lookahead=1, **kw)),
               "clips": (eng4, lambda e, hop, sched, K, **kw: A.fifo_denoise_clips(e, [canvas_p, canvas_p + 1.0], hop, sched, K,
                                                                                   [SEED, SEED + 1], **kw))}
    faults = [(dict(K=0), "n_slots"), (dict(K=True), "n_slots"), (dict(hop=0), "prompt_hop"), (dict(prompt_den=2), "prompt_interp"),
              (dict(sched=torch.tensor([999, 749, 499, -1])), None), (dict(K=2 ** 32 // sl), re.escape("2**32 canvas positions"))]
    calls = []
    for eng in (eng2, eng4):
        assert eng.slots == 2
        for name in ("step_slots", "set_prompt"):
            def spy(*a, _name=name, _real=getattr(eng, name), **kw):
                calls.append(_name)
                return _real(*a, **kw)
            monkeypatch.setattr(eng, name, spy)
    for name, (eng, run) in drivers.items():
        for fault, match in faults:
            for ctl in (dict(), dict(guidance_by_level=3.0)):
                args = dict(dict(hop=hop, sched=sched, K=2), **fault)
                with pytest.raises(ValueError, match=match):
                    run(eng, args.pop("hop"), args.pop("sched"), args.pop("K"), **args, **ctl)
                assert calls == [], (name, fault)
                assert eng._scfg is None and eng._clip is None and eng._clips is None, (name, fault)
    assert not torch.cuda.is_current_stream_capturing()
