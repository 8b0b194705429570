"""FIFO denoising under a clip-keyed latent guide on the MI355X (include/avdiff_hip.h, "clip-keyed latent guide"):
``fifo_denoise(init_canvas=...)`` against a loop written here from the unguided ``step_slots``, ``clip_guide_slots`` and ``fifo_shift``;
held slots; the zero mask; the SDEdit start; a clip longer than its canvas.  Reduced model, queues of 2 x 2 and 1 x 4 slots, 4 steps."""
import numpy as np
import pytest
import torch

import _clip_guide_ref as CG
from _kit import ABAR, dev, engine, model  # noqa: F401  (dev, model are fixtures)

pytestmark = pytest.mark.gpu

GS = 3.5
SEED = 0x5EED0F1F0          # the queue's start and entering noise
ESEED = 0x51075EED          # the engines' noise_seed: the step noise
GSEED = 0x4B4E0BADCAFE      # the guide's known noise
SCHED4 = torch.tensor([999, 749, 499, 249, -1])
K = 6                       # finished slots


def tol(ref):
    """the project's gate: 1e-4 max(1, max |ref|)"""
    return 1e-4 * max(1.0, float(np.abs(ref).max()))


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _setup(dev, mods, target, solver, eta, queue=(2, 2)):
    """(engine, prompt canvas, prompt hop) of a queue of B x S slots on either target"""
    B, S = queue
    g = torch.Generator().manual_seed(17)
    kw = dict(guidance=GS, solver=solver, eta=eta, **({"noise_seed": ESEED} if eta else {}))
    if target == "video":
        return engine(mods, "video", (B, 8, 2 * S, 16, 16), 10, **kw), torch.randn(8, 150, generator=g).to(dev), 20
    return engine(mods, "audio", (B, 8, 4 * S), 8, **kw), torch.randn(8, 14, 8, 8, generator=g).to(dev), 2


def _clip_canvases(dev, eng, P, seed=0):
    """(known, mask) canvases of P positions: ones on clip slots [2, 5), zeros before, fractional values after"""
    from multimodal_diffusion_amd.sampler import canvas_frame_mask
    g = torch.Generator().manual_seed(seed + P)
    cs = (eng.latent_shape[1], P) + tuple(eng.latent_shape[3:])
    sl = eng.slot_len
    mask = canvas_frame_mask(cs, 2 * sl, min(5 * sl, P))
    if P > 5 * sl:
        mask[:, 5 * sl:] = torch.rand(mask[:, 5 * sl:].shape, generator=g) * 0.5
    return torch.randn(cs, generator=g).to(dev), mask


def _loop(eng, canvas_p, hop, sched, n_slots, seed, known, mask, everywhere=False):
    """the guided queue from its parts: the unguided step_slots, then clip_guide_slots at each slot's t_prev (held slots left); the
    start and each entering tail slot through clip_guide_slots at s_0"""
    from multimodal_diffusion_amd import functional as Fn, schedule_utils as su
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_len, fifo_prompt_windows
    B, S, sl = eng.embed.B, eng.slots, eng.slot_len
    rn, rp, sn, sp = su.fifo_plan(sched, S)
    dpm = eng.solver == "dpmpp_2m"
    rl, last = su.fifo_plan_last(sched, S) if dpm else (None, None)
    n, s0 = B * S, int(sched[0])
    Lp = fifo_prompt_len(eng, canvas_p)
    m_dev = None if mask is None else mask.to(eng.device)
    gd = lambda z, tau, first, every=False: Fn.clip_guide_slots(known, tau, ABAR, z, m_dev, slot_len=sl, seed=GSEED, first=first,
                                                                 everywhere=every)
    at_prev = lambda tn, tp: torch.where(tn == tp, torch.full_like(tp, Fn.SLOT_LEAVE), tp)
    z = Fn.canvas_noise(seed, torch.full((B,), s0), eng.latent_shape, eng.latent_shape[2])
    z = gd(z, torch.full((B, S), s0), 0, everywhere)
    eng.set_prompt(fifo_prompt_windows(canvas_p, 0, B, S, hop, Lp))
    for r in range(n - 1):
        z = gd(eng.step_slots(z, rn[r], rp[r], t_last=rl[r] if dpm else None, clip_first=0), at_prev(rn[r], rp[r]), 0)
    tail = torch.full((B, S), Fn.SLOT_LEAVE)
    tail[B - 1, S - 1] = s0
    done = []
    for m in range(n_slots):
        eng.set_prompt(fifo_prompt_windows(canvas_p, m, B, S, hop, Lp))
        z = gd(eng.step_slots(z, sn, sp, t_last=last, clip_first=m), at_prev(sn, sp), m)
        z, popped = eng.fifo_shift(z, n + m, s0, seed=seed)
        z = gd(z, tail, m + 1, everywhere)
        done.append(popped)
    return torch.cat(done, 1)


CASES = [(t, s, e, (2, 2)) for t in ("video", "audio") for s, e in (("ddim", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0), ("dpmpp_2m", 0.5))]
CASES += [("video", "ddim", 0.5, (1, 4)), ("audio", "dpmpp_2m", 0.0, (1, 4))]


@pytest.mark.parametrize("target,solver,eta,queue", CASES)
def test_guided_fifo_denoise_equals_the_loop_of_its_parts(dev, model, target, solver, eta, queue):
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop = _setup(dev, model[1], target, solver, eta, queue)
    sl = eng.slot_len
    known, mask = _clip_canvases(dev, eng, K * sl)
    out = A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, SEED, init_canvas=known, mask=mask, guide_seed=GSEED)
    assert eng._clip is None                             # the engine's clip guide is set for the call only
    ref = _loop(eng, canvas_p, hop, SCHED4, K, SEED, known, mask)
    assert out.shape == tuple(known.shape) and torch.isfinite(out).all() and float(out.std()) > 0
    assert torch.equal(out, ref), float((out - ref).abs().max())
    # held slots: the canvas bit for bit where the mask is 1
    held = (mask == 1).to(dev)
    assert held.any() and torch.equal(out[held], known[held])
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, SEED, init_canvas=known, mask=mask, guide_seed=GSEED), out)


@pytest.mark.parametrize("solver,eta", [("ddim", 0.5), ("dpmpp_2m", 0.0)])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_held_slots_zero_mask_and_a_clip_longer_than_the_canvas(dev, model, target, solver, eta):
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd.sampler import canvas_frame_mask
    eng, canvas_p, hop = _setup(dev, model[1], target, solver, eta)
    sl = eng.slot_len
    plain = A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, SEED)
    cs = (8, K * sl) + tuple(eng.latent_shape[3:])
    known = torch.randn(cs, generator=torch.Generator().manual_seed(3)).to(dev)
    # a zero mask: today's fifo_denoise, bit for bit (which also shows the default path unchanged)
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, SEED, init_canvas=known, mask=torch.zeros(cs), guide_seed=GSEED), plain)
    # the mask 1 on clip slots [2, 5): known there bit for bit, and another clip than the unguided one elsewhere
    mask = canvas_frame_mask(cs, 2 * sl, 5 * sl)
    out = A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, SEED, init_canvas=known, mask=mask, guide_seed=GSEED)
    assert torch.isfinite(out).all()
    assert torch.equal(out[:, 2 * sl:5 * sl], known[:, 2 * sl:5 * sl])
    free = torch.cat([out[:, :2 * sl], out[:, 5 * sl:]], 1), torch.cat([plain[:, :2 * sl], plain[:, 5 * sl:]], 1)
    assert not torch.equal(free[0], free[1])
    # clip slot 5 shared its samples with held slots on its way up the queue: another latent, element for element.  Clip slot 0 never
    # shares a sample with a guided slot (it leaves before slot 2 reaches sample 0): the unguided run's bits
    assert float((out[:, 5 * sl:] != plain[:, 5 * sl:]).float().mean()) > 0.99
    assert torch.equal(out[:, :sl], plain[:, :sl])
    assert not torch.equal(out[:, 2 * sl:5 * sl], plain[:, 2 * sl:5 * sl])
    # a canvas of 3 slots under a clip of K: known on the canvas, the slots past P unguided and finite
    short = A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, SEED, init_canvas=known[:, :3 * sl].contiguous(), guide_seed=GSEED)
    assert short.shape == plain.shape and torch.isfinite(short).all()
    assert torch.equal(short[:, :3 * sl], known[:, :3 * sl])
    past = short[:, 3 * sl:]
    assert float(past.std()) > 0 and not torch.equal(past, known[:, 3 * sl:]) and not torch.equal(past, plain[:, 3 * sl:])
    # graph replay and lookahead refuse the guide before anything is allocated
    with pytest.raises(ValueError, match="graph=True is refused"):
        A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, SEED, graph=True, init_canvas=known)
    with pytest.raises(ValueError, match="lookahead > 0 is refused"):
        A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, SEED, lookahead=1, init_canvas=known)
    eng.set_clip_guide(known)
    with pytest.raises(ValueError, match="fifo_open takes no clip guide"):
        A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, SEED, graph=True)
    eng.clear_clip_guide()


@pytest.mark.parametrize("target", ["video", "audio"])
def test_guide_start_init_puts_the_queue_on_the_forward_path(dev, model, target, monkeypatch):
    """SDEdit: the truncated schedule sets the queue (2 steps: B x S = 1 x 2), and after the first clip_guide_slots call every in-canvas
    slot holds q(s_0) of the canvas, the slot past it its start noise"""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import functional as Fn, schedule_utils as su
    sched = su.truncate_schedule(SCHED4, 0.5)
    assert sched.tolist() == [499, 249, -1]
    eng, canvas_p, hop = _setup(dev, model[1], target, "ddim", 0.0, queue=(1, 2))
    sl = eng.slot_len
    P = sl + sl // 2                                     # the canvas ends inside queue slot 1
    g = torch.Generator().manual_seed(P)
    cs = (8, P) + tuple(eng.latent_shape[3:])
    known, mask = torch.randn(cs, generator=g).to(dev), torch.rand(cs, generator=g)
    calls, real = [], Fn.clip_guide_slots

    def spy(*a, **kw):
        out = real(*a, **kw)
        calls.append((kw.get("first"), kw.get("everywhere"), out.clone()))
        return out

    monkeypatch.setattr(Fn, "clip_guide_slots", spy)
    out = A.fifo_denoise(eng, canvas_p, hop, sched, 3, SEED, init_canvas=known, mask=mask, guide_seed=GSEED, guide_start="init")
    monkeypatch.setattr(Fn, "clip_guide_slots", real)
    assert torch.isfinite(out).all()
    assert [(f, e) for f, e, _ in calls] == [(0, True), (1, True), (2, True), (3, True)]      # the start, then one tail pass per shift
    z0 = Fn.canvas_noise(SEED, torch.full((1,), 499), eng.latent_shape, eng.latent_shape[2])
    ref = CG.clip_guide_slots(_np(known), None, np.full((1, 2), 499), ABAR.numpy(), _np(z0), GSEED, sl, everywhere=True)
    got = calls[0][2]
    err = float(np.abs(_np(got) - ref).max())
    print(f"guide_start='init' ({target}): the start against the mirror's q(s_0), max err {err:.3e} (gate {tol(ref):.3e})")
    assert err < tol(ref)
    assert torch.equal(got[:, :, P:], z0[:, :, P:]) and float((got[:, :, :P] != z0[:, :, :P]).float().mean()) > 0.99
    # "noise" starts the unmasked positions from the start noise: another clip
    noise = A.fifo_denoise(eng, canvas_p, hop, sched, 3, SEED, init_canvas=known, mask=mask, guide_seed=GSEED)
    assert not torch.equal(noise, out)
    ref_loop = _loop(eng, canvas_p, hop, sched, 3, SEED, known, mask, everywhere=True)
    assert torch.equal(out, ref_loop), float((out - ref_loop).abs().max())
