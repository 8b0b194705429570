"""FIFO lookahead denoising on the GPU: the lookahead kernel against the torch map of the logical queue, its ctx = 0 case against the
plain queue shift, and the driver (noise and supplied context, both solvers) against a loop written from its parts — bit for bit."""
import ctypes as C

import pytest
import torch

import _lookahead_ref as LR
from _kit import dev, engine, model  # noqa: F401  (dev, model are fixtures)

pytestmark = pytest.mark.gpu

GS = 3.5
SEED = 0x5EED0F1F0
T0 = 999


def _tail(Fn, shape, slot_len, c):
    one_slot = (1, shape[1], slot_len) + tuple(shape[3:])
    return Fn.canvas_noise(SEED, torch.tensor([T0]), one_slot, slot_len, window_offset=c)[0]


# ------------------------------------------------------------------------------------------------- the kernel
# B = 3: the smallest batch with a window whose slots are duplicated on both sides; ctx = 3 (h = 1): one slot lives in every window;
# the audio latent (inner = 1) takes the one-element lanes.  The last four are the smallest queues with h = 1, where the owner's window
# is the division's quotient alone: one window (no duplicates, every stepping position is the tail at shift 1), two, and inner = 3 (the
# one-element lanes on a video shape)
@pytest.mark.parametrize("shape,slot_len,ctx", [((3, 8, 8, 16, 16), 2, 1), ((3, 8, 8, 16, 16), 2, 2), ((3, 8, 8, 16, 16), 2, 3),
                                                ((3, 8, 16), 4, 2), ((2, 8, 4, 16, 16), 2, 1), ((1, 1, 2, 2, 2), 1, 1),
                                                ((2, 1, 2, 2, 2), 1, 1), ((2, 1, 3, 1, 3), 1, 2), ((2, 2, 8), 4, 1)])
def test_lookahead_equals_the_torch_map(dev, shape, slot_len, ctx):
    from multimodal_diffusion_amd import _lib as L, functional as Fn
    g = torch.Generator().manual_seed(len(shape) + ctx)
    z, hist = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)      # no copy equals its owner yet
    assert ctx == 0 or shape[0] == 1 or not LR.coherent(z, ctx, slot_len)      # one window holds no duplicate
    c = 11
    tail = _tail(Fn, shape, slot_len, c)
    B, S = shape[0], shape[2] // slot_len
    inner = shape[3] * shape[4] if len(shape) == 5 else 1
    for shift in (0, 1):
        kw = dict(c=c, seed=SEED, t=T0) if shift else {}
        ref, ref_popped = LR.lookahead(z, ctx, shift, slot_len, tail)
        ref_hist = LR.lookahead_hist(hist, ctx, shift, slot_len)
        out, popped = Fn.fifo_lookahead(z, ctx, shift, slot_len, **kw)
        out_h, popped_h, hist_out = Fn.fifo_lookahead(z, ctx, shift, slot_len, hist=hist, **kw)
        assert torch.equal(out, ref) and torch.equal(out_h, ref) and torch.isfinite(out).all()
        assert torch.equal(hist_out, ref_hist)
        if shift:
            assert torch.equal(popped, ref_popped) and torch.equal(popped_h, ref_popped)
            assert popped.shape == (shape[1], slot_len) + tuple(shape[3:])
            assert torch.equal(LR.slot(out, B - 1, S - 1, slot_len), tail)          # the entering tail: clip slot c's normals
        else:
            assert popped is None and popped_h is None
        assert LR.coherent(out, ctx, slot_len)                                      # every duplicate equals its owner
        assert (hist_out[:, :, :ctx * slot_len] == 0).all()                         # zeros on the context positions ...
        if shift:
            assert (LR.slot(hist_out, B - 1, S - 1, slot_len) == 0).all()           # ... and in the tail
        if B * (S - ctx) > shift:                                                   # a stepping position whose source is not the tail
            assert (hist_out[:, :, ctx * slot_len:] != 0).any()
        if len(shape) == 5:      # misaligned views take the one-element lanes: same bits
            zu, hu = (torch.empty(x.numel() + 1, device=dev)[1:].view(shape).copy_(x) for x in (z, hist))      # one float past an allocation
            assert zu.data_ptr() % 16 != 0 and hu.data_ptr() % 16 != 0
            o2, h2 = torch.empty_like(z), torch.empty_like(z)
            p2 = torch.empty_like(popped) if shift else None
            key = C.byref(Fn.noise_key(SEED, 0)) if shift else None
            dims = (B, shape[1], S, ctx, slot_len, inner, L.stream_ptr(dev))
            L.check(L.lib().avd_fifo_lookahead_f32(key, T0 * shift, c * shift, shift, zu.data_ptr(), o2.data_ptr(), L.ptr(p2), *dims))
            assert torch.equal(o2, ref) and (not shift or torch.equal(p2, ref_popped))
            o2.zero_()
            L.check(L.lib().avd_fifo_lookahead_hist_f32(key, T0 * shift, c * shift, shift, zu.data_ptr(), o2.data_ptr(), L.ptr(p2),
                                                        hu.data_ptr(), h2.data_ptr(), *dims))
            assert torch.equal(o2, ref) and torch.equal(h2, ref_hist)


# the last two are queues of one slot: every output lane is the tail and the only slot is the head
@pytest.mark.parametrize("shape,slot_len", [((2, 8, 4, 16, 16), 2), ((2, 8, 40), 4), ((3, 8, 4, 16, 16), 1), ((1, 1, 1, 2, 2), 1),
                                            ((1, 2, 4), 4)])
def test_ctx_0_is_the_plain_shift(dev, shape, slot_len):
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(5)
    z, hist = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
    ref, ref_popped = Fn.fifo_shift(z, 11, SEED, T0, slot_len)
    out, popped = Fn.fifo_lookahead(z, 0, 1, slot_len, c=11, seed=SEED, t=T0)
    assert torch.equal(out, ref) and torch.equal(popped, ref_popped)
    ref, ref_popped, ref_hist = Fn.fifo_shift(z, 11, SEED, T0, slot_len, hist=hist)
    out, popped, hist_out = Fn.fifo_lookahead(z, 0, 1, slot_len, c=11, seed=SEED, t=T0, hist=hist)
    assert torch.equal(out, ref) and torch.equal(popped, ref_popped) and torch.equal(hist_out, ref_hist)
    out0, none = Fn.fifo_lookahead(z, 0, 0, slot_len)                     # no duplicates at ctx = 0: the refresh is a copy
    assert none is None and torch.equal(out0, z)


@pytest.mark.parametrize("shape,slot_len", [((3, 2, 4, 2, 2), 1), ((2, 2, 8), 4)])
def test_every_entry_is_the_one_map(dev, shape, slot_len):
    """Every queue-move entry is one slot map: at ctx = 0, shift = 1 and one queue the shift, the lookahead, the cursor shift (the
    cursor holding m, c0 = c - m) and the clip batch give the torch map's bits, their histories fifo_carry's; at ctx > 0 fifo_carry is
    the lookahead's history output at either shift.  Once more on a view misaligned by one float (the one-element lanes)."""
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(23)
    z, hist = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
    S, c, m, n_clip = shape[2] // slot_len, 11, 2, 4
    ref, ref_popped = LR.lookahead(z, 0, 1, slot_len, _tail(Fn, shape, slot_len, c))
    ref_hist = Fn.fifo_carry(hist, S, slot_len)
    assert torch.equal(ref_hist, LR.lookahead_hist(hist, 0, 1, slot_len))
    canvas = (shape[1], n_clip * slot_len) + tuple(shape[3:])
    head = (slice(None), slice(m * slot_len, (m + 1) * slot_len))

    def entries(z_, h_):
        """(z_out, head, hist_out or None) of every entry"""
        kw = {} if h_ is None else dict(hist=h_)
        yield Fn.fifo_shift(z_, c, SEED, T0, slot_len, **kw) + (() if kw else (None,))
        yield Fn.fifo_lookahead(z_, 0, 1, slot_len, c=c, seed=SEED, t=T0, **kw) + (() if kw else (None,))
        clip = torch.full(canvas, 7.0, device=dev)
        res = Fn.fifo_shift_cursor(z_, c - m, torch.tensor([m], dtype=torch.int32, device=dev), clip, SEED, T0, slot_len, **kw)
        yield (res[0], clip[head], res[1]) if kw else (res, clip[head], None)
        clips = torch.full((1,) + canvas, 7.0, device=dev)
        res = Fn.fifo_shift_clips(z_, 1, c, [SEED], T0, slot_len, clips, m, **kw)
        yield (res[0], clips[0][head], res[1]) if kw else (res, clips[0][head], None)

    views = [(z, hist)]
    if len(shape) == 5:
        zu, hu = (torch.empty(x.numel() + 1, device=dev)[1:].view(shape).copy_(x) for x in (z, hist))
        assert zu.data_ptr() % 16 != 0 and hu.data_ptr() % 16 != 0
        views.append((zu, hu))
    for z_, h_ in views:
        for with_hist in (False, True):
            got = list(entries(z_, h_ if with_hist else None))
            assert len(got) == 4
            for out, popped, hist_out in got:
                assert torch.equal(out, ref) and torch.equal(popped, ref_popped)
                assert (hist_out is None) if not with_hist else torch.equal(hist_out, ref_hist)
        for ctx in sorted({1, S - 1}):
            for shift in (0, 1):
                kw = dict(c=c, seed=SEED, t=T0) if shift else {}
                want = LR.lookahead_hist(hist, ctx, shift, slot_len)
                assert torch.equal(Fn.fifo_carry(h_, S, slot_len, ctx=ctx, shift=shift), want)
                assert torch.equal(Fn.fifo_lookahead(z_, ctx, shift, slot_len, hist=h_, **kw)[2], want)


def test_functional_refusals(dev):
    from multimodal_diffusion_amd import functional as Fn
    z = torch.zeros(2, 8, 16, device=dev)
    with pytest.raises(ValueError, match="ctx"):
        Fn.fifo_lookahead(z, 4, 0, 4)
    with pytest.raises(ValueError, match="shift"):
        Fn.fifo_lookahead(z, 2, 2, 4)
    with pytest.raises(ValueError, match="shift=0"):
        Fn.fifo_lookahead(z, 2, 0, 4, c=3, seed=SEED, t=T0)
    with pytest.raises(ValueError, match="shift=1"):
        Fn.fifo_lookahead(z, 2, 1, 4, seed=SEED, t=T0)
    with pytest.raises(ValueError, match="seed"):
        Fn.fifo_lookahead(z, 2, 1, 4, c=3, t=T0)
    with pytest.raises(ValueError, match="divides"):
        Fn.fifo_lookahead(z, 2, 0, 3)


# ------------------------------------------------------------------------------------------------- the driver
def _setup(dev, mods, target, solver="ddim"):
    """(engine, prompt canvas, prompt_hop, schedule) at S = 4, ctx = 2.  Video [3, 8, 8, 16, 16], tube 2 x 4 x 4: B = 3 windows, n = 6,
    under an audio prompt of 10 chunks = 40 frames per sample, 10 per target slot; audio [2, 8, 16], chunk 4 / 4: B = 2, n = 4, under a
    video prompt of 8 tubes = 4 frames per sample, 1 per target slot."""
    g = torch.Generator().manual_seed(17)
    if target == "video":
        eng = engine(mods, "video", (3, 8, 8, 16, 16), 10, guidance=GS, solver=solver)
        return eng, torch.randn(8, 90, generator=g).to(dev), 10, torch.tensor([999, 832, 665, 499, 332, 165, -1])
    eng = engine(mods, "audio", (2, 8, 16), 8, guidance=GS, solver=solver)
    return eng, torch.randn(8, 9, 8, 8, generator=g).to(dev), 1, torch.tensor([999, 749, 499, 249, -1])


def _loop(eng, canvas_p, hop, sched, K, ctx, seed, context=None):
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_len
    shape = eng.latent_shape

    def noise(p0, n_pos):      # the seeded normals at s_0 of canvas positions p0 .. p0 + n_pos - 1: one window at hop 1
        return Fn.canvas_noise(seed, torch.tensor([int(sched[0])]), (1, shape[1], n_pos) + tuple(shape[3:]), 1, window_offset=p0)[0]

    return LR.loop(eng, canvas_p, hop, fifo_prompt_len(eng, canvas_p), sched.tolist(), K, ctx, noise, context)


def _driver_checks(eng, canvas_p, hop, sched, K, context=None):
    """the loop-of-parts equality at K slots and what goes with it: prefix stability, the seed, finiteness"""
    import multimodal_diffusion_amd as A
    sl = eng.slot_len
    kw = dict(lookahead=2, context=context)
    out = A.fifo_denoise(eng, canvas_p, hop, sched, K, SEED, **kw)
    ref = _loop(eng, canvas_p, hop, sched, K, 2, SEED, context)
    assert out.shape == (8, K * sl) + tuple(eng.latent_shape[3:]) and torch.isfinite(out).all() and float(out.std()) > 0
    assert torch.equal(out, ref), float((out - ref).abs().max())
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, sched, K, SEED, graph=None, **kw), out)      # None runs eagerly
    shorter = A.fifo_denoise(eng, canvas_p, hop, sched, 2, SEED, **kw)
    assert torch.equal(out[:, :2 * sl], shorter)                          # a longer clip leaves the slots already out unchanged
    assert not torch.equal(A.fifo_denoise(eng, canvas_p, hop, sched, 2, SEED + 1, **kw), shorter)
    return out


def test_lookahead_denoise_equals_the_loop_of_its_parts_video(dev, model):
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop, sched = _setup(dev, model[1], "video")
    _driver_checks(eng, canvas_p, hop, sched, 5)
    # lookahead=0 is the call without the argument (the plain queue needs n = B * S = 12 steps)
    sched12 = torch.linspace(999, -1, 13).round().long()
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, sched12, 2, SEED, lookahead=0), A.fifo_denoise(eng, canvas_p, hop, sched12, 2, SEED))


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_lookahead_denoise_equals_the_loop_of_its_parts_audio(dev, model, solver):
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop, sched = _setup(dev, model[1], "audio", solver)
    _driver_checks(eng, canvas_p, hop, sched, 5)
    sched8 = torch.linspace(999, -1, 9).round().long()
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, sched8, 2, SEED, lookahead=0), A.fifo_denoise(eng, canvas_p, hop, sched8, 2, SEED))


@pytest.mark.parametrize("target", ["video", "audio"])
def test_supplied_context_continues_a_clip(dev, model, target):
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop, sched = _setup(dev, model[1], target)
    sl = eng.slot_len
    context = torch.randn((8, 2 * sl) + tuple(eng.latent_shape[3:]), generator=torch.Generator().manual_seed(23)).to(dev)
    out = _driver_checks(eng, canvas_p, hop, sched, 3, context)           # the "clean" plan, prefix stability included
    noise_ctx = A.fifo_denoise(eng, canvas_p, hop, sched, 3, SEED, lookahead=2)
    assert not torch.equal(out[:, :sl], noise_ctx[:, :sl])                # the head really sees its context
    other = A.fifo_denoise(eng, canvas_p, hop, sched, 1, SEED, lookahead=2, context=context + 1.0)
    assert not torch.equal(other, out[:, :sl])


def test_lookahead_denoise_refusals(dev, model):
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop, sched = _setup(dev, model[1], "video")
    with pytest.raises(ValueError, match="graph"):
        A.fifo_denoise(eng, canvas_p, hop, sched, 2, SEED, graph=True, lookahead=2)
    for ctx in (4, 7, -1):
        with pytest.raises(ValueError, match="lookahead"):
            A.fifo_denoise(eng, canvas_p, hop, sched, 2, SEED, lookahead=ctx)
    with pytest.raises(ValueError, match="context"):
        A.fifo_denoise(eng, canvas_p, hop, sched, 2, SEED, lookahead=2, context=torch.zeros(8, 3, 16, 16, device=dev))
    with pytest.raises(ValueError, match="context"):
        A.fifo_denoise(eng, canvas_p, hop, sched, 2, SEED, context=torch.zeros(8, 4, 16, 16, device=dev))
    with pytest.raises(ValueError, match="queue"):
        A.fifo_denoise(eng, canvas_p, hop, torch.tensor([999, 749, 499, 249, -1]), 2, SEED, lookahead=2)      # n = 4, B * h = 6
    with pytest.raises(ValueError, match="queue"):
        A.fifo_denoise(eng, canvas_p, hop, sched, 2, SEED, lookahead=1)                                         # n = 6, B * h = 9
