"""The clip-keyed latent guide on the MI355X (include/avdiff_hip.h, "clip-keyed latent guide"): the stand-alone pass against the numpy
mirror and, bit for bit, against the canvas-keyed guide kernel; the fused guided slot updates against their composition (the unguided
seeded entry, then the stand-alone pass); the edges; and the whole step on the reduced model."""
import ctypes as C

import numpy as np
import pytest
import torch

import _clip_guide_ref as CG
import _slot_dpm_ref as SD
import _slot_ref as SR
from _kit import ABAR, case, dev, engine, model, soft_mask, ts  # noqa: F401  (dev, model are fixtures)
from _tune import tuned

pytestmark = pytest.mark.gpu

GS = 3.5
SEED = 0x5107_5EED_0001          # the slot key's: the step noise
GSEED = 0x4B4E_0BAD_CAFE         # the guide's known noise
# the shapes of test_gpu_slot_noise.py: W = 32 / 16 / 8 take the 8-token and the 4-token whole-line forms and the gather form; tube
# t = 1: S = T; B = 3
VIDEO_CASES = [((2, 8, 4, 16, 32), (2, 4, 4)), ((2, 8, 4, 16, 16), (2, 4, 4)), ((2, 8, 4, 16, 8), (2, 4, 4)),
               ((3, 8, 4, 16, 16), (2, 4, 4)), ((2, 8, 4, 16, 32), (1, 4, 4))]
# 16-byte lanes, the one-element path (inner = 15), audio (inner = 1), audio with an uncovered tail
PASS_SHAPES = [((2, 8, 4, 16, 32), 2), ((2, 3, 4, 3, 5), 2), ((2, 8, 40), 4), ((2, 8, 42), 4)]


def tol(ref):
    """the project's gate: 1e-4 max(1, max |ref|)"""
    return 1e-4 * max(1.0, float(np.abs(ref).max()))


def _lib():
    from multimodal_diffusion_amd import _lib as L
    return L, L.lib()


def cur(dev, v):
    return torch.tensor([v], dtype=torch.int32, device=dev)


def off(x):
    """a copy of x whose base is misaligned by one float"""
    v = torch.empty(x.numel() + 1, device=x.device)[1:].view(x.shape)
    assert v.data_ptr() % 16 != 0
    return v.copy_(x)


def _canvases(dev, shape, P, seed=0):
    """(known, soft mask) canvases [outer, P, *inner] for a batch of `shape`"""
    g = torch.Generator().manual_seed(seed + P)
    cs = (shape[1], P) + tuple(shape[3:])
    return torch.randn(cs, generator=g).to(dev), soft_mask(cs, seed=seed + 3).to(dev)


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ------------------------------------------------------------------------------------------------- 1. the stand-alone pass
@pytest.mark.parametrize("shape,slot_len", PASS_SHAPES)
def test_stand_alone_pass_equals_the_mirror(dev, shape, slot_len):
    from multimodal_diffusion_amd import functional as Fn
    B, L_ = shape[0], shape[2]
    S = L_ // slot_len
    P = 2 * L_ + 3                                       # sample 1 runs past the canvas end at first = 0 already
    known, mask = _canvases(dev, shape, P)
    z = torch.randn(shape, generator=torch.Generator().manual_seed(L_)).to(dev)
    tau, _ = SR.tables(B, S, seed=L_)
    tau[0, 0] = -1                                       # a == 1: q = x_k
    kw = dict(slot_len=slot_len, seed=GSEED)
    for first in (0, 5, -3, P):                          # P: every position past the canvas end
        out = Fn.clip_guide_slots(known, tau, ABAR, z, mask, first=first, **kw)
        ref = CG.clip_guide_slots(_np(known), _np(mask), tau.numpy(), ABAR.numpy(), _np(z), GSEED, slot_len, first=first)
        err = float(np.abs(_np(out) - ref).max())
        print(f"clip_guide_slots {shape} first {first}: max err {err:.3e} (gate {tol(ref):.3e})")
        assert err < tol(ref), (first, err)
        if first == P:
            assert torch.equal(out, z)
        else:
            assert not torch.equal(out, z)
        # misaligned bases take the one-element lanes: the aligned call's bits
        for kn, mk, zz in ((off(known), mask, z), (known, off(mask), z), (known, mask, off(z))):
            assert torch.equal(Fn.clip_guide_slots(kn, tau, ABAR, zz, mk, first=first, **kw), out), first
        assert torch.equal(Fn.clip_guide_slots(known, tau, ABAR, z, mask, first=first, out=off(z), **kw), out), first
    base = Fn.clip_guide_slots(known, tau, ABAR, z, mask, first=5, **kw)
    # a cursor adds to first; a negative one reads as 0; the stride moves the samples apart
    assert torch.equal(Fn.clip_guide_slots(known, tau, ABAR, z, mask, first=-2, cursor=cur(dev, 7), **kw), base)
    for m in (-1, -2 ** 31):
        assert torch.equal(Fn.clip_guide_slots(known, tau, ABAR, z, mask, first=5, cursor=cur(dev, m), **kw), base), m
    for m in (2 ** 31 - 1,):                             # a cursor far past the canvas: nothing is read, nothing is guided
        assert torch.equal(Fn.clip_guide_slots(known, tau, ABAR, z, mask, first=5, cursor=cur(dev, m), **kw), z)
    near = Fn.clip_guide_slots(known, tau, ABAR, z, mask, first=0, stride=1, **kw)
    ref = CG.clip_guide_slots(_np(known), _np(mask), tau.numpy(), ABAR.numpy(), _np(z), GSEED, slot_len, first=0, stride=1)
    assert float(np.abs(_np(near) - ref).max()) < tol(ref)
    # another seed, another known noise (first = 1: slots with a < 1 lie inside the canvas)
    assert not torch.equal(Fn.clip_guide_slots(known, tau, ABAR, z, mask, first=1, slot_len=slot_len, seed=GSEED + 1),
                           Fn.clip_guide_slots(known, tau, ABAR, z, mask, first=1, **kw))
    # everywhere == an all-ones mask == no mask, bit for bit
    every = Fn.clip_guide_slots(known, tau, ABAR, z, mask, first=1, everywhere=True, **kw)
    assert torch.equal(every, Fn.clip_guide_slots(known, tau, ABAR, z, torch.ones_like(mask), first=1, **kw))
    assert torch.equal(every, Fn.clip_guide_slots(known, tau, ABAR, z, None, first=1, **kw))


@pytest.mark.parametrize("shape,slot_len", PASS_SHAPES)
def test_left_slots_keep_z_in_place_and_out_of_place(dev, shape, slot_len):
    from multimodal_diffusion_amd import functional as Fn
    B, L_ = shape[0], shape[2]
    S = L_ // slot_len
    known, _ = _canvases(dev, shape, 3 * L_)
    z = torch.randn(shape, generator=torch.Generator().manual_seed(7)).to(dev)
    tau = torch.full((B, S), Fn.SLOT_LEAVE)
    tau[B - 1, S - 1] = 500                              # the tail slot alone (with F = 42 it owns the uncovered frames)
    full = Fn.clip_guide_slots(known, torch.full((B, S), 500), ABAR, z, slot_len=slot_len, seed=GSEED)
    lo = (S - 1) * slot_len
    want = z.clone()
    want[B - 1, :, lo:] = full[B - 1, :, lo:]
    assert not torch.equal(want, z)
    out = Fn.clip_guide_slots(known, tau, ABAR, z, slot_len=slot_len, seed=GSEED)
    assert torch.equal(out, want)
    buf = z.clone()
    assert Fn.clip_guide_slots(known, tau, ABAR, buf, slot_len=slot_len, seed=GSEED, out=buf) is buf
    assert torch.equal(buf, want)
    # every slot left: z, and an in-place call writes nothing (a NaN the kernel would have to rewrite stays)
    left = torch.full((B, S), Fn.SLOT_LEAVE)
    assert torch.equal(Fn.clip_guide_slots(known, left, ABAR, z, slot_len=slot_len, seed=GSEED), z)
    buf = z.clone()
    buf[0, 0, 0] = float("nan")
    Fn.clip_guide_slots(known, left, ABAR, buf, slot_len=slot_len, seed=GSEED, out=buf)
    assert torch.isnan(buf[0, 0, 0]).all() and torch.equal(buf[1], z[1])


# ------------------------------------------------------------------------------------------------- 2. against the canvas-keyed kernel
@pytest.mark.parametrize("shape,slot_len,stride,first", [((2, 8, 4, 16, 32), 2, 2, 4), ((3, 8, 4, 16, 16), 2, 1, 3),
                                                         ((2, 3, 4, 2, 3), 2, 3, 0), ((2, 8, 40), 4, 10, 10), ((2, 8, 42), 4, 7, 14)])
def test_uniform_tau_equals_the_canvas_keyed_guide_bit_for_bit(dev, shape, slot_len, stride, first):
    from multimodal_diffusion_amd import functional as Fn
    B, L_ = shape[0], shape[2]
    S = L_ // slot_len
    hop, w0 = stride * slot_len, first // stride
    assert first % stride == 0
    P = (w0 + B - 1) * hop + L_                          # the canvas ends with the last window
    known, mask = _canvases(dev, shape, P, seed=5)
    z = torch.randn(shape, generator=torch.Generator().manual_seed(11)).to(dev)
    t = torch.tensor([612, -1, 87][:B])
    tau = t[:, None].expand(B, S).contiguous()
    win = lambda c: torch.stack([c[:, (w0 + b) * hop:(w0 + b) * hop + L_] for b in range(B)], 0).contiguous()
    for m in (mask, None):
        out = Fn.clip_guide_slots(known, tau, ABAR, z, m, slot_len=slot_len, seed=GSEED, first=first, stride=stride)
        ref = Fn.latent_guide(win(known), t, ABAR, z, None if m is None else win(m), seed=GSEED, canvas_hop=hop, window_offset=w0)
        assert torch.equal(out, ref), float((out - ref).abs().max())


# ------------------------------------------------------------------------------------------------- 3. the fused updates
def _video_inputs(dev, shape, tube):
    g = torch.Generator().manual_seed(sum(shape) + tube[0])
    return torch.randn(shape, generator=g).to(dev), torch.randn(2 * shape[0], int(np.prod(shape[1:])), generator=g).to(dev)


def _video(dev, shape, tube, z, eps2, tabs, eta, key, guide=None, hist=None):
    """z_out of the guided (guide set) or the unguided seeded video slot update; tabs = (tn, tp) or (tl, tn, tp), device tables"""
    L, lib = _lib()
    B, Cc, T, H, W = shape
    tl = tabs[0] if len(tabs) == 3 else None
    tn, tp = tabs[-2:]
    out, ab = torch.full(shape, float("nan"), device=dev), ABAR.to(dev)
    head = (eps2.data_ptr(), z.data_ptr(), L.ptr(tl), tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), 1000, GS, eta)
    tail = (T // tube[0], L.ptr(hist), out.data_ptr(), B, Cc, T, H, W, *tube, L.stream_ptr(dev))
    if guide is None:
        L.check(lib.avd_cfg_unpatch_ddim_slots_seeded_f32(*head, C.byref(key), *tail))
    else:
        L.check(lib.avd_cfg_unpatch_ddim_slots_guided_f32(*head, None if key is None else C.byref(key), C.byref(guide), *tail))
    return out


def _audio_inputs(dev, F):
    g = torch.Generator().manual_seed(F)
    return torch.randn((2, 8, F), generator=g).to(dev), torch.randn(4, (F - 4) // 4 + 1, 32, generator=g).to(dev)


def _audio(dev, z, eps2, tabs, eta, key, guide=None, hist=None):
    L, lib = _lib()
    tl = tabs[0] if len(tabs) == 3 else None
    tn, tp = tabs[-2:]
    out, ab = torch.full_like(z, float("nan")), ABAR.to(dev)
    head = (eps2.data_ptr(), z.data_ptr(), L.ptr(tl), tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), 1000, GS, eta)
    tail = (tn.shape[1], L.ptr(hist), out.data_ptr(), *z.shape, 4, 4, L.stream_ptr(dev))
    if guide is None:
        L.check(lib.avd_cfg_untoken_ddim_audio_slots_seeded_f32(*head, C.byref(key), *tail))
    else:
        L.check(lib.avd_cfg_untoken_ddim_audio_slots_guided_f32(*head, None if key is None else C.byref(key), C.byref(guide), *tail))
    return out


def _tables(dev, solver, B, S, seed):
    """device tables of the solver — (tn, tp) or (tl, tn, tp) — with a hold and a final step among them, and the guide's tau: t_prev,
    held slots left"""
    from multimodal_diffusion_amd import functional as Fn
    tabs = SR.tables(B, S, seed=seed) if solver == "ddim" else SD.tables3(B, S, seed=seed)
    tn, tp = tabs[-2:]
    assert (tn == tp).any() and (tp == -1).any()
    tau = torch.where(tn == tp, torch.full_like(tp, Fn.SLOT_LEAVE), tp)
    return tuple(t.to(dev) for t in tabs), tau


def _hist(z, solver, seed=5):
    return None if solver == "ddim" else torch.randn(z.shape, generator=torch.Generator().manual_seed(seed)).to(z.device)


@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("shape,tube", VIDEO_CASES)
def test_video_guided_update_equals_the_composition(dev, shape, tube, solver, eta):
    from multimodal_diffusion_amd import functional as Fn
    B, S, sl = shape[0], shape[2] // tube[0], tube[0]
    tabs, tau = _tables(dev, solver, B, S, seed=S * 8 + B)
    z, eps2 = _video_inputs(dev, shape, tube)
    first, stride, m = -3, S + 1, 2                      # the cursor moves everything by 2: sample 0 starts one slot before the canvas
    P = (first + m + stride * (B - 1) + S) * sl - 1      # ... and the batch's last position is the first one past its end
    known, mask = _canvases(dev, shape, P)
    cursor = cur(dev, m)
    key = Fn.slot_key(SEED, first, stride, cursor)
    guide = Fn.clip_guide(known, mask, GSEED, first, stride, cursor, shape)
    h0 = _hist(z, solver)
    hg, hu = (None, None) if h0 is None else (h0.clone(), h0.clone())
    out = _video(dev, shape, tube, z, eps2, tabs, eta, key, guide, hist=hg)
    plain = _video(dev, shape, tube, z, eps2, tabs, eta, key, hist=hu)
    ref = Fn.clip_guide_slots(known, tau, ABAR, plain, mask, slot_len=sl, seed=GSEED, first=first + m, stride=stride)
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref), float((out - ref).abs().max())
    assert not torch.equal(out, plain)                   # the guide is live
    if h0 is not None:                                   # x0_hist receives the model's x0, not a blended value
        assert torch.equal(hg, hu)
    hold = (SR.per_position(tabs[-2], shape[2], sl, z) == SR.per_position(tabs[-1], shape[2], sl, z)).expand_as(z)
    assert hold.any() and torch.equal(out[hold], z[hold])
    # the gather and the whole-line forms agree; at eta == 0 the key may be null
    with tuned(cfg_rows=0):
        hq = None if h0 is None else h0.clone()
        assert torch.equal(_video(dev, shape, tube, z, eps2, tabs, eta, key, guide, hist=hq), out)
    if eta == 0:
        hq = None if h0 is None else h0.clone()
        assert torch.equal(_video(dev, shape, tube, z, eps2, tabs, eta, None, guide, hist=hq), out)
    # misaligned canvases: the same bits through scalar canvas reads
    kn, mk = off(known), off(mask)
    g2 = Fn.clip_guide(kn, mk, GSEED, first, stride, cursor, shape)
    hq = None if h0 is None else h0.clone()
    assert torch.equal(_video(dev, shape, tube, z, eps2, tabs, eta, key, g2, hist=hq), out)


@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("F", [40, 42])                  # 42: two uncovered frames, which follow the last slot
def test_audio_guided_update_equals_the_composition(dev, F, solver, eta):
    from multimodal_diffusion_amd import functional as Fn
    S = 10
    tabs, tau = _tables(dev, solver, 2, S, seed=F)
    z, eps2 = _audio_inputs(dev, F)
    first, stride = -2, S
    known, mask = _canvases(dev, tuple(z.shape), 2 * F - 13)
    key = Fn.slot_key(SEED, first, stride)
    guide = Fn.clip_guide(known, mask, GSEED, first, stride, None, tuple(z.shape))
    h0 = _hist(z, solver)
    hg, hu = (None, None) if h0 is None else (h0.clone(), h0.clone())
    out = _audio(dev, z, eps2, tabs, eta, key, guide, hist=hg)
    plain = _audio(dev, z, eps2, tabs, eta, key, hist=hu)
    ref = Fn.clip_guide_slots(known, tau, ABAR, plain, mask, slot_len=4, seed=GSEED, first=first, stride=stride)
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref), float((out - ref).abs().max())
    assert not torch.equal(out, plain)
    if h0 is not None:
        assert torch.equal(hg, hu)
    hold = (SR.per_position(tabs[-2], F, 4, z) == SR.per_position(tabs[-1], F, 4, z)).expand_as(z)
    assert hold.any() and torch.equal(out[hold], z[hold])


# ------------------------------------------------------------------------------------------------- 4. edges
@pytest.mark.parametrize("target", ["video", "audio"])
def test_edges_zero_mask_missed_canvas_final_step_fractional_mask_and_mismatch(dev, target):
    from multimodal_diffusion_amd import functional as Fn
    L, lib = _lib()
    eta = 0.5
    if target == "video":
        shape, tube, sl = (2, 8, 4, 16, 16), (2, 4, 4), 2
        z, eps2 = _video_inputs(dev, shape, tube)
        run = lambda tabs, key, guide=None: _video(dev, shape, tube, z, eps2, tabs, eta, key, guide)
    else:
        shape, sl = (2, 8, 40), 4
        z, eps2 = _audio_inputs(dev, 40)
        run = lambda tabs, key, guide=None: _audio(dev, z, eps2, tabs, eta, key, guide)
    S = shape[2] // sl
    tabs, tau = _tables(dev, "ddim", 2, S, seed=9)
    P = 2 * shape[2]
    known, mask = _canvases(dev, shape, P)
    key = Fn.slot_key(SEED, 0, S)
    plain = run(tabs, key)
    mk = lambda m, first=0: Fn.clip_guide(known, m, GSEED, first, S, None, shape)
    # an all-zero mask, and a canvas every position misses (before its start, past its end): the unguided bits
    zero = torch.zeros_like(mask)
    assert torch.equal(run(tabs, key, mk(zero)), plain)
    for first in (-2 * S, 2 * S):
        k2 = Fn.slot_key(SEED, first, S)
        assert torch.equal(run(tabs, k2, mk(None, first)), run(tabs, k2))
    # m == 1 at t_prev = -1 returns x_k bit for bit; m == 1 elsewhere is q; a fractional mask follows the mirror
    out = run(tabs, key, mk(mask))
    tp_e = SR.per_position(tabs[-1], shape[2], sl, z).expand_as(z)
    stepping = (SR.per_position(tabs[-2], shape[2], sl, z) != SR.per_position(tabs[-1], shape[2], sl, z)).expand_as(z)
    kw = torch.stack([known[:, b * shape[2]:(b + 1) * shape[2]] for b in range(2)], 0)
    mw = torch.stack([mask[:, b * shape[2]:(b + 1) * shape[2]] for b in range(2)], 0)
    final = stepping & (tp_e == -1) & (mw == 1)
    assert final.any() and torch.equal(out[final], kw[final])
    ref = CG.clip_guide_slots(_np(known), _np(mask), tau.numpy(), ABAR.numpy(), _np(plain), GSEED, sl)
    frac = (stepping & (mw > 0) & (mw < 1)).cpu().numpy()
    assert frac.any()
    err = float(np.abs(_np(out) - ref).max())
    print(f"guided {target} update vs mirror on the unguided update: max err {err:.3e} (gate {tol(ref):.3e})")
    assert err < tol(ref)
    assert float(np.abs(_np(out) - _np(plain))[frac].max()) > 0
    # a key whose geometry is not the guide's is refused, and nothing is written
    c0 = cur(dev, 0)
    for bad in (Fn.slot_key(SEED, 1, S), Fn.slot_key(SEED, 0, S + 1), Fn.slot_key(SEED, 0, S, c0)):
        with pytest.raises(ValueError, match="must equal the clip guide"):
            run(tabs, bad, mk(mask))


# ------------------------------------------------------------------------------------------------- 5. the whole step
def _uniform(t, B, S, dev):
    return torch.tensor(t, dtype=torch.long, device=dev)[:, None].expand(B, S).contiguous()


@pytest.mark.parametrize("solver,eta", [("ddim", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0), ("dpmpp_2m", 1.0)])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_guided_step_slots_equals_the_unguided_step_then_the_pass(dev, model, target, solver, eta):
    from multimodal_diffusion_amd import functional as Fn
    z, zp, npr, h0 = case(dev, target, B=2)
    kw = dict(guidance=GS, matmul="f32", solver=solver, eta=eta, **({"noise_seed": SEED} if eta else {}))
    eng = engine(model[1], target, tuple(z.shape), npr, **kw)
    eng.set_prompt(zp)
    S, sl = eng.slots, eng.slot_len
    tabs, tau = _tables(dev, solver, 2, S, seed=21)
    tl = tabs[0] if solver != "ddim" else None
    first, stride = 1, S + 1
    cursor = cur(dev, 1)
    known, mask = _canvases(dev, tuple(z.shape), 2 * z.shape[2] + 1)
    step = dict(t_last=tl, clip_first=first, clip_stride=stride, clip_cursor=cursor)
    if tl is not None:
        eng.x0_hist.copy_(h0)
    plain = eng.step_slots(z, *tabs[-2:], **step)
    hu = None if tl is None else eng.x0_hist.clone()
    eng.set_clip_guide(known, mask, guide_seed=GSEED)
    if tl is not None:
        eng.x0_hist.copy_(h0)
    out = eng.step_slots(z, *tabs[-2:], **step)
    ref = Fn.clip_guide_slots(known, tau, ABAR, plain, mask, slot_len=sl, seed=GSEED, first=first + 1, stride=stride)
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref), float((out - ref).abs().max())
    assert not torch.equal(out, plain)
    if tl is not None:
        assert torch.equal(eng.x0_hist, hu)
    # the engine's refusals under a clip guide, and back to the unguided step
    with pytest.raises(ValueError, match="clip_first, at any eta"):
        eng.step_slots(z, *tabs[-2:], t_last=tl)
    with pytest.raises(ValueError, match="step takes no clip guide"):
        eng.step(z, ts([500, 500], dev), ts([400, 400], dev))
    eng.clear_clip_guide()
    if tl is not None:
        eng.x0_hist.copy_(h0)
    assert torch.equal(eng.step_slots(z, *tabs[-2:], **step), plain)
    eng.set_known(z)
    with pytest.raises(ValueError, match=r"step_slots takes no latent guide \(its forward path is keyed by one t_prev per sample\)"):
        eng.step_slots(z, *tabs[-2:], **step)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_uniform_tables_give_the_canvas_guided_per_sample_step(dev, model, target, solver):
    """eta == 0, one pair per sample, first a multiple of stride = S: the windows of set_known(keying="canvas", hop=L)"""
    z, zp, npr, h0 = case(dev, target, B=2)
    kw = dict(guidance=GS, matmul="f32", solver=solver)
    eng = engine(model[1], target, tuple(z.shape), npr, **kw)
    per = engine(model[1], target, tuple(z.shape), npr, **kw)
    eng.set_prompt(zp)
    per.set_prompt(zp)
    S, L_ = eng.slots, z.shape[2]
    assert S * eng.slot_len == L_
    w0 = 1
    known, mask = _canvases(dev, tuple(z.shape), (w0 + 2) * L_)
    tl, tn, tp = [-1, 620], [981, 402], [961, -1]
    eng.set_clip_guide(known, mask, guide_seed=GSEED)
    win = lambda c: torch.stack([c[:, (w0 + b) * L_:(w0 + b + 1) * L_] for b in range(2)], 0).contiguous()
    per.set_known(win(known), win(mask), guide_seed=GSEED, keying="canvas", hop=L_, sample_offset=w0)
    dpm = solver == "dpmpp_2m"
    if dpm:
        eng.x0_hist.copy_(h0)
        per.x0_hist.copy_(h0)
    out = eng.step_slots(z, _uniform(tn, 2, S, dev), _uniform(tp, 2, S, dev), t_last=_uniform(tl, 2, S, dev) if dpm else None,
                         clip_first=w0 * S)
    ref = per.step(z, ts(tn, dev), ts(tp, dev), t_last=ts(tl, dev) if dpm else None)
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref), float((out - ref).abs().max())
    if dpm:
        assert torch.equal(eng.x0_hist, per.x0_hist)
    hard = win(mask)[1] == 1
    assert hard.any() and torch.equal(out[1][hard], win(known)[1][hard])        # sample 1's final step returns x_k where m == 1
