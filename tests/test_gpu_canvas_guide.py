"""The canvas-keyed latent guide on the MI355X (include/avdiff_hip.h, "canvas-keyed known noise"): avd_latent_guide_canvas_f32 against
the float64 mirror and, bit for bit, against the per-sample guide over the canvas positions gathered into windows; the fused
canvas-guided step against the unguided step followed by the elementwise entry (both video kernel forms, audio, cond-only, CFG control,
both solvers at eta 0 and 0.5); a held region under window consensus (the point of the keying, and the per-sample keying's failure);
graph replay; window-offset invariance; stream_generate with an init clip; and the refusals."""
from functools import partial

import numpy as np
import pytest
import torch

import _canvas_guide_ref as CG
import _canvas_noise_ref as CN
import _consensus_ref as W
import _guide_ref as G
from _kit import (ABAR, STREAM_HALF_SECOND, Recorder, audio_case, audio_prompt, components, dev, engine, matmul_f32, model,  # noqa: F401  (dev / model are fixtures)
                  pipeline, soft_mask, ts, video_case, video_prompt, with_sampling)
from _tune import cfg_rows  # noqa: F401  (fixture)
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
SEED, GSEED = 0xDEADBEEF12345678, 0x1234567ABCDEF01          # both key words non-zero
ETA, GD = 0.5, 3.0
_engine = partial(engine, guidance=GD)


def tol(ref):
    """the project's gate: 1e-4 max(1, max |ref|)"""
    return 1e-4 * max(1.0, float(np.abs(ref).max()))


def _eng(model, target, shape, n_prompt, hop, eta, solver="ddim", off=0, **kw):
    """an engine whose windows are `hop` apart: seeded and canvas-keyed, so that every eta takes the same constructor"""
    return _engine(model[1], target, shape, n_prompt, eta=eta, solver=solver, noise_seed=SEED, noise_keying="canvas", canvas_hop=hop,
                   sample_offset=off, **kw)


def _overlapped(shape, hop):
    """bool array of `shape`: the elements on canvas positions under two or more windows"""
    N = shape[0]
    outer, L_, inner = W.dims(shape)
    m = np.zeros((N, outer, L_, inner), dtype=bool)
    for p in range((N - 1) * hop + L_):
        lo, hi = W.window_range(p, L_, hop, N)
        for k in range(lo, hi + 1):
            m[k, :, p - k * hop, :] = hi > lo
    return m.reshape(shape)


# ------------------------------------------------------------------------------------------------- the elementwise kernel
FAR = (2 ** 32 - 6 - 3) // 3                                  # N = 2, L = 6, hop 3: the last canvas position is <= 2^32 - 1
KERNEL_CASES = [
    ("video hop 1", (3, 8, 4, 16, 32), 1, 0),
    ("video hop 3", (3, 8, 4, 16, 32), 3, 7),
    ("video hop 4 = L", (3, 8, 4, 16, 32), 4, 0),
    ("video inner 6", (2, 3, 4, 2, 3), 2, 1),
    ("audio hop 4", (3, 8, 40), 4, 5),
    ("positions next to 2^32", (2, 8, 6, 4, 4), 3, FAR),
]


@pytest.mark.parametrize("name,shape,hop,off", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_kernel_vs_mirror_and_per_sample_gather(dev, name, shape, hop, off):
    from multimodal_diffusion_amd import functional as Fn
    N = shape[0]
    outer, L_, inner = W.dims(shape)
    g = torch.Generator().manual_seed(5)
    known, z = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    m = soft_mask(shape, seed=6)                              # one mask per window: exact 0, exact 1 and fractional entries
    tau = [700, 300, -1][:N] if N == 3 else [700, -1]
    kd, zd, md, td = known.to(dev), z.to(dev), m.to(dev), ts(tau, dev)
    kw = dict(seed=GSEED, canvas_hop=hop, window_offset=off)
    q = Fn.latent_guide(kd, td, ABAR, **kw)                   # z = None: pure forward noising
    got = Fn.latent_guide(kd, td, ABAR, z=zd, mask=md, **kw)
    assert tuple(got.shape) == shape and got.dtype == torch.float32
    # the float64 mirror
    q_ref = CG.q_f64(known.numpy(), tau, ABAR.numpy(), GSEED, hop, off)
    ref = G.blend_f64(m.numpy(), q_ref, z.double().numpy())
    for name_, a, b in (("q", q, q_ref), ("blend", got, ref)):
        err = float(np.abs(a.cpu().double().numpy() - b).max())
        print(f"canvas guide kernel {name}: {name_} max err {err:.3e} (gate {tol(b):.3e})")
        assert err <= tol(b)
    # bit for bit: the per-sample guide over the window's L canvas positions as samples of outer*inner elements, gathered
    for b in range(N):
        rows = kd[b].reshape(outer, L_, inner).permute(1, 0, 2).reshape(L_, outer * inner).contiguous()
        q_rows = Fn.latent_guide(rows, ts([tau[b]] * L_, dev), ABAR, seed=GSEED, sample_offset=(off + b) * hop)
        assert np.array_equal(q[b:b + 1].cpu().numpy(), CN.gather_windows(q_rows.cpu().numpy(), (1,) + shape[1:], hop))
    # tau < 0 returns known bit for bit; both selects and the blend of the contract, in fp32 without contraction
    assert torch.equal(q[-1], kd[-1])
    assert torch.equal(got[md == 0], zd[md == 0]) and torch.equal(got[md == 1], q[md == 1])
    frac = (md > 0) & (md < 1)
    assert torch.equal(got[frac], ((1.0 - md) * zd + md * q)[frac])
    # a mask shared by the batch, no mask (1 everywhere), in place, and an unaligned z (one generator call per element): the same bits
    shared = Fn.latent_guide(kd, td, ABAR, z=zd, mask=md[0].contiguous(), **kw)
    assert torch.equal(shared[0], got[0]) and torch.equal(shared[md[0].expand(shape) == 1], q[md[0].expand(shape) == 1])
    assert torch.equal(Fn.latent_guide(kd, td, ABAR, z=zd, **kw), q)
    buf = torch.empty(z.numel() + 1, device=dev)
    zu = buf[1:].view(shape)
    zu.copy_(zd)
    assert zu.data_ptr() % 16 != 0
    assert torch.equal(Fn.latent_guide(kd, td, ABAR, z=zu, mask=md, **kw), got)
    # windows of one known canvas at one timestep agree on their overlaps, bit for bit; keyed per sample they do not
    canvas = torch.randn((outer, (N - 1) * hop + L_) + shape[3:], generator=g).numpy()
    kc = torch.from_numpy(W.windows_from_canvas(canvas, L_, hop)).to(dev)
    same_t = Fn.latent_guide(kc, ts([500] * N, dev), ABAR, **kw).cpu().numpy()
    per = Fn.latent_guide(kc, ts([500] * N, dev), ABAR, seed=GSEED, sample_offset=off).cpu().numpy()
    assert W.overlaps_agree(same_t, hop) and not np.array_equal(same_t, per)
    if hop < L_:
        assert not W.overlaps_agree(per, hop)


# ------------------------------------------------------------------------------------------------- fused = composed
def _case(dev, kernel, cfg_rows):
    if kernel == "audio":
        z, zp, npr, known = audio_case(dev, B=3, known=True)
        return "audio", z, zp, npr, known, 4
    cfg_rows(1 if kernel == "rows" else 0)
    z, zp, npr, known = video_case(dev, B=3, known=True)
    return "video", z, zp, npr, known, 1


def _fused_vs_composed(dev, model, target, z, zp, npr, known, hop, solver, eta, cond_only, **kw):
    from multimodal_diffusion_amd import functional as Fn
    shape, off = tuple(z.shape), 3
    mask = soft_mask(shape, seed=7).to(dev)
    guided = _eng(model, target, shape, npr, hop, eta, solver, off, **kw)
    plain = _eng(model, target, shape, npr, hop, eta, solver, off, **kw)
    for e in (guided, plain):
        e.set_prompt(zp)
    guided.set_known(known, mask, guide_seed=GSEED, keying="canvas", hop=hop)
    steps = [(ts([981, 402, 40], dev), ts([961, 382, -1], dev), None)]
    if solver == "dpmpp_2m":                                 # a second-order step on the history the first one left
        steps.append((ts([961, 382, 20], dev), ts([941, 362, 0], dev), ts([981, 402, 40], dev)))
    for tn, tp, tl in steps:
        out = guided.step(z, tn, tp, t_last=tl, cond_only=cond_only)
        stepped = plain.step(z, tn, tp, t_last=tl, cond_only=cond_only)
        ref = Fn.latent_guide(known, tp, ABAR, z=stepped, mask=mask, seed=GSEED, canvas_hop=hop, window_offset=off)
        assert torch.equal(out, ref)
        assert not torch.equal(out, stepped)
        if tl is None:                                       # t_prev[2] = -1 returns the known latent where the mask is 1
            keep = (mask == 1)[2]
            assert torch.equal(out[2][keep], known[2][keep])
        if solver == "dpmpp_2m":                             # the history receives the model's x0, not the blended value
            assert torch.equal(guided.x0_hist, plain.x0_hist)
    return guided


@pytest.mark.parametrize("solver,eta", [("ddim", 0.0), ("ddim", ETA), ("dpmpp_2m", 0.0), ("dpmpp_2m", ETA)])
@pytest.mark.parametrize("cond_only", [False, True])
@pytest.mark.parametrize("kernel", ["rows", "gather", "audio"])
def test_fused_step_equals_composed(dev, model, cfg_rows, kernel, cond_only, solver, eta):
    target, z, zp, npr, known, hop = _case(dev, kernel, cfg_rows)
    _fused_vs_composed(dev, model, target, z, zp, npr, known, hop, solver, eta, cond_only)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("kernel", ["rows", "gather", "audio"])
def test_fused_controlled_step_equals_composed(dev, model, cfg_rows, kernel, solver):
    """per-sample guidance and rescale: the control acts on eps before the update, the canvas guide's blend still comes last"""
    target, z, zp, npr, known, hop = _case(dev, kernel, cfg_rows)
    eng = _fused_vs_composed(dev, model, target, z, zp, npr, known, hop, solver, ETA, False, guidance=[2.0, 3.5, 5.0],
                             guidance_rescale=[0.7, 0.0, 1.0])
    assert eng._ctl is not None


# ------------------------------------------------------------------------------------------------- the point of the feature
@pytest.mark.parametrize("target", ["video", "audio"])
def test_held_region_passes_through_the_consensus(dev, model, target):
    """Mask 1 everywhere, B = 3 overlapping windows of one known canvas, non-uniform weights, eta = 0.5: after a step the canvas-keyed
    guide leaves q(t_prev) = A x_canvas + S n_k(p) in every window — the noise term passes through the weighted mean — while the
    per-sample keying, whose windows hold different normals at a shared position, leaves the forward path on the overlaps."""
    if target == "video":
        z, zp, npr = video_case(dev, B=3)
        hop, cshape = 1, (8, 6, 16, 32)
    else:
        z, zp, npr = audio_case(dev, B=3)
        hop, cshape = 4, (8, 48)
    shape, off = tuple(z.shape), 2
    L_ = W.dims(shape)[1]
    canvas = torch.randn(cshape, generator=torch.Generator().manual_seed(4))
    known_np = W.windows_from_canvas(canvas.numpy(), L_, hop)
    known = torch.from_numpy(known_np).to(dev)
    wts = np.linspace(0.5, 2.0, L_).astype(np.float32)
    eng = _eng(model, target, shape, npr, hop, ETA, off=off)
    eng.set_prompt(zp)
    eng.set_window_consensus(hop, torch.from_numpy(wts))
    eng.set_known(known, None, guide_seed=GSEED, keying="canvas", hop=hop)
    tn, tp = ts([900] * 3, dev), ts([700] * 3, dev)
    out = eng.step(z, tn, tp).cpu().numpy()
    ref = CG.q_f64(known_np, [700] * 3, ABAR.numpy(), GSEED, hop, off)
    err = float(np.abs(out.astype(np.float64) - ref).max())
    print(f"held region under consensus ({target}): canvas keying max err {err:.3e} (gate {tol(ref):.3e})")
    assert err <= tol(ref) and W.overlaps_agree(out, hop)
    # the bug the feature removes: the same engine, the guide keyed per sample
    eng.set_known(known, None, guide_seed=GSEED, keying="sample")
    bad = eng.step(z, tn, tp).cpu().numpy()
    ov = _overlapped(shape, hop)
    diff = float(np.abs(bad.astype(np.float64) - out)[ov].max())
    print(f"held region under consensus ({target}): per-sample keying is off by {diff:.3e} on the overlaps")
    assert diff > tol(ref)
    # the last step returns the known latent, then the consensus of the windows: bit for bit
    eng.set_known(known, None, guide_seed=GSEED, keying="canvas", hop=hop)
    last = eng.step(z, ts([40] * 3, dev), ts([-1] * 3, dev)).cpu().numpy()
    assert np.array_equal(last, W.consensus_f32(known_np, hop, wts))


# ------------------------------------------------------------------------------------------------- graph = eager
@pytest.mark.parametrize("n_steps", [5, 6])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_graph_equals_eager(dev, model, solver, n_steps):
    z, zp, npr, known = video_case(dev, B=3, known=True)
    shape, hop = tuple(z.shape), 1
    sched = R.sampling_schedule(1000, n_steps)
    eng = _eng(model, "video", shape, npr, hop, ETA, solver)
    eng.set_prompt(zp)
    eng.set_window_consensus(hop)
    eng.set_known(known, soft_mask(shape[1:], seed=7), guide_seed=GSEED, keying="canvas", hop=hop)
    zg = eng.run(z, sched, graph=True)
    ze = eng.run(z, sched, graph=False)
    assert torch.equal(zg, ze) and W.overlaps_agree(zg.cpu().numpy(), hop)


def test_captured_pair_is_stale_after_a_keying_change(dev, model):
    from multimodal_diffusion_amd import _lib as L
    z, zp, npr, known = video_case(dev, B=3, known=True)
    shape = tuple(z.shape)
    eng = _eng(model, "video", shape, npr, 1, 0.0)
    eng.set_prompt(zp)
    eng.set_known(known, None, guide_seed=GSEED, keying="canvas", hop=1)
    eng.begin(R.sampling_schedule(1000, 6))
    za, zb = z.clone(), torch.empty_like(z)
    eng.advance(za, zb)
    pair = eng.capture_pair(zb, za)
    pair.replay()
    gen = eng._generation
    eng.set_known(known, None, guide_seed=GSEED, keying="canvas", hop=1)         # the same guide: the pair stays valid
    assert eng._generation == gen
    pair.replay()
    eng.set_known(known, None, guide_seed=GSEED, keying="sample")
    assert eng._generation == gen + 1 and "keying" in eng._stale_reason
    with pytest.raises(L.AvdError, match="stale.*keying"):
        pair.replay()
    eng.set_known(known, None, guide_seed=GSEED, keying="canvas", hop=1)         # back again: still a new generation
    with pytest.raises(L.AvdError, match="stale"):
        pair.replay()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- offset invariance
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_window_offset_invariance(dev, model, solver):
    """windows [0, 4) in one engine = windows [0, 2) + [2, 4) in two engines with sample_offset 0 / 2, stepped in lock-step with one
    consensus pass over all windows: bit for bit in the fp32 kernel family"""
    from multimodal_diffusion_amd import functional as Fn
    z, zp, npr, known = video_case(dev, B=4, W=16, known=True)
    shape, hop = tuple(z.shape), 2
    L_ = W.dims(shape)[1]
    z = torch.from_numpy(W.windows_from_canvas(torch.randn(8, 3 * hop + L_, 16, 16, generator=torch.Generator().manual_seed(3)).numpy(),
                                               L_, hop)).to(dev)
    Fn.window_consensus(known, hop)
    mask = soft_mask(shape, seed=9).to(dev)
    wts = torch.linspace(0.5, 2.0, L_)
    sched = R.sampling_schedule(1000, 3)

    def build(sl, off):
        e = _eng(model, "video", (sl.stop - sl.start,) + shape[1:], npr, hop, ETA, solver, off)
        e.set_prompt(zp[sl].contiguous())
        e.set_known(known[sl].contiguous(), mask[sl].contiguous(), guide_seed=GSEED, keying="canvas", hop=hop)
        return e

    with matmul_f32(model[1]):
        whole = build(slice(0, 4), 0)
        whole.set_window_consensus(hop, wts)
        start, sk = whole.start_latent(z, sched, 1.0)
        ref = whole.run(start, sk, graph=False)
        parts = [(slice(0, 2), build(slice(0, 2), 0)), (slice(2, 4), build(slice(2, 4), 2))]
        za = torch.cat([e.start_latent(z[sl].contiguous(), sched, 1.0)[0] for sl, e in parts])
        assert torch.equal(za, start)
        zb = torch.empty_like(za)
        for _, e in parts:
            e.begin(sched)
        for _ in range(len(sched) - 1):
            for sl, e in parts:
                e.advance(za[sl], zb[sl])
            Fn.window_consensus(zb, hop, wts)
            za, zb = zb, za
    assert torch.equal(za, ref) and W.overlaps_agree(ref.cpu().numpy(), hop)


# ------------------------------------------------------------------------------------------------- stream_generate
@pytest.fixture
def stream(dev, model):
    """(kw, cfg, vae, codec): 0.5 s windows every 0.25 s, 32 x 32 frames, a 4-step schedule, 4 windows; the fp32 kernel family whatever
    the batch, so that batch sizes can be compared"""
    with matmul_f32(model[1]):
        vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND)
        yield dict(components(model[1], vae, codec, dev), cfg=cfg, shard=False), cfg, vae, codec


INIT_VIDEO = np.random.default_rng(5).integers(0, 256, size=(20, 32, 32, 3), dtype=np.uint8)          # 20 frames: 4 windows of 0.5 s
INIT_AUDIO = (0.1 * np.random.default_rng(6).standard_normal(18000)).astype(np.float32)              # 18000 samples: 4 windows


def _known_video(dev, vae, consensus_hop=None):
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd import stream_infer as S
    chunks = S.split_frames_into_windows(INIT_VIDEO, 16, 0.5, 0.25)[0]
    fr = torch.from_numpy(np.ascontiguousarray(chunks)).to(dev).float() / 255.0
    known = vae.encode(fr.permute(0, 4, 1, 2, 3).contiguous()).float().contiguous()
    return known if consensus_hop is None else Fn.window_consensus(known, consensus_hop)


@pytest.mark.parametrize("stochastic", [False, True])
def test_stream_generate_inpaints_under_consensus(dev, stream, stochastic):
    from multimodal_diffusion_amd import stream_infer as S
    from multimodal_diffusion_amd.sampler import canvas_frame_mask
    kw, cfg, vae, _ = stream
    hop, L_ = S.latent_hop(cfg, "video")
    assert (hop, L_) == (1, 2)
    mask = canvas_frame_mask((8, 5, 4, 4), 0, 2)
    kws = dict(kw, consensus="uniform", return_latents=True, init_video=INIT_VIDEO, mask=mask, guide_seed=11, **audio_prompt())
    if stochastic:
        kws.update(cfg=with_sampling(cfg, ddim_eta=0.5, solver="dpmpp_2m"), noise_keying="canvas", noise_seed=3)
    whole = S.stream_generate(**kws)
    lat = whole["latents"]
    assert lat.shape == (4, 8, 2, 4, 4) and np.isfinite(lat).all() and W.overlaps_agree(lat, hop)
    # the held canvas positions are the consensed encoded windows, bit for bit; the free ones are not
    known = S.canvas_from_windows(_known_video(dev, vae, hop), hop).cpu().numpy()
    canvas = S.canvas_from_windows(torch.from_numpy(lat), hop).numpy()
    assert np.array_equal(canvas[:, :2], known[:, :2]) and not np.array_equal(canvas[:, 2:], known[:, 2:])
    # max_windows_per_batch 2: lock-step engines whose guide (and noise) start at their first window
    part = S.stream_generate(max_windows_per_batch=2, **kws)
    assert np.array_equal(part["latents"], lat) and np.array_equal(part["video"], whole["video"])
    # the init clip is live in the free region too (the overlap of window 1 sees the held position 1), as is the guide seed's noise
    free = S.stream_generate(**{k: v for k, v in kws.items() if k not in ("init_video", "mask", "guide_seed")})
    assert not np.array_equal(free["latents"], lat)


def test_stream_generate_without_consensus_is_the_per_window_loop(dev, stream, model):
    from multimodal_diffusion_amd import stream_infer as S
    from multimodal_diffusion_amd import schedule_utils as su
    from multimodal_diffusion_amd.sampler import canvas_frame_mask
    kw, cfg, vae, codec = stream
    mask = canvas_frame_mask((8, 5, 4, 4), 1, 3)
    prompt = audio_prompt()
    kws = dict(kw, return_latents=True, init_video=INIT_VIDEO, mask=mask, guide_seed=11, strength=0.75, **prompt)
    whole = S.stream_generate(**kws)
    lat = whole["latents"]
    for mw in (2, 1):
        assert np.array_equal(S.stream_generate(max_windows_per_batch=mw, **kws)["latents"], lat)
    # by hand: one engine per window, the guide keyed per sample with sample_offset = the window index
    known = _known_video(dev, vae)
    mask_w = S.windows_from_canvas(mask, 2, 1)
    wav = S.split_audio_into_windows(prompt["prompt_audio"], 16000, 0.5, 0.25)[0]
    z_p = codec.encode(torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).to(dev)[:, None, :])
    z0 = torch.randn(4, 8, 2, 4, 4, generator=torch.Generator().manual_seed(prompt["seed"]))
    c = cfg["diffusion"]["video"]
    abar = su.alphas_cumprod_from_betas(su.make_beta_schedule(1000, kind=c["schedule"], min_beta=c["min_beta"], max_beta=c["max_beta"]))[1]
    sched = su.make_sampling_schedule(1000, 4)
    for i in range(4):
        eng = engine(model[1], "video", (1, 8, 2, 4, 4), (150 - 4) // 4 + 1, guidance=2.0, alpha_bar=abar)
        eng.set_prompt(z_p[i:i + 1].float().contiguous())
        eng.set_known(known[i:i + 1], mask_w[i:i + 1], guide_seed=11, sample_offset=i)
        z, sk = eng.start_latent(z0[i:i + 1].to(dev), sched, 0.75)
        assert sk.numel() == 4
        assert np.array_equal(eng.run(z, sk).cpu().numpy(), lat[i:i + 1])
    keep = mask_w.numpy() == 1
    assert np.array_equal(lat[keep], known.cpu().numpy()[keep])


def test_stream_generate_strength_zero_and_sdedit(dev, stream):
    from multimodal_diffusion_amd import stream_infer as S
    kw, cfg, vae, _ = stream
    rec = Recorder(vae)
    kws = dict(kw, vid_vae=rec, init_video=INIT_VIDEO, return_latents=True, **audio_prompt())
    out = S.stream_generate(strength=0.0, **kws)
    known = _known_video(dev, vae)
    assert torch.equal(rec.last, known) and np.array_equal(out["latents"], known.cpu().numpy())
    x = vae.decode(known).clamp(0, 1)
    frames = (x.permute(0, 2, 3, 4, 1) * 255.0).to(torch.uint8).contiguous()
    stitched = S.crossfade_tensor(frames, torch.from_numpy(S.video_fade_window(8, 2)), 4).cpu().numpy()
    assert out["video"].shape == (20, 32, 32, 3) and np.array_equal(out["video"], stitched)
    cons = S.stream_generate(strength=0.0, consensus="uniform", **kws)
    assert np.array_equal(cons["latents"], _known_video(dev, vae, 1).cpu().numpy())
    # SDEdit without a mask: a variation of the clip, for any batching; strength 1 without a mask leaves the init clip unused
    half = S.stream_generate(strength=0.5, consensus="uniform", **kws)
    assert W.overlaps_agree(half["latents"], 1) and not np.array_equal(half["latents"], cons["latents"])
    assert np.array_equal(S.stream_generate(strength=0.5, consensus="uniform", max_windows_per_batch=2, **kws)["latents"], half["latents"])
    plain = S.stream_generate(**{k: v for k, v in kws.items() if k != "init_video"})
    assert np.array_equal(S.stream_generate(**kws)["latents"], plain["latents"])
    # an all-zero mask is no guide: today's output, bit for bit
    zero = S.stream_generate(mask=torch.zeros(8, 5, 4, 4), **kws)
    assert np.array_equal(zero["latents"], plain["latents"]) and np.array_equal(zero["video"], plain["video"])


def test_stream_generate_video_prompt_direction(dev, stream):
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd import stream_infer as S
    from multimodal_diffusion_amd.sampler import canvas_frame_mask
    kw, cfg, _, codec = stream
    assert S.latent_hop(cfg, "audio") == (75, 150)
    mask = canvas_frame_mask((8, 375), 0, 100)
    kws = dict(kw, consensus="uniform", return_latents=True, init_audio=INIT_AUDIO, mask=mask, **video_prompt())
    whole = S.stream_generate(**kws)
    lat = whole["latents"]
    assert lat.shape == (4, 8, 150) and W.overlaps_agree(lat, 75) and np.isfinite(whole["audio"]).all()
    wav = S.split_audio_into_windows(INIT_AUDIO, 16000, 0.5, 0.25)[0]
    known = codec.encode(torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32)).to(dev)[:, None, :]).float().contiguous()
    kc = S.canvas_from_windows(Fn.window_consensus(known, 75), 75).cpu().numpy()
    canvas = S.canvas_from_windows(torch.from_numpy(lat), 75).numpy()
    assert np.array_equal(canvas[:, :100], kc[:, :100]) and not np.array_equal(canvas[:, 100:], kc[:, 100:])
    assert np.array_equal(S.stream_generate(max_windows_per_batch=2, **kws)["latents"], lat)


# ------------------------------------------------------------------------------------------------- misuse
def test_engine_misuse(dev, model):
    z, zp, npr, known = video_case(dev, B=3, W=16, known=True)
    shape = tuple(z.shape)
    eng = _eng(model, "video", shape, npr, 2, ETA)
    gen = eng._generation
    with pytest.raises(ValueError, match="keying"):
        eng.set_known(known, None, keying="position", hop=2)
    with pytest.raises(ValueError, match="needs hop"):
        eng.set_known(known, None, keying="canvas")
    with pytest.raises(ValueError, match="hop belongs"):
        eng.set_known(known, None, hop=2)
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            eng.set_known(known, None, keying="canvas", hop=bad)
    with pytest.raises(ValueError, match="canvas_hop"):
        eng.set_known(known, None, keying="canvas", hop=3)                       # the engine's noise is keyed for hop 2
    with pytest.raises(ValueError, match="2\\*\\*32"):
        eng.set_known(known, None, keying="canvas", hop=2, sample_offset=2 ** 32 - 2)
    assert eng._guide is None and eng._generation == gen                         # nothing changed
    # a canvas guide at eta > 0 needs the canvas-keyed engine: per-sample step noise is refused
    seeded = _engine(model[1], "video", shape, npr, eta=ETA, noise_seed=SEED)
    with pytest.raises(ValueError, match="noise_keying='canvas'"):
        seeded.set_known(known, None, keying="canvas", hop=2)
    # the consensus hop and the guide's hop are checked in either order (eta == 0: any consensus hop is allowed otherwise)
    det = _engine(model[1], "video", shape, npr, eta=0.0)
    det.set_window_consensus(3)
    with pytest.raises(ValueError, match="consensus hop 3"):
        det.set_known(known, None, keying="canvas", hop=2)
    det.set_known(known, None, keying="canvas", hop=3)
    with pytest.raises(ValueError, match="guide's hop 3"):
        det.set_window_consensus(2)
    assert det._cons_hop == 3
    det.clear_known()
    det.set_window_consensus(2)                                                  # no guide: free again
    # the C entry refuses what the engine would never send: a canvas guide over per-sample step noise
    from multimodal_diffusion_amd import _lib as L
    import ctypes as C
    seeded.set_prompt(zp)
    seeded.set_known(known, None)
    out = torch.empty_like(z)
    tn, tp = ts([900] * 3, dev), ts([700] * 3, dev)
    rc = L.lib().avd_denoise_step_canvas_guided_f32(C.byref(seeded.desc), C.byref(seeded._guide), 2, None, None, 0, None, None,
                                                    z.data_ptr(), seeded.Xp.data_ptr(), tn.data_ptr(), tp.data_ptr(), out.data_ptr(),
                                                    seeded.workspace.data_ptr(), seeded.workspace.numel(), L.stream_ptr(dev))
    assert rc == L.EINVAL and b"noise key" in L.lib().avd_last_error()


def test_stream_generate_misuse(dev, stream):
    from multimodal_diffusion_amd import stream_infer as S
    kw, cfg, _, _ = stream
    a2v = dict(kw, **audio_prompt())
    with pytest.raises(ValueError, match="init_audio"):
        S.stream_generate(init_audio=INIT_AUDIO, **a2v)
    with pytest.raises(ValueError, match="init clip"):
        S.stream_generate(mask=torch.ones(8, 5, 4, 4), **a2v)
    with pytest.raises(ValueError, match="init clip"):
        S.stream_generate(strength=0.5, **a2v)
    with pytest.raises(ValueError, match="windows"):
        S.stream_generate(init_video=INIT_VIDEO[:12], **a2v)
    with pytest.raises(ValueError, match="broadcast"):
        S.stream_generate(init_video=INIT_VIDEO, mask=torch.ones(8, 4, 4, 4), **a2v)
    with pytest.raises(ValueError, match="second broadcast"):
        S.stream_generate(init_video=INIT_VIDEO, **dict(a2v, shard=True))
    # eta > 0 under consensus still needs the canvas-keyed noise, with or without an init clip
    with pytest.raises(ValueError, match="ddim_eta.*noise_keying='canvas'"):
        S.stream_generate(init_video=INIT_VIDEO, consensus="uniform", noise_seed=3, **dict(a2v, cfg=with_sampling(cfg, ddim_eta=0.5)))
