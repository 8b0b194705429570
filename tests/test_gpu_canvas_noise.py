"""Canvas-keyed DDIM noise on the MI355X (include/avdiff_hip.h, "canvas-keyed noise"): avd_canvas_noise_f32 against the gather of the
per-sample stream bit for bit and against the numpy mirror, the fused canvas-keyed step against the unseeded step fed the same noise
explicitly (both targets, both video kernel forms, cond-only, CFG control, latent guide), the step under window consensus, graph replay
against eager launches, an eta > 0 consensus trajectory against the CPU oracle, stream_generate at ddim_eta > 0 under consensus for any
batching, and the refusals."""
from functools import partial

import numpy as np
import pytest
import torch

import _canvas_noise_ref as CN
import _consensus_ref as W
from _kit import (ABAR, STREAM_HALF_SECOND, audio_case, audio_prompt, components, dev, engine, matmul_f32, model,  # noqa: F401  (dev / model are fixtures)
                  pipeline, ts, video_case, video_prompt)
from _tune import cfg_rows  # noqa: F401  (fixture)
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
SEED = 0xDEADBEEF12345678           # both key words non-zero
ETA, G = 0.5, 3.0
_engine = partial(engine, guidance=G)        # engine(mods, target, shape, n_prompt, **kw) at this file's guidance


def _canvas_engine(model, target, shape, n_prompt, hop, **kw):
    return _engine(model[1], target, shape, n_prompt, eta=ETA, noise_seed=SEED, noise_keying="canvas", canvas_hop=hop, **kw)


# ------------------------------------------------------------------------------------------------- the noise kernel
KERNEL_CASES = [
    ("video inner % 4 == 0", (5, 8, 6, 16, 16), 2),
    ("video inner 15", (4, 3, 6, 3, 5), 2),
    ("video inner % 4 == 2", (3, 2, 5, 3, 6), 1),
    ("audio hop 50", (4, 8, 150), 50),
    ("audio hop 75", (4, 8, 150), 75),
    ("audio L not divisible by hop", (6, 3, 37), 5),
    ("hop >= L", (4, 8, 30), 31),
    ("N == 1 video", (1, 8, 6, 4, 4), 2),
    ("N == 1 audio", (1, 8, 30), 7),
]


@pytest.mark.parametrize("name,shape,hop", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_kernel_is_the_gather_of_the_per_sample_stream(dev, name, shape, hop):
    from multimodal_diffusion_amd import functional as Fn
    N = shape[0]
    outer, L_, inner = W.dims(shape)
    P = (N - 1) * hop + L_
    t = 731
    got = Fn.canvas_noise(SEED, ts([t] * N, dev), shape, hop)
    assert tuple(got.shape) == shape and got.dtype == torch.float32
    draw = Fn.gaussian_noise(SEED, 0, ts([t] * P, dev), (P, outer, inner)).cpu().numpy().reshape(P, outer * inner)
    ref = CN.gather_windows(draw, shape, hop)
    gn = got.cpu().numpy()
    assert np.array_equal(gn, ref)                                           # bit for bit
    assert W.overlaps_agree(gn, hop)
    # the numpy mirror, at the tolerance of test_gpu_seeded_noise.py::test_generator_matches_reference
    mirror = CN.canvas_normals(SEED, [t] * N, shape, hop)
    err = np.abs(gn.astype(np.float64) - mirror).max()
    assert err < 1e-5, err
    # an unaligned base address takes the per-element kernel: the same bits
    buf = torch.empty(int(np.prod(shape)) + 1, device=dev)
    zu = buf[1:].view(shape)
    assert zu.data_ptr() % 16 != 0
    assert Fn.canvas_noise(SEED, ts([t] * N, dev), shape, hop, out=zu) is zu
    assert np.array_equal(zu.cpu().numpy(), ref)
    # windows [lo, N) with window_offset = lo are that slice of the full batch
    for lo in {N // 2, N - 1}:
        part = Fn.canvas_noise(SEED, ts([t] * (N - lo), dev), (N - lo,) + shape[1:], hop, window_offset=lo)
        assert np.array_equal(part.cpu().numpy(), ref[lo:])
    # per-window timesteps that differ: window b is rows (b*hop .. b*hop + L - 1) of the per-sample stream at t_now[b]
    tn = [999 - 37 * b for b in range(N)]
    per_t = Fn.canvas_noise(SEED, ts(tn, dev), shape, hop).cpu().numpy()
    for b in range(N):
        rows = Fn.gaussian_noise(SEED, b * hop, ts([tn[b]] * L_, dev), (L_, outer, inner)).cpu().numpy().reshape(L_, outer * inner)
        assert np.array_equal(per_t[b:b + 1], CN.gather_windows(rows, (1,) + shape[1:], hop))
    assert np.abs(per_t.astype(np.float64) - CN.canvas_normals(SEED, tn, shape, hop)).max() < 1e-5
    if N > 1:
        assert not np.array_equal(per_t[1], gn[1])


def test_kernel_far_window_offset(dev):
    """canvas positions next to 2^32: the position is computed in 64 bits and keyed by its low word"""
    from multimodal_diffusion_amd import functional as Fn
    shape, hop = (2, 8, 6, 4, 4), 3
    off = (2 ** 32 - 6 - hop) // hop                                         # the last position is <= 2^32 - 1
    got = Fn.canvas_noise(7, ts([5, 5], dev), shape, hop, window_offset=off).cpu().numpy()
    rows = Fn.gaussian_noise(7, off * hop, ts([5] * 9, dev), (9, 8, 16)).cpu().numpy().reshape(9, 128)
    assert np.array_equal(got, CN.gather_windows(rows, shape, hop))
    with pytest.raises(ValueError):
        Fn.canvas_noise(7, ts([5, 5], dev), shape, hop, window_offset=off + 2)


# ------------------------------------------------------------------------------------------------- fused step = explicit noise
@pytest.mark.parametrize("cond_only", [False, True])
@pytest.mark.parametrize("rows", [1, 0])
def test_fused_step_equals_explicit_noise_video(dev, model, cfg_rows, rows, cond_only):
    from multimodal_diffusion_amd import functional as Fn
    cfg_rows(rows)
    z, za, npr = video_case(dev, B=3, W=16)
    tn, tp = ts([981, 402, 40], dev), ts([961, 382, -1], dev)
    hop, off = 2, 5
    canvas = _canvas_engine(model, "video", tuple(z.shape), npr, hop, sample_offset=off)
    plain = _engine(model[1], "video", tuple(z.shape), npr, eta=ETA)
    for e in (canvas, plain):
        e.set_prompt(za)
    a = canvas.step(z, tn, tp, cond_only=cond_only)
    b = plain.step(z, tn, tp, noise=Fn.canvas_noise(SEED, tn, tuple(z.shape), hop, window_offset=off), cond_only=cond_only)
    assert torch.equal(a, b)
    c = plain.step(z, tn, tp, noise=Fn.gaussian_noise(SEED, off, tn, tuple(z.shape)), cond_only=cond_only)
    assert not torch.equal(a, c)                              # not the per-sample keying


def test_fused_step_equals_explicit_noise_video_wide_rows(dev, model):
    """W = 32: the whole-line kernel with eight tokens per block (W = 16 above takes four)"""
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(2)
    z, za = torch.randn(2, 8, 4, 16, 32, generator=g).to(dev), torch.randn(2, 8, 40, generator=g).to(dev)
    tn, tp = ts([700, 300], dev), ts([680, 280], dev)
    canvas = _canvas_engine(model, "video", tuple(z.shape), 10, 3, sample_offset=1)
    plain = _engine(model[1], "video", tuple(z.shape), 10, eta=ETA)
    for e in (canvas, plain):
        e.set_prompt(za)
    noise = Fn.canvas_noise(SEED, tn, tuple(z.shape), 3, window_offset=1)
    assert torch.equal(canvas.step(z, tn, tp), plain.step(z, tn, tp, noise=noise))


@pytest.mark.parametrize("cond_only", [False, True])
def test_fused_step_equals_explicit_noise_audio(dev, model, cond_only):
    from multimodal_diffusion_amd import functional as Fn
    z, zv, npr = audio_case(dev, B=3, L=150)
    tn, tp = ts([981, 402, 40], dev), ts([961, 382, -1], dev)
    hop, off = 75, 11
    canvas = _canvas_engine(model, "audio", tuple(z.shape), npr, hop, sample_offset=off)
    plain = _engine(model[1], "audio", tuple(z.shape), npr, eta=ETA)
    for e in (canvas, plain):
        e.set_prompt(zv)
    a = canvas.step(z, tn, tp, cond_only=cond_only)
    b = plain.step(z, tn, tp, noise=Fn.canvas_noise(SEED, tn, tuple(z.shape), hop, window_offset=off), cond_only=cond_only)
    assert torch.equal(a, b)


@pytest.mark.parametrize("rows", [1, 0])
def test_fused_controlled_step_equals_composed(dev, model, cfg_rows, rows):
    """Per-sample guidance plus rescale.  An unseeded engine takes no CFG control at eta > 0, so the reference is composed from the
    elementwise entries on the step's own eps tokens: combine with g_b, r(y) with the s_b the statistics pass left in the scratch (U
    is a permutation for video, r is elementwise), un-patch, then avd_ddim_step_f32 on the explicit canvas noise.  Bit for bit."""
    from multimodal_diffusion_amd import functional as Fn
    cfg_rows(rows)
    z, za, npr = video_case(dev, B=3, W=16)
    B = z.shape[0]
    g, phi = [2.0, 3.5, 5.0], [0.7, 0.3, 1.0]
    tn, tp = ts([981, 402, 40], dev), ts([961, 382, 20], dev)
    hop = 2
    eng = _canvas_engine(model, "video", tuple(z.shape), npr, hop, guidance=g, guidance_rescale=phi)
    eng.set_prompt(za)
    out = eng.step(z, tn, tp)
    ep = eng.eps_tokens()
    ec, en = ep[:B], ep[B:]
    nb = eng._cfg_stats.numel()
    off = nb - ((4 * B + 15) // 16) * 16                      # the scale slot ends the scratch (functional.cfg_rescale)
    s = eng._cfg_stats[off:off + 4 * B].view(torch.float32).view(B, 1, 1)
    gt, ph = torch.tensor(g, device=dev).view(B, 1, 1), torch.tensor(phi, device=dev).view(B, 1, 1)
    y = en + gt * (ec - en)
    r = torch.where(ph == 1.0, y * s, ph * (y * s) + (1.0 - ph) * y)
    eps = Fn.tube_unpatch(r.contiguous(), *z.shape[1:], 2, 4, 4)
    ref = Fn.ddim_step(z, tn, tp, eps, ABAR, eta=ETA, noise=Fn.canvas_noise(SEED, tn, tuple(z.shape), hop))
    assert torch.equal(out, ref)
    # the control is live, and so is the keying
    plain = _canvas_engine(model, "video", tuple(z.shape), npr, hop)
    plain.set_prompt(za)
    assert not torch.equal(plain.step(z, tn, tp), out)
    sample = _engine(model[1], "video", tuple(z.shape), npr, guidance=g, guidance_rescale=phi, eta=ETA, noise_seed=SEED)
    sample.set_prompt(za)
    assert not torch.equal(sample.step(z, tn, tp), out)


@pytest.mark.parametrize("cond_only", [False, True])
def test_fused_guided_step_equals_composed(dev, model, cond_only):
    """A frame-masked latent guide: the seeded guided step's arithmetic, avd_eps_unpatch_ddim_f32 fed the explicit canvas noise followed
    by Fn.latent_guide (whose known-noise stream stays keyed per sample)."""
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd.sampler import frame_mask
    z, za, npr = video_case(dev, B=3, W=16)
    B = z.shape[0]
    known = torch.randn(z.shape, generator=torch.Generator().manual_seed(4)).to(dev)
    mask = frame_mask(tuple(z.shape[1:]), 0, 2).to(dev)
    tn, tp = ts([981, 402, 40], dev), ts([961, 382, -1], dev)
    hop, off, gseed = 2, 3, 77
    eng = _canvas_engine(model, "video", tuple(z.shape), npr, hop, sample_offset=off)
    eng.set_prompt(za)
    eng.set_known(known, mask, guide_seed=gseed)
    out = eng.step(z, tn, tp, cond_only=cond_only)
    ep = eng.eps_tokens()
    eps = ep if cond_only else (ep[B:] + G * (ep[:B] - ep[B:])).contiguous()
    noise = Fn.canvas_noise(SEED, tn, tuple(z.shape), hop, window_offset=off)
    stepped = torch.empty_like(z)
    L.check(L.lib().avd_eps_unpatch_ddim_f32(eps.data_ptr(), z.data_ptr(), tn.data_ptr(), tp.data_ptr(), eng.alpha_bar.data_ptr(),
                                             eng.alpha_bar.numel(), ETA, noise.data_ptr(), stepped.data_ptr(), *z.shape, 2, 4, 4,
                                             None, None, None, None, L.stream_ptr(dev)))
    ref = Fn.latent_guide(known, tp, ABAR, z=stepped, mask=mask, seed=gseed, sample_offset=off)
    assert torch.equal(out, ref)
    assert torch.equal(out[2, :, :2], known[2, :, :2]) and not torch.equal(out, stepped)       # t_prev = -1 returns the known frames


# ------------------------------------------------------------------------------------------------- with the consensus set
@pytest.mark.parametrize("target", ["video", "audio"])
def test_step_with_consensus_is_consensus_of_step(dev, model, target):
    from multimodal_diffusion_amd import functional as Fn
    if target == "video":
        z, zp, npr = video_case(dev, B=3, W=16)
        hop = 2
    else:
        z, zp, npr = audio_case(dev, B=3, L=150)
        hop = 50
    L_ = W.dims(tuple(z.shape))[1]
    tn, tp = ts([900] * 3, dev), ts([700] * 3, dev)
    eng = _canvas_engine(model, target, tuple(z.shape), npr, hop)
    eng.set_prompt(zp)
    free = eng.step(z, tn, tp)
    for weights in (None, torch.linspace(0.5, 2.0, L_)):
        eng.set_window_consensus(hop, weights)
        got = eng.step(z, tn, tp)
        assert torch.equal(got, Fn.window_consensus(free.clone(), hop, weights))
        assert W.overlaps_agree(got.cpu().numpy(), hop) and not torch.equal(got, free)
    eng.clear_window_consensus()
    assert torch.equal(eng.step(z, tn, tp), free)


# ------------------------------------------------------------------------------------------------- graph = eager
@pytest.mark.parametrize("interval", [None, "split"])
def test_graph_equals_eager(dev, model, interval):
    z, za, npr = video_case(dev, B=3, W=16)
    sched = R.sampling_schedule(1000, 6)
    iv = None if interval is None else (int(sched[4]), int(sched[1]))          # steps 1 .. 4 are CFG steps, 0 and 5 cond-only
    hop = 2
    eng = _canvas_engine(model, "video", tuple(z.shape), npr, hop, guidance_interval=iv)
    eng.set_prompt(za)
    eng.set_window_consensus(hop)
    zg = eng.run(z, sched, graph=True)
    ze = eng.run(z, sched, graph=False)
    assert torch.equal(zg, ze)
    assert W.overlaps_agree(zg.cpu().numpy(), hop)
    if iv is not None:
        eng.set_guidance_interval(None)
        assert not torch.equal(eng.run(z, sched, graph=False), ze)


# ------------------------------------------------------------------------------------------------- trajectory vs the oracle
def test_consensus_trajectory_vs_oracle(dev, model):
    """5 steps at eta = 0.5 with the consensus set, against the CPU oracle's DDIM step fed the mirror's noise followed by the consensus
    mirror; the gate of test_gpu_seeded_noise.py::test_seeded_trajectory_vs_oracle."""
    ws, _ = model
    n_steps, hop, off = 5, 2, 3
    sched = R.sampling_schedule(1000, n_steps)
    z, zp, npr = video_case(dev, B=3, W=16)
    wts = np.linspace(0.5, 2.0, 4).astype(np.float32)
    eng = _canvas_engine(model, "video", tuple(z.shape), npr, hop, sample_offset=off)
    eng.set_prompt(zp)
    eng.set_window_consensus(hop, torch.from_numpy(wts))
    out = eng.run(z, sched).cpu().double()
    x, p = z.cpu(), zp.cpu()
    kw = dict(adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"], head=ws["head"], n_layers=2, n_heads=8, guidance=G,
              eta=0.0, return_eps=True)
    for i in range(len(sched) - 1):
        tn, tp = sched[i].repeat(3), sched[i + 1].repeat(3)
        _, eps_tok = R.denoise_step_a2v(x, p, tn, tp, ABAR, **kw)
        eps = R.tube_unpatch(eps_tok, *x.shape[1:], 2, 4, 4)
        noise = torch.from_numpy(CN.canvas_normals(SEED, tn.numpy(), tuple(x.shape), hop, window_offset=off).astype(np.float32))
        x = R.ddim_update(x, tn, tp, eps, ABAR, eta=ETA, noise=noise)
        x = torch.from_numpy(W.consensus_f32(x.numpy(), hop, wts))
    ref = x.double()
    err = float((out - ref).norm() / ref.norm())
    print(f"canvas consensus trajectory vs oracle: relative error {err:.3e}")
    assert err < 1e-3


# ------------------------------------------------------------------------------------------------- stream_generate
@pytest.fixture
def stream(dev, model):
    """(kw, cfg): the geometry of test_gpu_window_consensus.py's stream tests (0.5 s windows every 0.25 s, 32 x 32 frames, a 4-step
    schedule) with ddim_eta = 0.5; the fp32 kernel family whatever the batch, so that batch sizes can be compared"""
    with matmul_f32(model[1]):
        vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND, sampling={"ddim_eta": 0.5})
        yield dict(components(model[1], vae, codec, dev), cfg=cfg, shard=False), cfg


def test_stream_generate_stochastic_consensus(dev, stream):
    from multimodal_diffusion_amd import stream_infer as S
    kw, cfg = stream
    kws = dict(kw, consensus="uniform", noise_seed=3, noise_keying="canvas", return_latents=True, **audio_prompt())
    hop, L_ = S.latent_hop(cfg, "video")
    assert (hop, L_) == (1, 2)
    whole = S.stream_generate(**kws)
    lat = whole["latents"]
    assert lat.shape == (4, 8, 2, 4, 4) and np.isfinite(lat).all()
    assert W.overlaps_agree(lat, hop)                                          # one coherent latent clip at eta > 0
    # max_windows_per_batch 32: one engine again (a second run repeats bit for bit); 2: lock-step engines with sample_offset = lo
    for mw in (32, 2):
        part = S.stream_generate(max_windows_per_batch=mw, **kws)
        assert np.array_equal(part["latents"], lat) and np.array_equal(part["video"], whole["video"])
    det = S.stream_generate(**dict(kws, cfg=dict(cfg, sampling=dict(cfg["sampling"], ddim_eta=0.0))))
    assert W.overlaps_agree(det["latents"], hop) and not np.array_equal(det["latents"], lat)       # the noise is live
    other = S.stream_generate(**dict(kws, noise_seed=4))
    assert not np.array_equal(other["latents"], lat)
    by_cfg = S.stream_generate(**dict(kws, noise_keying=None, cfg=dict(cfg, streaming=dict(cfg["streaming"], noise_keying="canvas"))))
    assert np.array_equal(by_cfg["latents"], lat)
    with pytest.raises(ValueError, match="halo"):
        S.stream_generate(**dict(kws, shard=True))
    with pytest.raises(ValueError, match="ddim_eta"):
        S.stream_generate(**dict(kws, noise_keying="sample"))
    with pytest.raises(ValueError, match="consensus"):
        S.stream_generate(**dict(kws, consensus=None))
    with pytest.raises(ValueError, match="noise_seed"):
        S.stream_generate(**dict(kws, noise_seed=None))


def test_stream_generate_video_prompt_direction(dev, stream):
    from multimodal_diffusion_amd import stream_infer as S
    kw, cfg = stream
    kws = dict(kw, consensus="uniform", noise_seed=3, noise_keying="canvas", return_latents=True, **video_prompt())
    assert S.latent_hop(cfg, "audio") == (75, 150)
    whole = S.stream_generate(**kws)
    assert whole["latents"].shape == (4, 8, 150) and W.overlaps_agree(whole["latents"], 75)
    part = S.stream_generate(max_windows_per_batch=2, **kws)
    assert np.array_equal(part["latents"], whole["latents"]) and np.array_equal(part["audio"], whole["audio"])


# ------------------------------------------------------------------------------------------------- misuse, and nothing else moved
def test_engine_misuse(dev, model):
    z, za, npr = video_case(dev, B=3, W=16)
    shape = tuple(z.shape)
    with pytest.raises(ValueError, match="noise_seed"):
        _engine(model[1], "video", shape, npr, eta=ETA, noise_keying="canvas", canvas_hop=2)
    with pytest.raises(ValueError, match="canvas_hop"):
        _engine(model[1], "video", shape, npr, eta=ETA, noise_seed=1, noise_keying="canvas")
    for bad in (0, -1, 1.5, True):
        with pytest.raises(ValueError):
            _engine(model[1], "video", shape, npr, eta=ETA, noise_seed=1, noise_keying="canvas", canvas_hop=bad)
    with pytest.raises(ValueError):
        _engine(model[1], "video", shape, npr, eta=ETA, noise_seed=1, noise_keying="position", canvas_hop=2)
    with pytest.raises(ValueError):
        _engine(model[1], "video", shape, npr, eta=ETA, noise_seed=1, canvas_hop=2)                  # canvas_hop without the keying
    with pytest.raises(ValueError):                                                                 # (2^32 - 2 + 2)*2 + 4 > 2^32
        _engine(model[1], "video", shape, npr, eta=ETA, noise_seed=1, noise_keying="canvas", canvas_hop=2, sample_offset=2 ** 32 - 2)
    eng = _canvas_engine(model, "video", shape, npr, 2)
    eng.set_prompt(za)
    gen = eng._generation
    with pytest.raises(ValueError, match="canvas_hop"):
        eng.set_window_consensus(3)
    assert eng._cons_hop is None and eng._generation == gen
    tn, tp = ts([900] * 3, dev), ts([700] * 3, dev)
    with pytest.raises(ValueError):
        eng.step(z, tn, tp, noise=torch.randn_like(z))
    # the sample-keyed engine keeps today's refusal, naming the option
    with pytest.raises(ValueError, match="eta.*noise_keying='canvas'"):
        _engine(model[1], "video", shape, npr, eta=ETA, noise_seed=1).set_window_consensus(2)


def test_default_engines_keep_their_bits(dev, model):
    """Nothing else moved: at eta == 0 a canvas-keyed engine is the plain engine, and a default (sample-keyed) seeded engine at eta > 0
    still draws the per-sample stream — each compared through the pre-existing entries."""
    from multimodal_diffusion_amd import functional as Fn
    z, za, npr = video_case(dev, B=3, W=16)
    shape = tuple(z.shape)
    tn, tp = ts([900, 100, 500], dev), ts([880, 80, 480], dev)
    canvas0 = _engine(model[1], "video", shape, npr, eta=0.0, noise_seed=SEED, noise_keying="canvas", canvas_hop=2)
    plain0 = _engine(model[1], "video", shape, npr, eta=0.0)
    seeded = _engine(model[1], "video", shape, npr, eta=ETA, noise_seed=SEED, sample_offset=5)
    plain = _engine(model[1], "video", shape, npr, eta=ETA)
    for e in (canvas0, plain0, seeded, plain):
        e.set_prompt(za)
    assert torch.equal(canvas0.step(z, tn, tp), plain0.step(z, tn, tp))
    assert torch.equal(canvas0.step(z, tn, tp, cond_only=True), plain0.step(z, tn, tp, cond_only=True))
    canvas0.set_window_consensus(3)                           # eta == 0: any hop, as on every engine
    assert torch.equal(canvas0.step(z, tn, tp), Fn.window_consensus(plain0.step(z, tn, tp), 3))
    assert seeded.noise_keying == "sample" and seeded.canvas_hop is None
    assert torch.equal(seeded.step(z, tn, tp), plain.step(z, tn, tp, noise=Fn.gaussian_noise(SEED, 5, tn, shape)))
