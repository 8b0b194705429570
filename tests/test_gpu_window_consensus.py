"""Latent window consensus on the MI355X (include/avdiff_hip.h, avd_window_consensus_f32): the kernel against the numpy mirror bit for
bit, the engine's consensus step against the plain step followed by the functional call, graph replay against eager launches, and
stream_generate: the finished latents agree on every overlap, whatever the batching, and equal a hand-written loop; off by default."""
from functools import partial

import numpy as np
import pytest
import torch

import _consensus_ref as W
from _kit import (STREAM_HALF_SECOND, audio_prompt, components, dev, engine, matmul_f32, model,  # noqa: F401  (dev / model are fixtures)
                  pipeline, ts, video_case, video_prompt, with_sampling)
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
G = 3.0
_engine = partial(engine, guidance=G)        # engine(mods, target, shape, n_prompt, **kw) at this file's guidance


# ------------------------------------------------------------------------------------------------- kernel = mirror, bit for bit
KERNEL_CASES = [
    ("video three-fold", (5, 8, 6, 16, 16), 2, False),
    ("video weights", (5, 8, 6, 16, 16), 2, True),
    ("audio hop 75", (4, 8, 150), 75, False),
    ("audio hop 50", (4, 8, 150), 50, False),
    ("audio weights", (4, 8, 150), 50, True),
    ("hop == L", (4, 8, 6, 4, 4), 6, False),
    ("hop > L", (4, 8, 30), 31, True),
    ("N == 1", (1, 8, 6, 4, 4), 2, True),
    ("odd inner", (4, 3, 6, 3, 5), 2, True),
    ("inner % 4 == 2", (3, 2, 5, 3, 6), 1, False),
    ("L not divisible by hop", (5, 4, 7, 4, 4), 3, True),
    ("audio L not divisible by hop", (6, 3, 37), 5, True),
]


@pytest.mark.parametrize("name,shape,hop,weighted", KERNEL_CASES, ids=[c[0] for c in KERNEL_CASES])
def test_kernel_matches_mirror_bit_for_bit(dev, name, shape, hop, weighted):
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(len(name) + hop)
    z = torch.randn(*shape, generator=g)
    w = (0.25 + 1.5 * torch.rand(W.dims(shape)[1], generator=g)) if weighted else None
    ref = W.consensus_f32(z.numpy(), hop, None if w is None else w.numpy())
    zd = z.to(dev)
    out = Fn.window_consensus(zd, hop, w)
    assert out is zd                                           # in place
    got = zd.cpu().numpy()
    assert np.array_equal(got, ref)
    if shape[0] == 1 or hop >= W.dims(shape)[1]:
        assert got.tobytes() == z.numpy().tobytes()            # nothing to agree on: unchanged
    else:
        assert W.overlaps_agree(got, hop) and not np.array_equal(got, z.numpy())
    # an unaligned base address takes the scalar kernel: the same bits
    buf = torch.empty(z.numel() + 1, device=dev)
    zu = buf[1:].view(shape)
    zu.copy_(z)
    assert np.array_equal(Fn.window_consensus(zu, hop, w).cpu().numpy(), ref)


def test_functional_misuse(dev):
    from multimodal_diffusion_amd import functional as Fn
    z = torch.zeros(3, 2, 8, device=dev)
    for hop in (0, -1):
        with pytest.raises(ValueError):
            Fn.window_consensus(z, hop)
    with pytest.raises(ValueError):
        Fn.window_consensus(z, 4, torch.ones(7))
    with pytest.raises(ValueError):
        Fn.window_consensus(z, 4, torch.zeros(8))
    with pytest.raises(ValueError):
        Fn.window_consensus(torch.zeros(3, 2, 8, 4, device=dev), 4)
    with pytest.raises(TypeError):
        Fn.window_consensus(torch.zeros(3, 8, 2, device=dev).transpose(1, 2), 4)     # in place needs a contiguous tensor


# ------------------------------------------------------------------------------------------------- engine
@pytest.mark.parametrize("solver,cond_only", [("ddim", False), ("dpmpp_2m", False), ("ddim", True), ("dpmpp_2m", True)])
def test_engine_step_is_step_then_consensus(dev, model, solver, cond_only):
    from multimodal_diffusion_amd import functional as Fn
    z, za, npr = video_case(dev, B=3, W=16)
    w = torch.linspace(0.5, 2.0, 4)
    tn, tp, tl = ts([900] * 3, dev), ts([700] * 3, dev), ts([950] * 3, dev)
    eng = _engine(model[1], "video", tuple(z.shape), npr, solver=solver)
    eng.set_prompt(za)
    hist = torch.randn(z.shape, generator=torch.Generator().manual_seed(3)).to(dev)

    def step():
        kw = {}
        if solver == "dpmpp_2m":
            eng.x0_hist.copy_(hist)
            kw["t_last"] = tl
        return eng.step(z, tn, tp, cond_only=cond_only, **kw)

    plain = step()
    x0_plain = None if eng.x0_hist is None else eng.x0_hist.clone()
    for hop, weights in ((2, None), (1, w)):
        eng.set_window_consensus(hop, weights)
        got = step()
        assert torch.equal(got, Fn.window_consensus(plain.clone(), hop, weights))
        assert W.overlaps_agree(got.cpu().numpy(), hop) and not torch.equal(got, plain)
        if x0_plain is not None:
            assert torch.equal(eng.x0_hist, x0_plain)          # the history stays per window
    eng.clear_window_consensus()
    assert torch.equal(step(), plain)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_graph_equals_eager_and_stale_pairs_are_refused(dev, model, solver):
    from multimodal_diffusion_amd import _lib as L
    z, za, npr = video_case(dev, B=3, W=16)
    sched = R.sampling_schedule(1000, 5)
    eng = _engine(model[1], "video", tuple(z.shape), npr, solver=solver)
    eng.set_prompt(za)
    free = eng.run(z, sched, graph=False)
    # a pair captured before the consensus is switched on holds no consensus launch: it refuses to replay afterwards
    eng.begin(sched)
    a, b = z.clone(), torch.empty_like(z)
    eng.advance(a, b)
    pair = eng.capture_pair(a, b)
    eng.set_window_consensus(2)
    with pytest.raises(L.AvdError, match="window consensus"):
        pair.replay()
    zg = eng.run(z, sched, graph=True)
    ze = eng.run(z, sched, graph=False)
    assert torch.equal(zg, ze)
    assert W.overlaps_agree(zg.cpu().numpy(), 2) and not torch.equal(zg, free)
    # a pair captured with the consensus follows new weights (engine-owned table) and goes stale with a new hop or when it is cleared
    eng.begin(sched)
    eng.advance(a.copy_(z), b)
    pair = eng.capture_pair(a, b)
    eng.set_window_consensus(2, torch.linspace(1.0, 2.0, 4))
    pair.replay()
    eng.set_window_consensus(1)
    with pytest.raises(L.AvdError, match="window consensus"):
        pair.replay()
    eng.clear_window_consensus()
    assert torch.equal(eng.run(z, sched, graph=True), free)


def test_engine_misuse(dev, model):
    z, za, npr = video_case(dev, B=3, W=16)
    noisy = _engine(model[1], "video", tuple(z.shape), npr, eta=0.5, noise_seed=1)
    with pytest.raises(ValueError, match="eta"):
        noisy.set_window_consensus(2)
    eng = _engine(model[1], "video", tuple(z.shape), npr)
    for hop in (0, -2, 1.5):
        with pytest.raises(ValueError):
            eng.set_window_consensus(hop)
    with pytest.raises(ValueError):
        eng.set_window_consensus(2, torch.ones(3))             # L is 4
    with pytest.raises(ValueError):
        eng.set_window_consensus(2, torch.tensor([1.0, 0.0, 1.0, 1.0]))
    assert eng._cons_hop is None and eng._generation == _engine(model[1], "video", tuple(z.shape), npr)._generation


# ------------------------------------------------------------------------------------------------- stream_generate
@pytest.fixture
def stream(dev, model):
    """(kw, cfg) for stream_generate at the geometry of test_gpu_dpm_solver.py::test_stream_generate_batch_invariance: 0.5 s windows
    every 0.25 s, 32 x 32 frames, a 4-step schedule; the fp32 kernel family whatever the batch, so that batch sizes can be compared"""
    with matmul_f32(model[1]):
        vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND)
        yield dict(components(model[1], vae, codec, dev), cfg=cfg, shard=False), cfg


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_stream_latents_agree_on_overlaps_for_any_batching(dev, stream, solver):
    from multimodal_diffusion_amd import stream_infer as S
    kw, cfg = stream
    kw = dict(kw, cfg=with_sampling(cfg, solver=solver), **audio_prompt())
    hop, L_ = S.latent_hop(kw["cfg"], "video")
    assert (hop, L_) == (1, 2)
    whole = S.stream_generate(consensus="uniform", return_latents=True, **kw)
    lat = whole["latents"]
    assert lat.shape == (4, 8, 2, 4, 4) and lat.dtype == np.float32
    assert W.overlaps_agree(lat, hop)                                          # the feature: one coherent latent clip
    canvas = S.canvas_from_windows(torch.from_numpy(lat), hop)
    assert tuple(canvas.shape) == (8, 5, 4, 4) and np.array_equal(S.windows_from_canvas(canvas, L_, hop).numpy(), lat)
    free = S.stream_generate(return_latents=True, **kw)
    assert free["latents"].shape == lat.shape and not W.overlaps_agree(free["latents"], hop)     # independent windows do not
    assert not np.array_equal(free["video"], whole["video"])
    for mw in (2, 1):                                                          # lock-step engines, one consensus pass per step
        part = S.stream_generate(consensus="uniform", return_latents=True, max_windows_per_batch=mw, **kw)
        assert np.array_equal(part["latents"], lat) and np.array_equal(part["video"], whole["video"])
    # "uniform" is the all-ones table; the config key switches it on as well, and the argument wins over it
    ones = S.stream_generate(consensus=np.ones(L_, dtype=np.float32), return_latents=True, **kw)
    assert np.array_equal(ones["latents"], lat)
    by_cfg = S.stream_generate(return_latents=True, **dict(kw, cfg=dict(kw["cfg"], streaming=dict(cfg["streaming"], latent_consensus="uniform"))))
    assert np.array_equal(by_cfg["latents"], lat)
    weighted = S.stream_generate(consensus=[1.0, 3.0], return_latents=True, **kw)
    assert W.overlaps_agree(weighted["latents"], hop) and not np.array_equal(weighted["latents"], lat)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_stream_equals_hand_written_loop(dev, model, stream, solver):
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd import schedule_utils as su
    from multimodal_diffusion_amd import stream_infer as S
    kw, cfg = stream
    kw = dict(kw, cfg=with_sampling(cfg, solver=solver), **audio_prompt())
    got = S.stream_generate(consensus="uniform", return_latents=True, **kw)["latents"]
    # the same trajectory by hand: the prompt windows, the seeded canvas cropped into windows, one engine, and after every step the
    # functional consensus
    chunks, _, _ = S.split_audio_into_windows(kw["prompt_audio"], sr=16000, win_s=0.5, hop_s=0.25)
    z_p = kw["aud_codec"].encode(torch.from_numpy(np.ascontiguousarray(chunks, dtype=np.float32)).to(dev)[:, None, :])
    canvas = torch.randn(8, 5, 4, 4, generator=torch.Generator().manual_seed(10))
    z = S.windows_from_canvas(canvas, 2, 1).to(dev)
    c = cfg["diffusion"]["video"]
    abar = su.alphas_cumprod_from_betas(su.make_beta_schedule(1000, kind=c["schedule"], min_beta=c["min_beta"], max_beta=c["max_beta"]))[1]
    sched = su.make_sampling_schedule(1000, 4)
    eng = engine(model[1], "video", tuple(z.shape), (150 - 4) // 4 + 1, alpha_bar=abar, guidance=2.0, solver=solver)
    eng.set_prompt(z_p.float().contiguous())
    for i in range(sched.numel() - 1):
        kws = {}
        if solver == "dpmpp_2m" and i > 0:
            kws["t_last"] = ts([int(sched[i - 1])] * 4, dev)
        z = eng.step(z, ts([int(sched[i])] * 4, dev), ts([int(sched[i + 1])] * 4, dev), **kws)
        Fn.window_consensus(z, 1)
    assert np.array_equal(z.cpu().numpy(), got)


def test_stream_guidance_interval_keeps_batch_invariance(dev, stream):
    from multimodal_diffusion_amd import schedule_utils as su
    from multimodal_diffusion_amd import stream_infer as S
    kw, cfg = stream
    sched = su.make_sampling_schedule(1000, 4)
    interval = (int(sched[2]), int(sched[1]))                                   # steps 1 and 2 are CFG steps, 0 and 3 cond-only
    kinds = [c for _, _, c in su.guidance_segments(sched, interval)]
    assert kinds == [False, True, False]
    for solver in ("ddim", "dpmpp_2m"):
        kws = dict(kw, cfg=with_sampling(cfg, solver=solver), guidance_interval=interval, consensus="uniform", return_latents=True,
                   **audio_prompt())
        whole = S.stream_generate(**kws)
        assert W.overlaps_agree(whole["latents"], 1)
        for mw in (2, 1):
            part = S.stream_generate(max_windows_per_batch=mw, **kws)
            assert np.array_equal(part["latents"], whole["latents"]) and np.array_equal(part["video"], whole["video"])
        every = S.stream_generate(**dict(kws, guidance_interval=None))
        assert not np.array_equal(every["latents"], whole["latents"])           # the interval is live


def test_stream_video_prompt_direction(dev, stream):
    from multimodal_diffusion_amd import stream_infer as S
    kw, cfg = stream
    for solver in ("ddim", "dpmpp_2m"):
        kws = dict(kw, cfg=with_sampling(cfg, solver=solver), **video_prompt())
        assert S.latent_hop(kws["cfg"], "audio") == (75, 150)
        whole = S.stream_generate(consensus="uniform", return_latents=True, **kws)
        assert whole["latents"].shape == (4, 8, 150) and W.overlaps_agree(whole["latents"], 75)
        assert not W.overlaps_agree(S.stream_generate(return_latents=True, **kws)["latents"], 75)
        for mw in (2, 1):
            part = S.stream_generate(consensus="uniform", return_latents=True, max_windows_per_batch=mw, **kws)
            assert np.array_equal(part["latents"], whole["latents"]) and np.array_equal(part["audio"], whole["audio"])


def test_stream_off_by_default_and_single_window(dev, stream):
    from multimodal_diffusion_amd import stream_infer as S
    kw, cfg = stream
    kws = dict(kw, **audio_prompt())
    today = S.stream_generate(**kws)
    assert set(today) == {"video", "fps"}
    off = S.stream_generate(consensus=None, return_latents=True, **kws)
    assert np.array_equal(off["video"], today["video"])
    # one window has nothing to agree with: the same output with and without
    one = dict(kw, **audio_prompt(8000))
    a = S.stream_generate(return_latents=True, **one)
    b = S.stream_generate(consensus="uniform", return_latents=True, **one)
    assert a["latents"].shape == (1, 8, 2, 4, 4)
    assert np.array_equal(a["latents"], b["latents"]) and np.array_equal(a["video"], b["video"])


def test_stream_misuse(dev, stream):
    from multimodal_diffusion_amd import stream_infer as S
    kw, cfg = stream
    kws = dict(kw, **audio_prompt())
    with pytest.raises(ValueError, match="halo"):
        S.stream_generate(consensus="uniform", **dict(kws, shard=True))
    with pytest.raises(ValueError, match="ddim_eta"):
        S.stream_generate(consensus="uniform", noise_seed=3, **dict(kws, cfg=with_sampling(cfg, solver="ddim", ddim_eta=0.5)))
    misaligned = dict(cfg, streaming=dict(cfg["streaming"], hop_seconds=0.125))              # 2 frames per hop, t_down 4
    with pytest.raises(ValueError, match="t_down"):
        S.stream_generate(consensus="uniform", **dict(kws, cfg=misaligned))
    with pytest.raises(ValueError):
        S.stream_generate(consensus="gaussian", **kws)
    with pytest.raises(ValueError):
        S.stream_generate(consensus=[1.0, 1.0, 1.0], **kws)                                   # L is 2
    noise = torch.randn(4, 8, 2, 4, 4, generator=torch.Generator().manual_seed(13))          # independent windows
    with pytest.raises(ValueError, match="windows_from_canvas"):
        S.stream_generate(consensus="uniform", init_noise=noise, **kws)
    with pytest.raises(ValueError, match="shape"):
        S.stream_generate(consensus="uniform", init_noise=noise[:3], **kws)
    # windows of a canvas are accepted, and give what the same canvas drawn from `seed` gives
    canvas = torch.randn(8, 5, 4, 4, generator=torch.Generator().manual_seed(10))
    ok = S.stream_generate(consensus="uniform", return_latents=True, init_noise=S.windows_from_canvas(canvas, 2, 1), **kws)
    assert np.array_equal(ok["latents"], S.stream_generate(consensus="uniform", return_latents=True, **kws)["latents"])
