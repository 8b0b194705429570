"""The fractional prompt hop on the MI355X (include/avdiff_hip.h, "fractional prompt hop"): ``functional.fifo_prompt_gather_frac``
against ``fifo_prompt_windows`` computed on the CPU, on both lane widths, off a cursor and by value; its den == 1 case against the
integer gather; the three drivers of ``fifo_denoise`` under an audio target with a video prompt at hop 2/3 against loops written here
from their parts; and ``stream_generate(sampler="fifo", fifo={"prompt_interp": ...})`` video -> audio.  Every comparison is bit for
bit: the gather's only arithmetic is the fp32 blend, which the contract fixes operation by operation."""
import numpy as np
import pytest
import torch

from _kit import components, dev, engine, model, pipeline_cfg  # noqa: F401  (dev, model are fixtures)

pytestmark = pytest.mark.gpu

GS = 3.5
SEED = 0x5EED0F1F0
ESEED = 77
STREAM_ONE_SECOND = {"window_seconds": 1.0, "hop_seconds": 0.5, "crossfade_seconds": 0.25}
MODES = ("nearest", "linear")
SCHED12 = torch.linspace(999, -1, 13).round().long()


def cur(dev, v):
    return torch.tensor([v], dtype=torch.int32, device=dev)


def off(x):
    """a copy of x whose base is misaligned by one float"""
    v = torch.empty(x.numel() + 1, device=x.device)[1:].view(x.shape).copy_(x)
    assert v.data_ptr() % 16 != 0
    return v


# ------------------------------------------------------------------------------------------------- the kernel
def _canvas(kind):
    g = torch.Generator().manual_seed(5)
    return torch.randn({"audio": (3, 11), "video": (2, 7, 4, 4), "video_off": (2, 7, 4, 4), "video_6": (2, 7, 2, 3)}[kind], generator=g)


@pytest.mark.parametrize("kind", ["audio", "video", "video_off", "video_6"])
def test_gather_equals_fifo_prompt_windows_on_the_cpu(dev, kind):
    """audio: inner = 1, the one-element lane; video: inner = 16 from an aligned base, 16-byte lanes; the same canvas from a base 4
    bytes on, and inner = 6: the one-element lane again.  S = 4, a window of 3 rows."""
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_windows
    cpu = _canvas(kind)
    canvas = off(cpu.to(dev)) if kind == "video_off" else cpu.to(dev)
    assert (canvas.data_ptr() % 16 == 0) == (kind != "video_off")
    S, Lp = 4, 3
    far = 2 ** 31 - 1
    for num, den in ((2, 3), (8, 25), (3, 2)):
        for mode in MODES:
            for B in (1, 3):
                for stride in (2, S):
                    ref = lambda first: fifo_prompt_windows(cpu, 0, B, S, num, Lp, stride=stride, first=first, prompt_den=den, prompt_interp=mode)
                    tag = (num, den, mode, B, stride)
                    for m in (-3, 0, 1, 2, 5, far):                              # off the cursor: m = max(*cursor, 0), first = 0
                        out = Fn.fifo_prompt_gather_frac(canvas, cur(dev, m), B, 0, stride, num, den, mode, Lp)
                        assert out.shape == (B, cpu.shape[0], Lp) + tuple(cpu.shape[2:])
                        assert torch.equal(out.cpu(), ref(max(m, 0))), tag + (m,)
                    assert not out.any()                                         # far past the end: the null prompt
                    for first in range(-5, 13):                                  # by value, no cursor
                        out = Fn.fifo_prompt_gather_frac(canvas, None, B, first, stride, num, den, mode, Lp)
                        assert torch.equal(out.cpu(), ref(first)), tag + (first,)
                    # the cursor adds to a negative first: the lookahead's m - ctx
                    out = Fn.fifo_prompt_gather_frac(canvas, cur(dev, 4), B, -3, stride, num, den, mode, Lp)
                    assert torch.equal(out.cpu(), ref(1)), tag
    # hop 2/3 walks rem through 0, 2, 1
    assert [(q * 2) % 3 for q in range(3)] == [0, 2, 1]
    # a misaligned out takes the one-element lane: same bits
    want = fifo_prompt_windows(cpu, 0, 3, S, 2, Lp, first=1, prompt_den=3, prompt_interp="linear")
    o2 = off(torch.full_like(want, float("nan")).to(dev))
    assert torch.equal(Fn.fifo_prompt_gather_frac(canvas, None, 3, 1, S, 2, 3, "linear", Lp, out=o2).cpu(), want)


@pytest.mark.parametrize("kind", ["audio", "video"])
def test_den_1_equals_the_integer_gather(dev, kind):
    from multimodal_diffusion_amd import functional as Fn
    canvas = _canvas(kind).to(dev)
    canvas[0, 3] = float("inf")                                                  # a blend at rem == 0 would spread it
    B, S, Lp = 3, 2, 3
    for hop in (1, 2):
        for m in (0, 1, 2, 5):
            ref = Fn.fifo_prompt_gather(canvas, cur(dev, m), B, S, hop, Lp)
            for mode in MODES:
                assert torch.equal(Fn.fifo_prompt_gather_frac(canvas, cur(dev, m), B, 0, S, hop, 1, mode, Lp), ref), (hop, m, mode)
                assert torch.equal(Fn.fifo_prompt_gather_frac(canvas, None, B, m, S, hop, 1, mode, Lp), ref), (hop, m, mode)


def test_gather_refusals(dev):
    from multimodal_diffusion_amd import functional as Fn
    canvas = _canvas("video").to(dev)
    with pytest.raises(ValueError, match="prompt_interp must be None or one of"):
        Fn.fifo_prompt_gather_frac(canvas, None, 1, 0, 1, 2, 3, "cubic", 3)
    with pytest.raises(ValueError, match="interp must be one of"):
        Fn.fifo_prompt_gather_frac(canvas, None, 1, 0, 1, 2, 1, None, 3)
    with pytest.raises(ValueError, match="needs prompt_interp"):
        Fn.fifo_prompt_gather_frac(canvas, None, 1, 0, 1, 2, 3, None, 3)
    with pytest.raises(ValueError, match="prompt_den must be an int"):
        Fn.fifo_prompt_gather_frac(canvas, None, 1, 0, 1, 2, 0, "linear", 3)
    with pytest.raises(ValueError, match="first must be an int"):
        Fn.fifo_prompt_gather_frac(canvas, None, 1, 2 ** 31, 1, 2, 3, "linear", 3)
    with pytest.raises(ValueError, match="a cursor is one int32"):
        Fn.fifo_prompt_gather_frac(canvas, torch.zeros(1, dtype=torch.int32), 1, 0, 1, 2, 3, "linear", 3)
    both = torch.zeros(canvas.numel() + 2 * 3 * 16 - 4, device=dev)
    c2, o2 = both[:canvas.numel()].view(canvas.shape), both[canvas.numel() - 4:].view(1, 2, 3, 4, 4)
    with pytest.raises(ValueError, match="overlap"):
        Fn.fifo_prompt_gather_frac(c2, None, 1, 0, 1, 2, 3, "linear", 3, out=o2)


# ------------------------------------------------------------------------------------------------- the drivers
def _setup(dev, mods, B, solver="ddim", eta=0.0):
    """(engine, CPU prompt canvas): an audio target of 24 latent frames in chunks of 4 / 4 (S = 6) under a video prompt of 4 latent
    frames per sample (8 tubes of 2 x 4 x 4 on 8 x 8), hop 4 * 4 / 24 = 2 / 3.  The canvas has 9 positions: with n = 12 and 5 slots the
    queue's last windows start at position floor(16 * 2 / 3) = 10, past its end."""
    kw = dict(guidance=GS, solver=solver, eta=eta, **({"noise_seed": ESEED} if eta > 0 else {}))
    eng = engine(mods, "audio", (B, 8, 24), 8, **kw)
    assert (eng.slots, eng.slot_len) == (6, 4)
    return eng, torch.randn(8, 9, 8, 8, generator=torch.Generator().manual_seed(17))


def _loop(eng, canvas_cpu, mode, K, seed):
    """fifo_denoise(prompt_den=3) restated from its parts: the plan's tables, the prompt windows computed on the CPU and uploaded,
    set_prompt, step_slots and the engine's queue shift"""
    from multimodal_diffusion_amd import functional as Fn, schedule_utils as su
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_windows
    dev = eng.device
    B, S, sl = eng.embed.B, eng.slots, eng.slot_len
    n = B * S
    rn, rp, sn, sp = su.fifo_plan(SCHED12, S)
    dpm = eng.solver == "dpmpp_2m"
    rl, last = su.fifo_plan_last(SCHED12, S) if dpm else (None, None)
    key = (lambda m: m) if eng.eta > 0 else (lambda m: None)
    prompt = lambda m: fifo_prompt_windows(canvas_cpu, m, B, S, 2, 4, prompt_den=3, prompt_interp=mode).to(dev)
    z = Fn.canvas_noise(seed, torch.full((B,), 999), eng.latent_shape, eng.latent_shape[2])
    eng.set_prompt(prompt(0))
    for r in range(n - 1):
        z = eng.step_slots(z, rn[r], rp[r], t_last=rl[r] if dpm else None, clip_first=key(0))
    done = []
    for m in range(K):
        eng.set_prompt(prompt(m))
        z = eng.step_slots(z, sn, sp, t_last=last, clip_first=key(m))
        z, popped = eng.fifo_shift(z, n + m, 999, seed=seed)
        done.append(popped.clone())
    return torch.cat(done, 1)


@pytest.mark.parametrize("solver,eta", [("ddim", 0.0), ("dpmpp_2m", 0.0), ("ddim", 0.5)])
@pytest.mark.parametrize("mode", MODES)
def test_fifo_denoise_walks_the_fraction(dev, model, mode, solver, eta):
    """12 steps on S = 6: B = 2; n_slots = 5: the graph driver takes eager + two pairs.  The eager loop, the replayed one and the loop
    of parts give the same bits."""
    import multimodal_diffusion_amd as A
    eng, canvas = _setup(dev, model[1], 2, solver, eta)
    out = A.fifo_denoise(eng, canvas.to(dev), 2, SCHED12, 5, SEED, prompt_den=3, prompt_interp=mode)
    assert out.shape == (8, 20) and torch.isfinite(out).all() and float(out.std()) > 0
    ref = _loop(eng, canvas, mode, 5, SEED)
    assert torch.equal(out, ref), float((out - ref).abs().max())
    replayed = A.fifo_denoise(eng, canvas.to(dev), 2, SCHED12, 5, SEED, graph=True, prompt_den=3, prompt_interp=mode)
    assert not torch.cuda.is_current_stream_capturing()
    assert torch.equal(replayed, out), float((replayed - out).abs().max())
    if (solver, eta) == ("ddim", 0.0):
        # the prompt is read: the other mode, and the whole hop 2 / 1, are other clips
        other = A.fifo_denoise(eng, canvas.to(dev), 2, SCHED12, 5, SEED, prompt_den=3, prompt_interp=MODES[1 - MODES.index(mode)])
        assert not torch.equal(other, out)
        whole = A.fifo_denoise(eng, canvas.to(dev), 2, SCHED12, 5, SEED)
        assert not torch.equal(whole, out)
        # den == 1 under a mode is that whole hop, on every driver
        assert torch.equal(A.fifo_denoise(eng, canvas.to(dev), 2, SCHED12, 5, SEED, prompt_den=1, prompt_interp=mode), whole)
        assert torch.equal(A.fifo_denoise(eng, canvas.to(dev), 2, SCHED12, 5, SEED, graph=True, prompt_den=1, prompt_interp=mode), whole)


def _lookahead_loop(eng, canvas_cpu, mode, K, ctx, seed):
    """fifo_denoise(lookahead=ctx, prompt_den=3) restated from its parts: the lookahead plan, the start queue cut into overlapping
    windows, the CPU prompt windows of clip slots m - ctx + k * h, step_slots and the engine's lookahead launch"""
    from multimodal_diffusion_amd import functional as Fn, schedule_utils as su
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_windows, windows_from_canvas
    dev = eng.device
    B, S, sl = eng.embed.B, eng.slots, eng.slot_len
    h = S - ctx
    n = B * h
    rn, rp, sn, sp = su.fifo_lookahead_plan(SCHED12, S, ctx, "noise")
    dpm = eng.solver == "dpmpp_2m"
    rl, last = su.fifo_lookahead_plan_last(SCHED12, S, ctx) if dpm else (None, None)
    off_, stride = su.fifo_slot_keying(S, ctx)
    key = (lambda m: dict(clip_first=m + off_, clip_stride=stride)) if eng.eta > 0 else (lambda m: {})
    prompt = lambda m: fifo_prompt_windows(canvas_cpu, 0, B, S, 2, 4, stride=h, first=m - ctx, prompt_den=3, prompt_interp=mode).to(dev)
    t0 = torch.tensor([999])
    head = Fn.canvas_noise(seed, t0, (1, 8, ctx * sl), 1, window_offset=2 ** 32 - ctx * sl)[0]
    z = windows_from_canvas(torch.cat([head, Fn.canvas_noise(seed, t0, (1, 8, n * sl), n * sl)[0]], 1), S * sl, h * sl)
    eng.set_prompt(prompt(0))
    for r in range(n - 1):
        z = eng.step_slots(z, rn[r], rp[r], t_last=rl[r] if dpm else None, **key(0))
        z, _ = eng.fifo_lookahead(z, ctx, 0)
    done = []
    for m in range(K):
        eng.set_prompt(prompt(m))
        row = min(m, ctx)
        z = eng.step_slots(z, sn[row], sp[row], t_last=last[row] if dpm else None, **key(m))
        z, popped = eng.fifo_lookahead(z, ctx, 1, c=n + m, t=999, seed=seed)
        done.append(popped.clone())
    return torch.cat(done, 1)


@pytest.mark.parametrize("solver,eta", [("ddim", 0.0), ("dpmpp_2m", 0.0), ("ddim", 0.5)])
@pytest.mark.parametrize("mode", MODES)
def test_lookahead_walks_the_fraction(dev, model, mode, solver, eta):
    """lookahead 3 of S = 6: h = 3, 12 steps: B = 4 windows; the first windows start at clip slots -3 .. (prompt rows before the canvas)"""
    import multimodal_diffusion_amd as A
    eng, canvas = _setup(dev, model[1], 4, solver, eta)
    out = A.fifo_denoise(eng, canvas.to(dev), 2, SCHED12, 5, SEED, lookahead=3, prompt_den=3, prompt_interp=mode)
    assert out.shape == (8, 20) and torch.isfinite(out).all() and float(out.std()) > 0
    ref = _lookahead_loop(eng, canvas, mode, 5, 3, SEED)
    assert torch.equal(out, ref), float((out - ref).abs().max())
    if (solver, eta) == ("ddim", 0.0):
        assert not torch.equal(A.fifo_denoise(eng, canvas.to(dev), 2, SCHED12, 5, SEED, lookahead=3), out)


# ------------------------------------------------------------------------------------------------- the pipeline
def test_video_prompt_to_audio_at_a_fractional_hop(dev, model):
    """24 audio latent frames per 1.0 s window in chunks of 4: S = 6 under 4 prompt latent frames, hop 2 / 3; 12 steps: B = 2"""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import _pipeline as P
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd import schedule_utils as su
    from multimodal_diffusion_amd import stream_infer as S
    torch.manual_seed(8)
    vae = A.VideoVAE.from_config({"latent": {"channels": 8, "t_down": 4, "s_down": 8}}).eval().to(dev)
    codec = A.AudioCodec.from_config({"sr": 24000, "latent": {"channels": 8, "frames_per_clip": 24},
                                      "codec": {"hop_samples": 1000}}).eval().to(dev)
    cfg = pipeline_cfg(clip_seconds=1.0, sampler_steps=4, streaming=STREAM_ONE_SECOND)
    cfg["audio"]["latent"]["frames_per_clip"] = 24
    cfg["audio"]["sr"] = 24000
    vid = torch.randint(0, 256, (32, 32, 32, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).numpy()      # 3 windows
    kw = dict(components(model[1], vae, codec, dev), cfg=cfg, prompt_modality="video", prompt_video=vid, prompt_audio=None, seed=31)
    geo = S.fifo_geometry(cfg, "video", 3, 12, prompt_interp="linear")
    assert (geo.S, geo.prompt_hop, geo.prompt_den, geo.B, geo.P, geo.n_slots, geo.P_p) == (6, 2, 3, 2, 48, 12, 8)
    res = S.stream_generate(sampler="fifo", return_latents=True, fifo={"steps": 12, "prompt_interp": "linear"}, **kw)
    old = S.stream_generate(**kw)
    assert res["audio"].shape == old["audio"].shape and res["audio"].dtype == old["audio"].dtype and res["sr"] == 24000
    assert np.isfinite(res["audio"]).all()
    # the latent canvas is fifo_denoise's, called by hand on the same canvases and seed
    chunks = S.split_frames_into_windows(vid, 16, 1.0, 0.5)[0]
    assert chunks.shape[0] == 3
    z_p = P.encode_video(vae, chunks, dev).float().contiguous()
    prompt_canvas = S.canvas_from_windows(Fn.window_consensus(z_p, 2), 2)
    assert tuple(prompt_canvas.shape) == (8, 8, 4, 4)
    eng = engine(model[1], "audio", (2, 8, 24), 2, guidance=2.0, tube=(2, 4, 4), chunk=(4, 4),
                 alpha_bar=su.alphas_cumprod_from_betas(su.make_beta_schedule(1000, kind="cosine", min_beta=1e-4, max_beta=0.02))[1])
    want = A.fifo_denoise(eng, prompt_canvas, 2, su.make_sampling_schedule(1000, 12), 12, 31, prompt_den=3, prompt_interp="linear")
    assert tuple(want.shape) == (8, 48) and np.array_equal(res["latent_canvas"], want.cpu().numpy())
    assert res["latents"].shape == (3, 8, 24)
    nearest = S.stream_generate(sampler="fifo", return_latents=True, fifo={"steps": 12, "prompt_interp": "nearest"}, **kw)
    assert not np.array_equal(nearest["latent_canvas"], res["latent_canvas"])
    by_cfg = dict(cfg, streaming=dict(STREAM_ONE_SECOND, sampler="fifo", fifo={"steps": 12, "prompt_interp": "linear"}))
    assert np.array_equal(S.stream_generate(return_latents=True, **dict(kw, cfg=by_cfg))["latent_canvas"], res["latent_canvas"])
    with pytest.raises(ValueError, match="whole positions"):                     # without a mode: today's refusal
        S.stream_generate(sampler="fifo", fifo={"steps": 12}, **kw)
