"""``stream_generate(sampler="fifo")`` on the MI355X: the latent canvas equals ``fifo_denoise`` called by hand on an engine built with
the same arguments and a prompt canvas made from ``encode_*``, ``window_consensus`` and ``canvas_from_windows``; the output equals
the existing decode and cross-fade of that canvas' windows; every option reaches the matching ``fifo_denoise`` argument; an init clip
guides the queue.  Every comparison is bit for bit."""
import numpy as np
import pytest
import torch

from _kit import STREAM_HALF_SECOND, audio_prompt, components, dev, engine, model, pipeline, pipeline_cfg, with_sampling  # noqa: F401

pytestmark = pytest.mark.gpu
STREAM_ONE_SECOND = {"window_seconds": 1.0, "hop_seconds": 0.5, "crossfade_seconds": 0.25}
SEED = 31


def _abar():
    from multimodal_diffusion_amd import schedule_utils as su
    return su.alphas_cumprod_from_betas(su.make_beta_schedule(1000, kind="cosine", min_beta=1e-4, max_beta=0.02))[1]


def _one_canvas(windows, hop):
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd import stream_infer as S
    return S.canvas_from_windows(Fn.window_consensus(windows.float().contiguous(), hop), hop)


class Case:
    """one reduced audio -> video pipeline: window / hop seconds, the geometry they imply, the prompt canvas made by hand once"""

    def __init__(self, dev, mods, streaming, clip_seconds, n_samples, S_, hop_t, prompt_hop):
        from multimodal_diffusion_amd import _pipeline as P
        from multimodal_diffusion_amd import stream_infer as S
        self.dev, self.mods = dev, mods
        self.vae, self.codec, self.cfg = pipeline(dev, seed=8, clip_seconds=clip_seconds, sampler_steps=4, streaming=streaming)
        self.kw = dict(components(mods, self.vae, self.codec, dev), cfg=self.cfg, **dict(audio_prompt(n_samples), seed=SEED))
        self.S, self.sl, self.hop_t, self.L_t, self.prompt_hop = S_, 2, hop_t, S_ * 2, prompt_hop
        self.P = 3 * hop_t + self.L_t
        self.n_slots = -(-self.P // 2)
        chunks = S.split_audio_into_windows(self.kw["prompt_audio"], 16000, streaming["window_seconds"], streaming["hop_seconds"])[0]
        assert chunks.shape[0] == 4
        self.prompt_canvas = _one_canvas(P.encode_audio(self.codec, chunks, dev), 75)
        assert tuple(self.prompt_canvas.shape) == (8, 375)

    def engine(self, B, **kw):
        return engine(self.mods, "video", (B, 8, self.L_t, 4, 4), 37, guidance=2.0, alpha_bar=_abar(), tube=(2, 4, 4), chunk=(4, 4), **kw)

    def by_hand(self, steps=4, B=None, eng_kw=None, sched=None, **fifo_kw):
        import multimodal_diffusion_amd as A
        from multimodal_diffusion_amd import schedule_utils as su
        sched = su.make_sampling_schedule(1000, steps) if sched is None else sched
        B = (sched.numel() - 1) // (self.S - fifo_kw.get("lookahead", 0)) if B is None else B
        canvas = A.fifo_denoise(self.engine(B, **(eng_kw or {})), self.prompt_canvas, self.prompt_hop, sched, self.n_slots, SEED, **fifo_kw)
        assert canvas.shape[1] == self.n_slots * 2
        return canvas[:, :self.P].contiguous()

    def video(self, canvas):
        """the existing decode and cross-fade of the canvas' windows"""
        from multimodal_diffusion_amd import stream_infer as S
        x = self.vae.decode(S.windows_from_canvas(canvas, self.L_t, self.hop_t)).clamp(0, 1)
        frames = (x.permute(0, 2, 3, 4, 1) * 255.0).to(torch.uint8).contiguous()
        st = self.cfg["streaming"]
        w = torch.from_numpy(S.video_fade_window(frames.shape[1], int(round(st["crossfade_seconds"] * 16))))
        return S.crossfade_tensor(frames, w, int(round(16 * st["hop_seconds"]))).cpu().numpy()

    def init_clip(self):
        """(init_video, its known canvas made by hand)"""
        from multimodal_diffusion_amd import _pipeline as P
        from multimodal_diffusion_amd import stream_infer as S
        st = self.cfg["streaming"]
        n = int(round(16 * (st["window_seconds"] + 3 * st["hop_seconds"])))
        vid = torch.randint(0, 256, (n, 32, 32, 3), generator=torch.Generator().manual_seed(5), dtype=torch.uint8).numpy()
        chunks = S.split_frames_into_windows(vid, 16, st["window_seconds"], st["hop_seconds"])[0]
        assert chunks.shape[0] == 4
        return vid, _one_canvas(P.encode_video(self.vae, chunks, self.dev), self.hop_t)


@pytest.fixture(scope="module")
def one_second(dev, model):
    """1.0 s windows every 0.5 s: S = 2 slots of 2, P = 10, 5 slots; 36000 samples are 4 windows"""
    return Case(dev, model[1], STREAM_ONE_SECOND, 1.0, 36000, 2, 2, 75)


@pytest.fixture(scope="module")
def half_second(dev, model):
    """0.5 s windows every 0.25 s: S = 1, P = 5 of 3 slots = 6 positions: the canvas is cropped"""
    return Case(dev, model[1], STREAM_HALF_SECOND, 0.5, 18000, 1, 1, 150)


def _fifo(case, **kw):
    from multimodal_diffusion_amd import stream_infer as S
    return S.stream_generate(sampler="fifo", return_latents=True, **dict(case.kw, **kw))


# ------------------------------------------------------------------------------------------------- by-hand equivalence
@pytest.mark.parametrize("which", ["one_second", "half_second"])
def test_fifo_sampler_equals_fifo_denoise_by_hand(request, which):
    from multimodal_diffusion_amd import stream_infer as S
    case = request.getfixturevalue(which)
    res = _fifo(case)
    want = case.by_hand()
    assert want.shape[1] == case.P and (case.n_slots * 2 > case.P) == (which == "half_second")
    assert res["latent_canvas"].dtype == np.float32 and np.array_equal(res["latent_canvas"], want.cpu().numpy())
    assert np.array_equal(res["latents"], S.windows_from_canvas(want, case.L_t, case.hop_t).cpu().numpy())
    assert res["latents"].shape == (4, 8, case.L_t, 4, 4)
    assert np.array_equal(res["video"], case.video(want)) and res["fps"] == 16
    again = _fifo(case)
    assert again["video"].tobytes() == res["video"].tobytes() and again["latent_canvas"].tobytes() == res["latent_canvas"].tobytes()
    # the windows sampler's output has the same length and dtype; streaming.sampler selects the queue as the argument does
    old = S.stream_generate(**case.kw)
    assert old["video"].shape == res["video"].shape and old["video"].dtype == res["video"].dtype == np.uint8
    by_cfg = dict(case.cfg, streaming=dict(case.cfg["streaming"], sampler="fifo"))
    by_cfg = S.stream_generate(return_latents=True, **dict(case.kw, cfg=by_cfg))
    assert np.array_equal(by_cfg["latent_canvas"], res["latent_canvas"])
    # decoding window by window gives the same frames
    assert np.array_equal(_fifo(case, max_windows_per_batch=1)["video"], res["video"])


def test_seed_none_is_drawn_from_the_global_generator(one_second):
    torch.manual_seed(123)
    a = _fifo(one_second, seed=None)["latent_canvas"]
    torch.manual_seed(123)
    b = _fifo(one_second, seed=None)["latent_canvas"]
    c = _fifo(one_second, seed=None)["latent_canvas"]
    assert np.array_equal(a, b) and not np.array_equal(b, c)


# ------------------------------------------------------------------------------------------------- options
def test_solver_and_eta_reach_the_engine(one_second):
    case = one_second
    got = _fifo(case, cfg=with_sampling(case.cfg, solver="dpmpp_2m"))["latent_canvas"]
    assert np.array_equal(got, case.by_hand(eng_kw=dict(solver="dpmpp_2m")).cpu().numpy())
    assert not np.array_equal(got, _fifo(case)["latent_canvas"])
    got = _fifo(case, cfg=with_sampling(case.cfg, ddim_eta=0.5), noise_seed=5)["latent_canvas"]
    assert np.array_equal(got, case.by_hand(eng_kw=dict(eta=0.5, noise_seed=5)).cpu().numpy())
    with pytest.raises(ValueError, match="noise_seed"):                          # fifo_denoise's own refusal
        _fifo(case, cfg=with_sampling(case.cfg, ddim_eta=0.5))


def test_fifo_options_reach_fifo_denoise(one_second):
    case = one_second
    plain = _fifo(case)["latent_canvas"]
    got = _fifo(case, fifo={"lookahead": 1})["latent_canvas"]                   # h = 1: B = 4 windows of the queue
    assert np.array_equal(got, case.by_hand(lookahead=1).cpu().numpy()) and not np.array_equal(got, plain)
    got = _fifo(case, fifo={"graph": True})["latent_canvas"]
    assert np.array_equal(got, case.by_hand(graph=True).cpu().numpy()) and np.array_equal(got, plain)
    got = _fifo(case, fifo={"steps": 8})["latent_canvas"]                       # B = 4
    assert np.array_equal(got, case.by_hand(steps=8).cpu().numpy())
    by_cfg = _fifo(case, cfg=dict(case.cfg, streaming=dict(STREAM_ONE_SECOND, fifo={"steps": 8})))["latent_canvas"]
    assert np.array_equal(by_cfg, got)


def test_config_cfg_controls_become_slot_controls(one_second):
    from multimodal_diffusion_amd import schedule_utils as su
    case = one_second
    plain = _fifo(case)["latent_canvas"]
    table = su.guidance_interval_table(2.0, (200, 800), 1000)
    got = _fifo(case, guidance_interval=(200, 800), cfg=with_sampling(case.cfg, guidance_rescale={"video": 0.5}))["latent_canvas"]
    assert np.array_equal(got, case.by_hand(guidance_by_level=table, rescale_by_level=0.5).cpu().numpy())
    assert not np.array_equal(got, plain)
    by_cfg = _fifo(case, cfg=with_sampling(case.cfg, guidance_interval={"video": [200, 800]}))["latent_canvas"]
    assert np.array_equal(by_cfg, case.by_hand(guidance_by_level=table).cpu().numpy())
    apg = {"norm_threshold": 2.0, "eta_parallel": 0.5}
    got = _fifo(case, cfg=with_sampling(case.cfg, apg={"video": apg}))["latent_canvas"]
    assert np.array_equal(got, case.by_hand(apg=apg).cpu().numpy()) and not np.array_equal(got, plain)


# ------------------------------------------------------------------------------------------------- init clip
def test_init_clip_guides_the_queue(one_second):
    case = one_second
    vid, known = case.init_clip()
    assert tuple(known.shape) == (8, 10, 4, 4)
    plain = _fifo(case)["latent_canvas"]
    mask = torch.zeros(8, 10, 4, 4)
    mask[:, 2:6] = 1.0                                                           # clip slots 1 and 2, whole
    res = _fifo(case, init_video=vid, mask=mask)
    got = res["latent_canvas"]
    assert np.array_equal(got[:, 2:6], known[:, 2:6].cpu().numpy())              # held: the consensus-made known canvas, bit for bit
    assert not np.array_equal(got[:, :2], plain[:, :2]) and not np.array_equal(got[:, 6:], plain[:, 6:])
    assert np.array_equal(got, case.by_hand(init_canvas=known, mask=mask).cpu().numpy())      # the stand-alone tail pass after every shift
    assert np.array_equal(got, case.by_hand(init_canvas=known, mask=mask, guided_shift=True).cpu().numpy())      # what the pipeline runs
    assert np.array_equal(res["video"], case.video(torch.from_numpy(got).to(case.dev)))
    assert np.array_equal(_fifo(case, init_video=vid, mask=torch.zeros(1))["latent_canvas"], plain)      # nothing held: the unguided bits
    # dpmpp_2m moves its history through the guided shift
    cfg2 = with_sampling(case.cfg, solver="dpmpp_2m")
    got = _fifo(case, init_video=vid, mask=mask, cfg=cfg2)["latent_canvas"]
    assert np.array_equal(got, case.by_hand(eng_kw=dict(solver="dpmpp_2m"), init_canvas=known, mask=mask).cpu().numpy())
    assert np.array_equal(got[:, 2:6], known[:, 2:6].cpu().numpy())
    with pytest.raises(ValueError, match="graph=True is refused"):
        _fifo(case, init_video=vid, mask=mask, fifo={"graph": True})
    with pytest.raises(ValueError, match="lookahead > 0 is refused"):
        _fifo(case, init_video=vid, mask=mask, fifo={"lookahead": 1})


def test_strength_truncates_the_schedule(one_second):
    from multimodal_diffusion_amd import schedule_utils as su
    case = one_second
    vid, known = case.init_clip()
    sched = su.truncate_schedule(su.make_sampling_schedule(1000, 8), 0.5)
    assert sched.numel() - 1 == 4                                                # 4 of 8 steps: B = 2
    got = _fifo(case, init_video=vid, strength=0.5, fifo={"steps": 8})["latent_canvas"]
    want = case.by_hand(sched=sched, init_canvas=known, mask=torch.zeros(1), guide_start="init")
    assert np.array_equal(got, want.cpu().numpy())
    assert not np.array_equal(got, _fifo(case)["latent_canvas"])
    mask = torch.zeros(8, 10, 4, 4)
    mask[:, 4:8] = 1.0
    got = _fifo(case, init_video=vid, strength=0.5, mask=mask, fifo={"steps": 8}, guide_seed=9)["latent_canvas"]
    want = case.by_hand(sched=sched, init_canvas=known, mask=mask, guide_start="init", guide_seed=9)
    assert np.array_equal(got, want.cpu().numpy()) and np.array_equal(got[:, 4:8], known[:, 4:8].cpu().numpy())
    # strength 0: the decoded known canvas, no model call (without the model's modules an engine could not be built)
    res = _fifo(case, init_video=vid, strength=0.0, core=None, head=None, adapt_v=None, adapt_a=None)
    assert np.array_equal(res["latent_canvas"], known.cpu().numpy()) and np.array_equal(res["video"], case.video(known))


# ------------------------------------------------------------------------------------------------- video prompt -> audio
def test_video_prompt_to_audio(dev, model):
    """16 audio latent frames per 1.0 s window in chunks of 4: S = 4, one prompt latent frame per slot, 4 steps: B = 1"""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import _pipeline as P
    from multimodal_diffusion_amd import stream_infer as S
    from multimodal_diffusion_amd import schedule_utils as su
    torch.manual_seed(8)
    vae = A.VideoVAE.from_config({"latent": {"channels": 8, "t_down": 4, "s_down": 8}}).eval().to(dev)
    codec = A.AudioCodec.from_config({"sr": 16000, "latent": {"channels": 8, "frames_per_clip": 16},
                                      "codec": {"hop_samples": 1000}}).eval().to(dev)
    cfg = pipeline_cfg(clip_seconds=1.0, sampler_steps=4, streaming=STREAM_ONE_SECOND)
    cfg["audio"]["latent"]["frames_per_clip"] = 16
    geo = S.fifo_geometry(cfg, "video", 4, 4)
    assert (geo.S, geo.prompt_hop, geo.B, geo.P, geo.n_slots) == (4, 1, 1, 40, 10)
    vid = torch.randint(0, 256, (40, 32, 32, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).numpy()
    kw = dict(components(model[1], vae, codec, dev), cfg=cfg, prompt_modality="video", prompt_video=vid, prompt_audio=None, seed=SEED)
    res = S.stream_generate(sampler="fifo", return_latents=True, **kw)
    chunks = S.split_frames_into_windows(vid, 16, 1.0, 0.5)[0]
    assert chunks.shape[0] == 4
    prompt_canvas = _one_canvas(P.encode_video(vae, chunks, dev), 2)
    assert tuple(prompt_canvas.shape) == (8, 10, 4, 4)
    eng = engine(model[1], "audio", (1, 8, 16), 2, guidance=2.0, alpha_bar=_abar(), tube=(2, 4, 4), chunk=(4, 4))
    want = A.fifo_denoise(eng, prompt_canvas, 1, su.make_sampling_schedule(1000, 4), 10, SEED)
    assert tuple(want.shape) == (8, 40) and np.array_equal(res["latent_canvas"], want.cpu().numpy())
    assert res["latents"].shape == (4, 8, 16)
    wav = codec.decode(S.windows_from_canvas(want, 16, 8))[:, 0, :].contiguous()
    w = torch.from_numpy(S.audio_fade_window(wav.shape[1], int(round(16000 * 0.25))))
    assert np.array_equal(res["audio"], S.crossfade_tensor(wav, w, 8000).cpu().numpy()) and res["sr"] == 16000
    assert res["audio"].shape == S.stream_generate(**kw)["audio"].shape
