"""Token geometries beyond tube 2 x 4 x 4 and chunk 4 / 4 on the MI355X (the tables of _geom.py): the layout kernels against the CPU
oracle bit for bit, the single-branch fused updates against the composed ops bit for bit in every solver state, the CFG fused updates
against the fp64 oracle, the engine at the geometries the kit's weights serve (one step against the oracle, the controlled step against
the composed path, cond-only, canvas keying, graph replay), sample_one_direction and stream_generate following tokenizer.video.tube / audio.chunk of
the config, and the refusals."""
from functools import partial

import numpy as np
import pytest
import torch

import _geom as G
from _kit import ABAR, STREAM_HALF_SECOND, Recorder, components, dev, engine, model, pipeline, soft_mask, ts  # noqa: F401  (dev / model are fixtures)
from _tune import cfg_rows  # noqa: F401  (fixture)
from conftest import rel_err
from oracle import ref_cpu as R
from test_gpu_cfg_rescale import G2, PHI2, SOLVERS, _check_fused_equals_composed
from test_gpu_guidance_interval import STATES, _check_kernels_equal_composed, _composed, _fused

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # the project's one-step tolerance (test_gpu_parity.TOL)
GS = 3.0
_engine = partial(engine, guidance=GS)        # engine(mods, target, shape, n_prompt, **kw) at this file's guidance
TN, TP = [981, 402, 40], [961, 382, -1]
# what the other modality's prompt looks like at the geometries the kit's weights serve: an audio prompt [B, 8, 40] in 19 chunks of
# 4 / 2, a video prompt [B, 8, 4, 8, 8] in 8 tubes of 1 x 4 x 8
PROMPT_CHUNK, PROMPT_TUBE = (4, 2), (1, 4, 8)
ROWS = [("video", g) for g in G.VIDEO] + [("audio", g) for g in G.AUDIO]
ROW_IDS = [g.id for _, g in ROWS]


def _seed(g):
    return 1000 + int(g.id[1:]) + (100 if g.id[0] == "A" else 0)


def _tok_shape(target, g):
    return (G.n_video_tokens(g), g.D) if target == "video" else (g.Na, g.lat[0] * g.chunk[0])


def _geom(target, g):
    return g.tube if target == "video" else g.chunk


def _untok_ref(target, g, tok):
    """the oracle's U: tokens -> the latent's natural layout"""
    if target == "video":
        return R.tube_unpatch(tok, *g.lat, *g.tube)
    return R.audio_untokens(tok, g.lat[0], g.chunk[0], g.lat[1], g.chunk[1])


# ------------------------------------------------------------------------------------------------- 1. layout kernels = CPU oracle
@pytest.mark.parametrize("g", G.VIDEO, ids=[g.id for g in G.VIDEO])
def test_tube_kernels_equal_oracle(dev, g):
    from multimodal_diffusion_amd import functional as Fn
    gen = torch.Generator().manual_seed(_seed(g))
    z = torch.randn(3, *g.lat, generator=gen)
    tok = torch.randn(3, G.n_video_tokens(g), g.D, generator=gen)
    got = Fn.tube_patch(z.to(dev), *g.tube)
    assert torch.equal(got.cpu(), R.tube_patch(z, *g.tube))
    assert torch.equal(Fn.tube_unpatch(tok.to(dev), *g.lat, *g.tube).cpu(), R.tube_unpatch(tok, *g.lat, *g.tube))
    assert torch.equal(Fn.tube_unpatch(got, *g.lat, *g.tube).cpu(), z)


@pytest.mark.parametrize("g", G.AUDIO, ids=[g.id for g in G.AUDIO])
def test_audio_kernels_equal_oracle(dev, g):
    from multimodal_diffusion_amd import functional as Fn
    (Ca, F), (ln, st) = g.lat, g.chunk
    gen = torch.Generator().manual_seed(_seed(g))
    z = torch.randn(3, Ca, F, generator=gen)
    tok = torch.randn(3, g.Na, Ca * ln, generator=gen)
    assert torch.equal(Fn.audio_tokens(z.to(dev), ln, st).cpu(), R.audio_tokens(z, ln, st))
    off = torch.from_numpy(~G.covered(g))
    for hann in (False, True):
        win = torch.hann_window(ln).to(dev) if hann else None
        got = Fn.audio_untokens(tok.to(dev), Ca, ln, F, st, window=win).cpu()
        ref = R.audio_untokens(tok.float(), Ca, ln, F, st, hann=hann)
        diff = (got - ref).abs()
        assert torch.equal(got, ref), (hann, float(diff.max()), int((diff > 0).sum()))
        assert bool((got[..., off] == 0).all())                # under no window, or the zero padding
    assert int(off.sum()) == {"A2": 1, "A4": 12, "A6": 6}.get(g.id, 0)


# ------------------------------------------------------------------------------------------------- 2. single-branch fused = composed
KCASES = [(t, g, st, gd) for t, g in ROWS for st in STATES for gd in (False, True) if not (gd and st == "noise")]


@pytest.mark.parametrize("target,g,state,guided", KCASES, ids=[f"{g.id}-{st}-{'guide' if gd else 'free'}" for _, g, st, gd in KCASES])
def test_kernels_equal_composed_ops(dev, cfg_rows, target, g, state, guided):
    """test_gpu_guidance_interval.test_kernels_equal_composed_ops at every row of the tables"""
    _check_kernels_equal_composed(dev, cfg_rows, target, g.lat, state, guided, _seed(g), _tok_shape(target, g), _geom(target, g))


# ------------------------------------------------------------------------------------------------- 3. CFG fused vs the fp64 oracle
@pytest.mark.parametrize("eta", [0.0, 0.5])
@pytest.mark.parametrize("target,g", ROWS, ids=ROW_IDS)
def test_cfg_fused_update_vs_oracle(dev, cfg_rows, target, g, eta):
    """avd_cfg_unpatch_ddim_f32 / avd_cfg_untoken_ddim_audio_f32: e = null + g (cond - null) per token, U, DDIM, all in fp64.  The
    null half is three times the cond half's scale: a kernel that finds it at the wrong offset (Na D != Ca F) cannot pass."""
    from multimodal_diffusion_amd import _lib as L
    B, gd = 3, 3.5
    gen = torch.Generator().manual_seed(_seed(g))
    nt, D = _tok_shape(target, g)
    eps2 = torch.randn(2 * B, nt, D, generator=gen)
    eps2[B:] *= 3.0
    z = torch.randn(B, *g.lat, generator=gen)
    noise = torch.randn(B, *g.lat, generator=gen) if eta > 0 else None
    tn, tp = torch.tensor(TN), torch.tensor(TP)
    d_eps, d_z, d_tn, d_tp, d_ab = eps2.to(dev), z.to(dev), tn.to(dev), tp.to(dev), ABAR.to(dev)     # (kept alive across the launches)
    d_noise = None if noise is None else noise.to(dev)
    outs = []
    for rows in ((1, 0) if target == "video" else (1,)):
        cfg_rows(rows)
        out = torch.full((B, *g.lat), float("nan"), device=dev)
        head = (d_eps.data_ptr(), d_z.data_ptr(), d_tn.data_ptr(), d_tp.data_ptr(), d_ab.data_ptr(), d_ab.numel(), gd, eta, L.ptr(d_noise),
                out.data_ptr(), B)
        fn = L.lib().avd_cfg_unpatch_ddim_f32 if target == "video" else L.lib().avd_cfg_untoken_ddim_audio_f32
        L.check(fn(*head, *g.lat, *_geom(target, g), L.stream_ptr(dev)))
        outs.append(out.cpu())
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1])                   # rows form == gather form
    e = eps2[B:].double() + gd * (eps2[:B].double() - eps2[B:].double())
    ref = R.ddim_update(z.double(), tn, tp, _untok_ref(target, g, e), ABAR.double(), eta=eta, noise=None if noise is None else noise.double())
    err = rel_err(outs[0], ref)
    print(f"cfg fused update vs fp64 oracle: {g.id} eta {eta}: rel_err {err:.3e} (bound 1e-5)")
    assert torch.isfinite(outs[0]).all() and err < 1e-5, (g.id, eta, err)


# ------------------------------------------------------------------------------------------------- 4. the engine
ENGINE_ROWS = [("video", G.V[i]) for i in ("V1", "V9", "V10")] + [("audio", G.A[i]) for i in ("A1", "A2", "A4", "A5", "A9")]
ENGINE_IDS = [g.id for _, g in ENGINE_ROWS]


def _case(dev, target, g, B):
    """(z, prompt latent, prompt tokens, engine keywords) of a kit-compatible row"""
    gen = torch.Generator().manual_seed(_seed(g))
    z = torch.randn(B, *g.lat, generator=gen).to(dev)
    if target == "video":
        zp, npr, kw = torch.randn(B, 8, 40, generator=gen), 19, dict(tube=g.tube, chunk=PROMPT_CHUNK)
    else:
        zp, npr, kw = torch.randn(B, 8, 4, 8, 8, generator=gen), 8, dict(tube=PROMPT_TUBE, chunk=g.chunk)
    return z, zp.to(dev), npr, kw


@pytest.mark.parametrize("target,g", ENGINE_ROWS, ids=ENGINE_IDS)
def test_engine_step_vs_oracle(dev, model, target, g):
    ws, mods = model
    z, zp, npr, kw = _case(dev, target, g, 3)
    eng = _engine(mods, target, tuple(z.shape), npr, **kw)
    assert eng.embed.Nt == _tok_shape(target, g)[0]
    eng.set_prompt(zp)
    assert eng.Xp.shape[1] == npr
    tn, tp = ts(TN, dev), ts(TP, dev)
    out = eng.step(z, tn, tp)
    assert tuple(eng.eps_tokens().shape) == (6, *_tok_shape(target, g))
    step = R.denoise_step_a2v if target == "video" else R.denoise_step_v2a
    ref = step(z.cpu(), zp.cpu(), tn.cpu(), tp.cpu(), ABAR, adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"], head=ws["head"],
               n_layers=2, n_heads=8, guidance=GS, tube=kw["tube"], chunk=kw["chunk"])
    err = rel_err(out.cpu(), ref)
    print(f"one CFG step vs the oracle: {g.id}: rel_err {err:.3e} (bound {TOL:g})")
    assert torch.isfinite(out).all() and err < TOL, (g.id, err)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("skw", SOLVERS, ids=["ddim", "seeded", "dpmpp_2m"])
@pytest.mark.parametrize("target,g", ENGINE_ROWS, ids=ENGINE_IDS)
def test_fused_equals_composed(dev, model, cfg_rows, target, g, skw, guided):
    """test_gpu_cfg_rescale.test_fused_equals_composed (per-sample guidance and rescale) at the engine rows, and s_b of the composed
    path against the numpy mirror (A9: two statistics chunks per sample)"""
    z, zp, npr, kw = _case(dev, target, g, 2)
    eng = _engine(model[1], target, tuple(z.shape), npr, guidance=G2, guidance_rescale=PHI2, **kw, **skw)
    eng.set_prompt(zp)
    known = torch.randn(z.shape, generator=torch.Generator().manual_seed(9)).to(dev)
    mask = soft_mask(tuple(z.shape[1:])).to(dev) if guided else None
    _check_fused_equals_composed(dev, eng, cfg_rows, z, known, mask, skw, check_scale=True)


@pytest.mark.parametrize("target,g", [("video", G.V["V1"]), ("video", G.V["V9"]), ("audio", G.A["A1"]), ("audio", G.A["A4"])],
                         ids=["V1", "V9", "A1", "A4"])
def test_cond_only_step_equals_composed(dev, model, cfg_rows, target, g):
    z, zp, npr, kw = _case(dev, target, g, 3)
    eng = _engine(model[1], target, tuple(z.shape), npr, guidance_interval=(300, 700), **kw)
    eng.set_prompt(zp)
    tn, tp = ts(TN, dev), ts(TP, dev)
    geom = _geom(target, g)
    outs = []
    for rows in ((1, 0) if target == "video" else (1,)):
        cfg_rows(rows)
        out = eng.step(z, tn, tp, cond_only=True).clone()
        eps = eng.eps_tokens()
        assert tuple(eps.shape) == (3, *_tok_shape(target, g))
        assert torch.equal(out, _composed(dev, target, eps, z, tn, tp, "plain", None, None, None, geom)[0])
        assert torch.equal(out, _fused(dev, target, eps, z, tn, tp, "plain", None, None, geom)[0])
        outs.append(out)
    assert all(torch.equal(o, outs[0]) for o in outs)
    assert not torch.equal(eng.step(z, tn, tp), outs[0])


@pytest.mark.parametrize("cond_only", [False, True])
@pytest.mark.parametrize("target,g,hop", [("video", G.V["V1"], 2), ("audio", G.A["A1"], 20)], ids=["V1", "A1"])
def test_canvas_keyed_step_equals_explicit_noise(dev, model, cfg_rows, target, g, hop, cond_only):
    """test_gpu_canvas_noise.test_fused_step_equals_explicit_noise_*: the canvas-keyed draw inside the fused kernels at w = 8 / stride 2"""
    from multimodal_diffusion_amd import functional as Fn
    seed, off = 0xDEADBEEF12345678, 5
    z, zp, npr, kw = _case(dev, target, g, 3)
    assert g.lat[1] % hop == 0
    canvas = _engine(model[1], target, tuple(z.shape), npr, eta=0.5, noise_seed=seed, noise_keying="canvas", canvas_hop=hop,
                     sample_offset=off, **kw)
    plain = _engine(model[1], target, tuple(z.shape), npr, eta=0.5, **kw)
    for e in (canvas, plain):
        e.set_prompt(zp)
    tn, tp = ts(TN, dev), ts(TP, dev)
    noise = Fn.canvas_noise(seed, tn, tuple(z.shape), hop, window_offset=off)
    for rows in ((1, 0) if target == "video" else (1,)):
        cfg_rows(rows)
        a = canvas.step(z, tn, tp, cond_only=cond_only)
        assert torch.equal(a, plain.step(z, tn, tp, noise=noise, cond_only=cond_only))
        c = plain.step(z, tn, tp, noise=Fn.gaussian_noise(seed, off, tn, tuple(z.shape)), cond_only=cond_only)
        assert not torch.equal(a, c)                            # not the per-sample keying


@pytest.mark.parametrize("target,g", [("video", G.V["V9"]), ("audio", G.A["A2"])], ids=["V9", "A2"])
def test_graph_equals_eager(dev, model, target, g):
    z, zp, npr, kw = _case(dev, target, g, 2)
    eng = _engine(model[1], target, tuple(z.shape), npr, **kw)
    eng.set_prompt(zp)
    sched = R.sampling_schedule(1000, 4)
    zg = eng.run(z, sched, graph=True)
    ze = eng.run(z, sched, graph=False)
    assert torch.isfinite(zg).all() and torch.equal(zg, ze)
    assert not torch.equal(zg, z)


# ------------------------------------------------------------------------------------------------- 5. the config path
TOKENIZER = {"video": {"tube": {"t": 1, "h": 4, "w": 8}}, "audio": {"chunk": {"length": 4, "stride": 2}}}


@pytest.mark.parametrize("target", ["video", "audio"])
def test_sample_one_direction_follows_the_tokenizer_config(dev, model, target):
    """as test_entry_points_follow_the_config_key: the entry point's last decoded latent is the hand-driven engine's, bit for bit"""
    import multimodal_diffusion_amd as A
    vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=1.0, sampler_steps=2, size=(32, 64), tokenizer=TOKENIZER)
    vae, codec = Recorder(vae), Recorder(codec)
    kw = dict(components(model[1], vae, codec, dev), cfg=cfg)
    sched = A.schedule_utils.make_sampling_schedule(1000, 2)
    if target == "video":
        wav = (0.1 * torch.randn(16000, generator=torch.Generator().manual_seed(9))).numpy()
        lat = (1, 8, 4, 4, 8)                                   # 16 frames of 32 x 64: one tube row of 1 x 4 x 8 per frame
        noise = torch.randn(lat, generator=torch.Generator().manual_seed(4))
        A.sample_one_direction(init_noise=noise, prompt_modality="audio", prompt_video=None, prompt_audio=wav, **kw)
        got = vae.last.clone()
        with torch.no_grad():
            z_p = codec.encode(torch.from_numpy(wav).to(dev).view(1, 1, -1)).float()
        npr = (z_p.shape[-1] - 4) // 2 + 1
    else:
        vid = torch.randint(0, 256, (16, 32, 64, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).numpy()
        lat = (1, 8, 150)
        noise = torch.randn(lat, generator=torch.Generator().manual_seed(4))
        A.sample_one_direction(init_noise=noise, prompt_modality="video", prompt_video=vid, prompt_audio=None, **kw)
        got = codec.last.clone()
        with torch.no_grad():
            frames = torch.from_numpy(vid).to(dev).float() / 255.0
            z_p = vae.encode(frames.permute(3, 0, 1, 2).unsqueeze(0).contiguous()).float()
        assert tuple(z_p.shape) == (1, 8, 4, 4, 8)
        npr = 4
    eng = _engine(model[1], target, lat, npr, guidance=2.0, tube=(1, 4, 8), chunk=(4, 2))
    assert eng.embed.Nt == (4 if target == "video" else 74)
    eng.set_prompt(z_p)
    hand = eng.run(noise.to(dev), sched)
    assert torch.isfinite(got).all() and torch.equal(got, hand)
    # and the geometry matters: the default one gives another latent (video: a tube of 2 x 4 x 4 holds 256 values as well)
    other = _engine(model[1], target, lat, (z_p.shape[-1] - 4) // 4 + 1 if target == "video" else 4, guidance=2.0,
                    tube=(2, 4, 4) if target == "video" else (1, 4, 8))
    other.set_prompt(z_p)
    assert not torch.equal(other.run(noise.to(dev), sched), hand)


def test_stream_generate_follows_the_tokenizer_config(dev, model):
    """the video prompt direction: four windows of 8 frames of 32 x 64, each prompt latent [8, 2, 4, 8] in 2 tubes of 1 x 4 x 8, the
    audio target in 74 chunks of 4 / 2; the finished latents are those of one hand-driven engine over the four windows"""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import stream_infer as S
    vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=0.5, sampler_steps=2, size=(32, 64), streaming=STREAM_HALF_SECOND,
                               tokenizer=TOKENIZER)
    vid = torch.randint(0, 256, (20, 32, 64, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).numpy()
    noise = torch.randn(4, 8, 150, generator=torch.Generator().manual_seed(4))
    got = S.stream_generate(cfg=cfg, init_noise=noise, shard=False, return_latents=True, prompt_modality="video", prompt_video=vid,
                            prompt_audio=None, **components(model[1], vae, codec, dev))["latents"]
    chunks, _, _ = S.split_frames_into_windows(vid, fps=16, win_s=0.5, hop_s=0.25)
    with torch.no_grad():
        frames = torch.from_numpy(np.ascontiguousarray(chunks)).to(dev).float() / 255.0
        z_p = vae.encode(frames.permute(0, 4, 1, 2, 3).contiguous()).float()
    assert tuple(z_p.shape) == (4, 8, 2, 4, 8)
    eng = _engine(model[1], "audio", (4, 8, 150), 2, guidance=2.0, tube=(1, 4, 8), chunk=(4, 2))
    eng.set_prompt(z_p)
    hand = eng.run(noise.to(dev), A.schedule_utils.make_sampling_schedule(1000, 2))
    assert np.isfinite(got).all() and np.array_equal(got, hand.cpu().numpy())


# ------------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(dev):
    """through the Python wrappers, and for F < len also at the C entries; nothing is launched"""
    from multimodal_diffusion_amd import _lib as L, functional as Fn
    z = torch.randn(1, 8, 4, 8, 32, device=dev)
    with pytest.raises(AssertionError, match="tube sizes must divide latent dims"):
        Fn.tube_patch(z, 3, 4, 4)
    with pytest.raises(AssertionError, match="tube sizes must divide latent dims"):
        Fn.tube_patch(z, 2, 4, 12)
    with pytest.raises(L.AvdError, match="w=2 must be a multiple of 4"):
        Fn.tube_patch(z, 2, 4, 2)
    with pytest.raises(L.AvdError, match="w=2 must be a multiple of 4"):
        Fn.tube_unpatch(torch.randn(1, 2 * 2 * 16, 8 * 2 * 4 * 2, device=dev), 8, 4, 8, 32, 2, 4, 2)
    # F < len: the wrapper refuses in the entry's words before it allocates; the entries themselves refuse without a launch
    za = torch.randn(1, 8, 3, device=dev)
    with pytest.raises(L.AvdError, match="need 0 < len <= F"):
        Fn.audio_tokens(za, 4, 4)
    tok = torch.full((1, 18, 32), 7.0, device=dev)
    assert L.lib().avd_audio_tokens_f32(za.data_ptr(), tok.data_ptr(), 1, 8, 3, 4, 4, L.stream_ptr(dev)) == L.EUNSUPPORTED
    assert "need 0 < len <= F" in L.lib().avd_last_error().decode()
    out = torch.full((1, 8, 3), 7.0, device=dev)
    assert L.lib().avd_audio_untokens_f32(tok.data_ptr(), None, out.data_ptr(), 1, 8, 3, 4, 4, L.stream_ptr(dev)) == L.EUNSUPPORTED
    assert "audio_untokens: bad chunking" in L.lib().avd_last_error().decode()
    torch.cuda.synchronize()
    assert bool((tok == 7.0).all()) and bool((out == 7.0).all())       # nothing was launched
    # (40, 4, 2) makes 19 tokens
    with pytest.raises(L.AvdError, match="token count does not match"):
        Fn.audio_untokens(tok, 8, 4, 40, 2)
    with pytest.raises(L.AvdError, match="token count does not match"):
        Fn.audio_untokens(tok, 8, 4, 3, 2)                      # F < len
