"""DPM-Solver++(2M) on the MI355X (include/avdiff_hip.h, avd_dpmpp_2m_step_f32): the elementwise update against the fp32 numpy mirror
(edge cases included), the fused CFG + un-patch / overlap-add + DPM kernels against explicit computation from the step's own eps
tokens (both video kernel forms, audio, split streams), the first-order step against DDIM, graph replay against eager launches,
trajectories against the CPU oracle driven by the fp64 reference, batch invariance of stream_generate, and misuse."""
import numpy as np
import pytest
import torch

import _dpm_ref as D
from _tune import cfg_rows  # noqa: F401  (fixture)
from conftest import rel_err
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
ABAR = R.alpha_bar_table(R.beta_table(1000))
G = 3.0


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def model(dev):
    import multimodal_diffusion_amd as A
    ws = R.synth_weights(seed=0, n_layers=2)
    core = A.MMDiT(d_model=512, n_layers=2, n_heads=8, mlp_ratio=4.0).eval()
    core.load_state_dict(ws["core"], strict=True)
    head = A.MultiModalNoiseHead({"video": 512, "audio": 512}, {"video": 256, "audio": 32}, hidden_dim=512).eval()
    head.load_state_dict(ws["head"], strict=True)
    av, aa = A.LinearAdapter(256, 256), A.LinearAdapter(32, 256)
    av.load_state_dict(ws["adapt_v"])
    aa.load_state_dict(ws["adapt_a"])
    return ws, tuple(m.to(dev) for m in (core, head, av, aa))


def _engine(model, target, shape, n_prompt, **kw):
    import multimodal_diffusion_amd as A
    _, (core, head, av, aa) = model
    return A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=256, target=target, latent_shape=shape,
                           prompt_tokens=n_prompt, alpha_bar=ABAR, guidance=G, **kw)


def _video_case(dev, B=2, W=32, seed=0):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, 8, 4, 16, W, generator=g).to(dev)
    za = torch.randn(B, 8, 40, generator=g).to(dev)           # 10 prompt tokens (chunk 4, stride 4)
    return z, za, 10


def _audio_case(dev, B=2, seed=1):
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, 8, 40, generator=g).to(dev)
    zv = torch.randn(B, 8, 4, 8, 8, generator=g).to(dev)      # 8 prompt tokens (tube 2 x 4 x 4)
    return z, zv, 8


def _t(v, dev):
    return torch.tensor(v, dtype=torch.long, device=dev)


# ------------------------------------------------------------------------------------------------- elementwise update = fp32 mirror
def test_elementwise_step_matches_fp32_mirror(dev):
    from multimodal_diffusion_amd import functional as Fn
    abar = ABAR.clone()
    abar[5] = 1.0                                             # an a = 1.0f entry: sigma = 0
    # (t_last, t_now, t_prev): first step, second order, final step, non-decreasing history, t_now = 0 final, a_t = 1 (first
    # order), a_s = 1 (returns x0), second order, equal lambdas (first order), t_now = T-1 with a history at or above it (first
    # order), second order
    cases = [(-1, 999, 950), (999, 950, 900), (600, 500, -1), (0, 999, 950), (300, 0, -1), (40, 20, 5), (10, 5, 2),
             (200, 100, 60), (100, 100, 60), (999, 999, 980), (1200, 999, 980), (500, 400, 300)]
    tl, tn, tp = (np.array(c) for c in zip(*cases))
    B, per = len(cases), 4099                                 # not a multiple of 4
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, per, generator=g)
    e = torch.randn(B, per, generator=g)
    h = torch.randn(B, per, generator=g)
    cx, c0, c1 = D.coefs(abar.numpy(), tl, tn, tp)
    first = torch.from_numpy(c1 == 0)
    h[first] = float("nan")                                   # a first-order step never reads its history
    assert (~first).sum() >= 3 and first.sum() >= 6
    hd = h.to(dev)
    out = Fn.dpmpp_2m_step(x.to(dev), e.to(dev), hd, _t(tl, dev), _t(tn, dev), _t(tp, dev), abar)
    ref, x0 = D.step_f32(x.numpy(), e.numpy(), h.numpy(), abar.numpy(), tl, tn, tp)
    out = out.cpu()
    assert torch.isfinite(out).all() and torch.isfinite(hd).all()
    assert rel_err(out, torch.from_numpy(ref)) <= 1e-6
    assert torch.equal(hd.cpu(), torch.from_numpy(x0))
    # where the mirror returns x0_s (final step, a_t = 1, a_s = 1) the kernel does so bit for bit
    for i in (2, 4, 5, 6):
        assert torch.equal(out[i], torch.from_numpy(x0[i]))


# ------------------------------------------------------------------------------------------------- fused step = explicit
def _explicit(eng, z, h0, tl, tn, tp, target):
    """the step's eps tokens -> CFG combine -> un-patch / overlap-add (oracle) -> the fp32 mirror update"""
    tok = eng.eps_tokens().cpu()
    B = z.shape[0]
    e_tok = tok[B:] + G * (tok[:B] - tok[B:])
    zc = z.cpu()
    if target == "video":
        eps = R.tube_unpatch(e_tok, *zc.shape[1:], 2, 4, 4)
    else:
        eps = R.audio_untokens(e_tok, zc.shape[1], 4, zc.shape[2], 4)
    return D.step_f32(zc.numpy(), eps.numpy(), h0.cpu().numpy(), ABAR.numpy(), tl, tn, tp)


TL, TN, TP = [-1, 981, 700], [981, 402, 40], [961, 382, -1]      # first order, second order, final step


def test_fused_step_video_both_forms(dev, model, cfg_rows):
    z, za, npr = _video_case(dev, B=3)
    h0 = torch.randn(z.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    outs = []
    for rows in (1, 0):
        cfg_rows(rows)
        eng = _engine(model, "video", tuple(z.shape), npr, solver="dpmpp_2m")
        eng.set_prompt(za)
        eng.x0_hist.copy_(h0)
        out = eng.step(z, _t(TN, dev), _t(TP, dev), t_last=_t(TL, dev))
        ref, x0 = _explicit(eng, z, h0, TL, TN, TP, "video")
        assert rel_err(out.cpu(), torch.from_numpy(ref)) <= 1e-6
        assert rel_err(eng.x0_hist.cpu(), torch.from_numpy(x0)) <= 1e-6
        assert torch.isfinite(out).all()
        outs.append((out.clone(), eng.x0_hist.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])     # rows form == gather form


def test_fused_step_audio(dev, model):
    z, zv, npr = _audio_case(dev, B=3)
    h0 = torch.randn(z.shape, generator=torch.Generator().manual_seed(8)).to(dev)
    eng = _engine(model, "audio", tuple(z.shape), npr, solver="dpmpp_2m")
    eng.set_prompt(zv)
    eng.x0_hist.copy_(h0)
    out = eng.step(z, _t(TN, dev), _t(TP, dev), t_last=_t(TL, dev))
    ref, x0 = _explicit(eng, z, h0, TL, TN, TP, "audio")
    assert rel_err(out.cpu(), torch.from_numpy(ref)) <= 1e-6
    assert rel_err(eng.x0_hist.cpu(), torch.from_numpy(x0)) <= 1e-6


def test_fused_step_split_streams_f16x2(dev, model):
    z, za, npr = _video_case(dev, B=2)
    tl, tn, tp = [999, 720], [700, 300], [680, 280]
    h0 = torch.randn(z.shape, generator=torch.Generator().manual_seed(9)).to(dev)
    eng = _engine(model, "video", tuple(z.shape), npr, solver="dpmpp_2m", matmul="f16x2", split_streams=True)
    eng.set_prompt(za)
    eng.x0_hist.copy_(h0)
    out = eng.step(z, _t(tn, dev), _t(tp, dev), t_last=_t(tl, dev))
    ref, _ = _explicit(eng, z, h0, tl, tn, tp, "video")
    assert rel_err(out.cpu(), torch.from_numpy(ref)) <= 1e-6


# ------------------------------------------------------------------------------------------------- against DDIM
@pytest.mark.parametrize("target", ["video", "audio"])
def test_first_order_step_and_one_step_trajectory_match_ddim(dev, model, target):
    z, zp, npr = _video_case(dev, B=2) if target == "video" else _audio_case(dev, B=2)
    dpm = _engine(model, target, tuple(z.shape), npr, solver="dpmpp_2m")
    ddim = _engine(model, target, tuple(z.shape), npr)
    for e in (dpm, ddim):
        e.set_prompt(zp)
    tn, tp = _t([999, 500], dev), _t([950, 450], dev)
    a = dpm.step(z, tn, tp)                                   # t_last = None: first order
    b = ddim.step(z, tn, tp)
    assert rel_err(a.cpu(), b.cpu()) <= 2e-6
    sched = R.sampling_schedule(1000, 1)                      # [999, -1]: both return x0_s
    assert torch.equal(dpm.run(z, sched), ddim.run(z, sched))


# ------------------------------------------------------------------------------------------------- graph = eager
@pytest.mark.parametrize("n_steps", [5, 6])
def test_graph_equals_eager(dev, model, n_steps):
    z, za, npr = _video_case(dev, B=2)
    sched = R.sampling_schedule(1000, n_steps)
    eng = _engine(model, "video", tuple(z.shape), npr, solver="dpmpp_2m")
    eng.set_prompt(za)
    zg = eng.run(z, sched, graph=True)
    ze = eng.run(z, sched, graph=False)
    assert torch.equal(zg, ze)
    assert torch.equal(eng.run(z, sched, graph=True), zg)     # a second run starts first order again: no stale history
    # explicit steps with the history passed by hand land on the same bits
    eng2 = _engine(model, "video", tuple(z.shape), npr, solver="dpmpp_2m")
    eng2.set_prompt(za)
    x = z.clone()
    for i in range(n_steps):
        tl = None if i == 0 else _t([int(sched[i - 1])] * 2, dev)
        x = eng2.step(x, _t([int(sched[i])] * 2, dev), _t([int(sched[i + 1])] * 2, dev), t_last=tl)
    assert torch.equal(x, zg)
    ddim = _engine(model, "video", tuple(z.shape), npr)
    ddim.set_prompt(za)
    assert not torch.equal(ddim.run(z, sched), zg)             # the second-order steps are live


# ------------------------------------------------------------------------------------------------- trajectory vs the oracle
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_trajectory_vs_oracle(dev, model, target, mode):
    ws, _ = model
    n_steps = 8
    sched = R.sampling_schedule(1000, n_steps)
    if target == "video":
        z, zp, npr = _video_case(dev, B=2, W=16)
    else:
        z, zp, npr = _audio_case(dev, B=2)
    eng = _engine(model, target, tuple(z.shape), npr, solver="dpmpp_2m", matmul=mode)
    eng.set_prompt(zp)
    out = eng.run(z, sched).cpu().double()
    x, p = z.cpu(), zp.cpu()
    hist, t_last = np.zeros(tuple(x.shape)), -1
    kw = dict(adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"], head=ws["head"], n_layers=2, n_heads=8, guidance=G,
              eta=0.0, return_eps=True)
    for i in range(n_steps):
        tn, tp = sched[i].repeat(2), sched[i + 1].repeat(2)
        if target == "video":
            _, eps_tok = R.denoise_step_a2v(x, p, tn, tp, ABAR, **kw)
            eps = R.tube_unpatch(eps_tok, *x.shape[1:], 2, 4, 4)
        else:
            _, eps_tok = R.denoise_step_v2a(x, p, tn, tp, ABAR, **kw)
            eps = R.audio_untokens(eps_tok, x.shape[1], 4, x.shape[2], 4)
        y, hist = D.step_f64(x.numpy(), eps.numpy(), hist, ABAR.numpy(), [t_last] * 2, tn.numpy(), tp.numpy())
        x, t_last = torch.from_numpy(y).float(), int(sched[i])
    ref = x.double()
    assert float((out - ref).norm() / ref.norm()) < 1e-3


# ------------------------------------------------------------------------------------------------- batch invariance
def test_stream_generate_batch_invariance(dev, model):
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import stream_infer as S
    _, (core, head, av, aa) = model
    prev = core.matmul, head.matmul
    core.matmul = head.matmul = "f32"     # one kernel family whatever the batch (the "auto" rule switches at 2,048 / 6,144 rows)
    try:
        torch.manual_seed(8)
        vae = A.VideoVAE.from_config({"latent": {"channels": 8, "t_down": 4, "s_down": 8}}).eval().to(dev)
        codec = A.AudioCodec.from_config({"sr": 16000, "latent": {"channels": 8, "frames_per_clip": 150},
                                          "codec": {"hop_samples": 320}}).eval().to(dev)
        cfg = {"tokenizer": {"width": 512, "video": {"tube": {"t": 2, "h": 4, "w": 4}}, "audio": {"chunk": {"length": 4, "stride": 4}}},
               "video": {"fps": 16, "size": [32, 32], "latent": {"channels": 8, "t_down": 4, "s_down": 8}},
               "audio": {"sr": 16000, "latent": {"channels": 8, "frames_per_clip": 150}},
               "data": {"clip_seconds": 0.5}, "streaming": {"window_seconds": 0.5, "hop_seconds": 0.25, "crossfade_seconds": 0.125},
               "diffusion": {m: {"steps": 1000, "sampler_steps": 4, "schedule": "cosine", "min_beta": 1e-4, "max_beta": 0.02}
                             for m in ("video", "audio")},
               "sampling": {"solver": "dpmpp_2m", "guidance_scale": {"video": 2.0, "audio": 2.0}}}
        wav = (0.1 * torch.randn(18000, generator=torch.Generator().manual_seed(9))).numpy()      # 4 windows
        kw = dict(cfg=cfg, vid_vae=vae, aud_codec=codec, adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=256, device=dev,
                  prompt_modality="audio", prompt_video=None, prompt_audio=wav, seed=10)
        whole = S.stream_generate(shard=False, **kw)
        per_window = S.stream_generate(shard=False, max_windows_per_batch=1, **kw)
        assert np.array_equal(whole["video"], per_window["video"])
        ddim = S.stream_generate(shard=False, **dict(kw, cfg=dict(cfg, sampling={"guidance_scale": cfg["sampling"]["guidance_scale"]})))
        assert not np.array_equal(ddim["video"], whole["video"])       # the config key selects the solver
    finally:
        core.matmul, head.matmul = prev


# ------------------------------------------------------------------------------------------------- misuse
def test_misuse(dev, model):
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd import _lib as L
    z, za, npr = _video_case(dev, B=2)
    eng = _engine(model, "video", tuple(z.shape), npr, solver="dpmpp_2m")
    eng.set_prompt(za)
    tn, tp = _t([900, 900], dev), _t([800, 800], dev)
    eng.x0_hist.copy_(z)
    with pytest.raises(L.AvdError):
        eng.step(eng.x0_hist, tn, tp)
    with pytest.raises(L.AvdError):
        eng.step(z, tn, tp, out=eng.x0_hist)
    with pytest.raises(ValueError):
        eng.step(z, tn, tp, noise=torch.randn_like(z))
    for bad in ([999, 500, 500, -1], [999, 200, 500, -1]):
        with pytest.raises(ValueError, match="decreasing"):
            eng.run(z, torch.tensor(bad))
    x = torch.randn(2, 64, device=dev)
    with pytest.raises(ValueError, match="x0_hist"):
        Fn.dpmpp_2m_step(x, torch.randn_like(x), x, tn, tn, tp, ABAR)
    with pytest.raises(ValueError):
        _engine(model, "video", tuple(z.shape), npr, solver="dpmpp_2m", eta=0.5)
    ddim = _engine(model, "video", tuple(z.shape), npr)
    ddim.set_prompt(za)
    with pytest.raises(ValueError):
        ddim.step(z, tn, tp, t_last=tn)
    assert ddim.x0_hist is None and isinstance(eng, A.DenoiseEngine)
