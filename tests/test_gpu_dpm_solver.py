"""DPM-Solver++(2M) on the MI355X (include/avdiff_hip.h, avd_dpmpp_2m_step_f32): the elementwise update against the fp32 numpy mirror
(edge cases included), the fused CFG + un-patch / overlap-add + DPM kernels against explicit computation from the step's own eps
tokens (both video kernel forms, audio, split streams), the first-order step against DDIM, graph replay against eager launches,
trajectories against the CPU oracle driven by the fp64 reference, batch invariance of stream_generate, and misuse."""
from functools import partial

import numpy as np
import pytest
import torch

import _dpm_ref as D
from _kit import (ABAR, STREAM_HALF_SECOND, audio_case, audio_prompt, components, dev, engine, matmul_f32, model,  # noqa: F401  (dev / model are fixtures)
                  pipeline, ts, video_case)
from _tune import cfg_rows  # noqa: F401  (fixture)
from conftest import rel_err
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
G = 3.0
_engine = partial(engine, guidance=G)        # engine(mods, target, shape, n_prompt, **kw) at this file's guidance


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
    out = Fn.dpmpp_2m_step(x.to(dev), e.to(dev), hd, ts(tl, dev), ts(tn, dev), ts(tp, dev), abar)
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
    z, za, npr = video_case(dev, B=3)
    h0 = torch.randn(z.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    outs = []
    for rows in (1, 0):
        cfg_rows(rows)
        eng = _engine(model[1], "video", tuple(z.shape), npr, solver="dpmpp_2m")
        eng.set_prompt(za)
        eng.x0_hist.copy_(h0)
        out = eng.step(z, ts(TN, dev), ts(TP, dev), t_last=ts(TL, dev))
        ref, x0 = _explicit(eng, z, h0, TL, TN, TP, "video")
        assert rel_err(out.cpu(), torch.from_numpy(ref)) <= 1e-6
        assert rel_err(eng.x0_hist.cpu(), torch.from_numpy(x0)) <= 1e-6
        assert torch.isfinite(out).all()
        outs.append((out.clone(), eng.x0_hist.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])     # rows form == gather form


def test_fused_step_audio(dev, model):
    z, zv, npr = audio_case(dev, B=3)
    h0 = torch.randn(z.shape, generator=torch.Generator().manual_seed(8)).to(dev)
    eng = _engine(model[1], "audio", tuple(z.shape), npr, solver="dpmpp_2m")
    eng.set_prompt(zv)
    eng.x0_hist.copy_(h0)
    out = eng.step(z, ts(TN, dev), ts(TP, dev), t_last=ts(TL, dev))
    ref, x0 = _explicit(eng, z, h0, TL, TN, TP, "audio")
    assert rel_err(out.cpu(), torch.from_numpy(ref)) <= 1e-6
    assert rel_err(eng.x0_hist.cpu(), torch.from_numpy(x0)) <= 1e-6


def test_fused_step_split_streams_f16x2(dev, model):
    z, za, npr = video_case(dev, B=2)
    tl, tn, tp = [999, 720], [700, 300], [680, 280]
    h0 = torch.randn(z.shape, generator=torch.Generator().manual_seed(9)).to(dev)
    eng = _engine(model[1], "video", tuple(z.shape), npr, solver="dpmpp_2m", matmul="f16x2", split_streams=True)
    eng.set_prompt(za)
    eng.x0_hist.copy_(h0)
    out = eng.step(z, ts(tn, dev), ts(tp, dev), t_last=ts(tl, dev))
    ref, _ = _explicit(eng, z, h0, tl, tn, tp, "video")
    assert rel_err(out.cpu(), torch.from_numpy(ref)) <= 1e-6


# ------------------------------------------------------------------------------------------------- against DDIM
@pytest.mark.parametrize("target", ["video", "audio"])
def test_first_order_step_and_one_step_trajectory_match_ddim(dev, model, target):
    z, zp, npr = video_case(dev, B=2) if target == "video" else audio_case(dev, B=2)
    dpm = _engine(model[1], target, tuple(z.shape), npr, solver="dpmpp_2m")
    ddim = _engine(model[1], target, tuple(z.shape), npr)
    for e in (dpm, ddim):
        e.set_prompt(zp)
    tn, tp = ts([999, 500], dev), ts([950, 450], dev)
    a = dpm.step(z, tn, tp)                                   # t_last = None: first order
    b = ddim.step(z, tn, tp)
    assert rel_err(a.cpu(), b.cpu()) <= 2e-6
    sched = R.sampling_schedule(1000, 1)                      # [999, -1]: both return x0_s
    assert torch.equal(dpm.run(z, sched), ddim.run(z, sched))


# ------------------------------------------------------------------------------------------------- graph = eager
@pytest.mark.parametrize("n_steps", [5, 6])
def test_graph_equals_eager(dev, model, n_steps):
    z, za, npr = video_case(dev, B=2)
    sched = R.sampling_schedule(1000, n_steps)
    eng = _engine(model[1], "video", tuple(z.shape), npr, solver="dpmpp_2m")
    eng.set_prompt(za)
    zg = eng.run(z, sched, graph=True)
    ze = eng.run(z, sched, graph=False)
    assert torch.equal(zg, ze)
    assert torch.equal(eng.run(z, sched, graph=True), zg)     # a second run starts first order again: no stale history
    # explicit steps with the history passed by hand land on the same bits
    eng2 = _engine(model[1], "video", tuple(z.shape), npr, solver="dpmpp_2m")
    eng2.set_prompt(za)
    x = z.clone()
    for i in range(n_steps):
        tl = None if i == 0 else ts([int(sched[i - 1])] * 2, dev)
        x = eng2.step(x, ts([int(sched[i])] * 2, dev), ts([int(sched[i + 1])] * 2, dev), t_last=tl)
    assert torch.equal(x, zg)
    ddim = _engine(model[1], "video", tuple(z.shape), npr)
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
        z, zp, npr = video_case(dev, B=2, W=16)
    else:
        z, zp, npr = audio_case(dev, B=2)
    eng = _engine(model[1], target, tuple(z.shape), npr, solver="dpmpp_2m", matmul=mode)
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
    from multimodal_diffusion_amd import stream_infer as S
    with matmul_f32(model[1]):            # one kernel family whatever the batch (the "auto" rule switches at 2,048 / 6,144 rows)
        vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND,
                                   sampling={"solver": "dpmpp_2m"})
        kw = dict(components(model[1], vae, codec, dev), cfg=cfg, **audio_prompt())                # 4 windows
        whole = S.stream_generate(shard=False, **kw)
        per_window = S.stream_generate(shard=False, max_windows_per_batch=1, **kw)
        assert np.array_equal(whole["video"], per_window["video"])
        ddim = S.stream_generate(shard=False, **dict(kw, cfg=dict(cfg, sampling={"guidance_scale": cfg["sampling"]["guidance_scale"]})))
        assert not np.array_equal(ddim["video"], whole["video"])       # the config key selects the solver


# ------------------------------------------------------------------------------------------------- misuse
def test_misuse(dev, model):
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd import _lib as L
    z, za, npr = video_case(dev, B=2)
    eng = _engine(model[1], "video", tuple(z.shape), npr, solver="dpmpp_2m")
    eng.set_prompt(za)
    tn, tp = ts([900, 900], dev), ts([800, 800], dev)
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
        _engine(model[1], "video", tuple(z.shape), npr, solver="dpmpp_2m", eta=0.5)
    ddim = _engine(model[1], "video", tuple(z.shape), npr)
    ddim.set_prompt(za)
    with pytest.raises(ValueError):
        ddim.step(z, tn, tp, t_last=tn)
    assert ddim.x0_hist is None and isinstance(eng, A.DenoiseEngine)
