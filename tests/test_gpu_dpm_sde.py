"""SDE-DPM-Solver++(2M) on the MI355X (include/avdiff_hip.h, avd_dpmpp_2m_sde_step_f32): the elementwise update against the fp32 numpy
mirror (edge cases included), the fused kernels — per-sample and canvas-keyed, both video forms and both rows tiles, audio, split
streams — against explicit computation from the step's own eps tokens and the device stream's normals, the compositions with the latent
guide, the CFG control and the cond-only step, the first-order step against seeded DDIM at eta = 1, graph replay against eager
launches, split invariance, window consensus at eta > 0, trajectories against the CPU oracle driven by the fp64 reference,
stream_generate, and misuse."""
from functools import partial

import numpy as np
import pytest
import torch

import _canvas_noise_ref as CN
import _consensus_ref as W
import _dpm_sde_ref as S
import _geom
import _noise_ref as NR
from _kit import (ABAR, STREAM_HALF_SECOND, audio_case, audio_prompt, components, dev, engine, matmul_f32, model,  # noqa: F401  (dev / model are fixtures)
                  pipeline, soft_mask, ts, video_case)
from _tune import cfg_rows  # noqa: F401  (fixture)
from conftest import rel_err
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
G, ETA, SEED, GSEED = 3.0, 0.7, 0xDEADBEEF12345678, 77
_engine = partial(engine, guidance=G)        # engine(mods, target, shape, n_prompt, **kw) at this file's guidance


def _sde(model, target, shape, n_prompt, eta=ETA, **kw):
    return _engine(model[1], target, shape, n_prompt, solver="dpmpp_2m", eta=eta, noise_seed=SEED, **kw)


def _canvas(model, target, shape, n_prompt, hop, eta=ETA, **kw):
    return _sde(model, target, shape, n_prompt, eta, noise_keying="canvas", canvas_hop=hop, **kw)


def _h0(z, seed=7):
    return torch.randn(z.shape, generator=torch.Generator().manual_seed(seed)).to(z.device)


def _noise(eng, tn, shape):
    """the normals the engine's fused step draws, from the device's noise kernels"""
    from multimodal_diffusion_amd import functional as Fn
    if eng.canvas_hop is not None:
        return Fn.canvas_noise(SEED, tn, shape, eng.canvas_hop, window_offset=eng.sample_offset)
    return Fn.gaussian_noise(SEED, eng.sample_offset, tn, shape)


# ------------------------------------------------------------------------------------------------- elementwise update = fp32 mirror
def test_elementwise_step_matches_fp32_mirror(dev):
    from multimodal_diffusion_amd import functional as Fn
    abar = ABAR.clone()
    abar[5] = 1.0                                             # an a = 1.0f entry: sigma = 0
    # the 12 cases of test_gpu_dpm_solver.py::test_elementwise_step_matches_fp32_mirror
    cases = [(-1, 999, 950), (999, 950, 900), (600, 500, -1), (0, 999, 950), (300, 0, -1), (40, 20, 5), (10, 5, 2),
             (200, 100, 60), (100, 100, 60), (999, 999, 980), (1200, 999, 980), (500, 400, 300)]
    tl, tn, tp = (np.array(c) for c in zip(*cases))
    B, per = len(cases), 4099                                 # not a multiple of 4
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, per, generator=g)
    e = torch.randn(B, per, generator=g)
    h = torch.randn(B, per, generator=g)
    first = torch.from_numpy(D_first(abar, tl, tn, tp))
    h[first] = float("nan")                                   # a first-order step never reads its history
    assert (~first).sum() >= 3 and first.sum() >= 6
    noise = Fn.gaussian_noise(SEED, 3, ts(tn, dev), (B, per))
    for eta in (0.3, 1.0):
        hd = h.to(dev)
        out = Fn.dpmpp_2m_sde_step(x.to(dev), e.to(dev), hd, ts(tl, dev), ts(tn, dev), ts(tp, dev), abar, eta, noise).cpu()
        ref, x0 = S.step_f32(x.numpy(), e.numpy(), h.numpy(), abar.numpy(), tl, tn, tp, eta, noise.cpu().numpy())
        assert torch.isfinite(out).all() and torch.isfinite(hd).all()
        assert rel_err(out, torch.from_numpy(ref)) <= 1e-6
        assert torch.equal(hd.cpu(), torch.from_numpy(x0))
        for i in (2, 4, 5, 6):                                # final step, a_t = 1, a_s = 1: x0_s bit for bit
            assert torch.equal(out[i], torch.from_numpy(x0[i]))
        ode = Fn.dpmpp_2m_step(x.to(dev), e.to(dev), h.to(dev), ts(tl, dev), ts(tn, dev), ts(tp, dev), abar).cpu()
        assert not torch.equal(out[1], ode[1])                # the noise term is live
    # eta == 0: the ODE entry's bits, and the noise is not read
    h_sde, h_ode = h.to(dev), h.to(dev)
    nan = torch.full((B, per), float("nan"), device=dev)
    a = Fn.dpmpp_2m_sde_step(x.to(dev), e.to(dev), h_sde, ts(tl, dev), ts(tn, dev), ts(tp, dev), abar, 0.0, nan)
    b = Fn.dpmpp_2m_step(x.to(dev), e.to(dev), h_ode, ts(tl, dev), ts(tn, dev), ts(tp, dev), abar)
    assert torch.equal(a, b) and torch.equal(h_sde, h_ode)
    assert torch.equal(Fn.dpmpp_2m_sde_step(x.to(dev), e.to(dev), h.to(dev), ts(tl, dev), ts(tn, dev), ts(tp, dev), abar, 0.0), b)


def D_first(abar, tl, tn, tp):
    """which of the cases are first order (the same at every eta: the conditions are the ODE solver's)"""
    c1 = S.coefs(abar.numpy(), tl, tn, tp, 0.5)[2]
    assert np.array_equal(c1 == 0, S.coefs(abar.numpy(), tl, tn, tp, 0.0)[2] == 0)
    return c1 == 0


# ------------------------------------------------------------------------------------------------- fused step = explicit
def _explicit(eng, z, h0, tl, tn, tp, target, tube=(2, 4, 4), chunk=(4, 4)):
    """the step's eps tokens -> CFG combine -> un-patch / overlap-add (oracle) -> the fp32 mirror update on the device stream's normals"""
    tok = eng.eps_tokens().cpu()
    B = z.shape[0]
    e_tok = tok[B:] + G * (tok[:B] - tok[B:])
    zc = z.cpu()
    if target == "video":
        eps = R.tube_unpatch(e_tok, *zc.shape[1:], *tube)
    else:
        eps = R.audio_untokens(e_tok, zc.shape[1], chunk[0], zc.shape[2], chunk[1])
    noise = _noise(eng, ts(tn, z.device), tuple(z.shape)).cpu().numpy()
    return S.step_f32(zc.numpy(), eps.numpy(), h0.cpu().numpy(), ABAR.numpy(), tl, tn, tp, eng.eta, noise)


TL, TN, TP = [-1, 981, 700], [981, 402, 40], [961, 382, -1]      # first order, second order, final step


def _check_fused(eng, z, zp, target, tl=TL, tn=TN, tp=TP, **geom):
    dev_ = z.device
    eng.set_prompt(zp)
    h0 = _h0(z)
    eng.x0_hist.copy_(h0)
    out = eng.step(z, ts(tn, dev_), ts(tp, dev_), t_last=ts(tl, dev_))
    ref, x0 = _explicit(eng, z, h0, tl, tn, tp, target, **geom)
    assert torch.isfinite(out).all()
    assert rel_err(out.cpu(), torch.from_numpy(ref)) <= 1e-6
    assert rel_err(eng.x0_hist.cpu(), torch.from_numpy(x0)) <= 1e-6
    return out.clone(), eng.x0_hist.clone()


@pytest.mark.parametrize("keying", ["sample", "canvas"])
def test_fused_step_video_both_forms(dev, model, cfg_rows, keying):
    z, za, npr = video_case(dev, B=3)
    outs = []
    for rows in (1, 0):
        cfg_rows(rows)
        if keying == "sample":
            eng = _sde(model, "video", tuple(z.shape), npr, sample_offset=5)
        else:                                                 # N = 3 windows, canvas_hop = L / 2, sample_offset > 0
            eng = _canvas(model, "video", tuple(z.shape), npr, 2, sample_offset=4)
        # windows of a canvas share their timesteps in use; the kernel reads t_now[b] per window and is checked with distinct ones
        outs.append(_check_fused(eng, z, za, "video"))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])     # rows form == gather form
    # the ODE step from the same state differs: the noise term is live
    ode = _engine(model[1], "video", tuple(z.shape), npr, solver="dpmpp_2m")
    ode.set_prompt(za)
    ode.x0_hist.copy_(_h0(z))
    assert not torch.equal(ode.step(z, ts(TN, dev), ts(TP, dev), t_last=ts(TL, dev))[:2], outs[0][0][:2])


@pytest.mark.parametrize("keying", ["sample", "canvas"])
def test_fused_step_video_other_rows_tile(dev, model, cfg_rows, keying):
    """V1 of _geom.py: tube 1 x 4 x 8 takes the 4-token rows tile (the kit's default geometry takes 8)"""
    geo = _geom.V["V1"]
    assert geo.form == "rows4" and geo.D == 256
    g = torch.Generator().manual_seed(2)
    z, za = torch.randn(3, *geo.lat, generator=g).to(dev), torch.randn(3, 8, 40, generator=g).to(dev)
    outs = []
    for rows in (1, 0):
        cfg_rows(rows)
        kw = dict(tube=geo.tube, sample_offset=1)
        eng = _sde(model, "video", tuple(z.shape), 10, **kw) if keying == "sample" else _canvas(model, "video", tuple(z.shape), 10, 2, **kw)
        outs.append(_check_fused(eng, z, za, "video", tube=geo.tube))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("keying", ["sample", "canvas"])
def test_fused_step_audio(dev, model, keying):
    z, zv, npr = audio_case(dev, B=3)
    if keying == "sample":
        eng = _sde(model, "audio", tuple(z.shape), npr, sample_offset=2)
    else:
        eng = _canvas(model, "audio", tuple(z.shape), npr, 20, sample_offset=3)
    _check_fused(eng, z, zv, "audio")


def test_fused_step_split_streams_f16x2(dev, model):
    z, za, npr = video_case(dev, B=2)
    eng = _sde(model, "video", tuple(z.shape), npr, matmul="f16x2", split_streams=True)
    _check_fused(eng, z, za, "video", tl=[999, 720], tn=[700, 300], tp=[680, 280])


# ------------------------------------------------------------------------------------------------- compositions
def _untok(eng, tok):
    from multimodal_diffusion_amd import functional as Fn
    if eng.target == "video":
        return Fn.tube_unpatch(tok.contiguous(), *eng.latent_shape[1:], *eng.tube)
    return Fn.audio_untokens(tok.contiguous(), eng.latent_shape[1], eng.chunk[0], eng.latent_shape[2], eng.chunk[1])


def _composed(eng, z, eps, h0, tl, tn, tp):
    """the elementwise SDE update on latent-layout eps with the normals of the engine's keying: (z_out, x0_hist)"""
    from multimodal_diffusion_amd import functional as Fn
    h = h0.clone()
    out = Fn.dpmpp_2m_sde_step(z, eps, h, tl, tn, tp, ABAR, eng.eta, _noise(eng, tn, tuple(z.shape)))
    return out, h


@pytest.mark.parametrize("target,keying", [("video", "sample"), ("video", "canvas"), ("audio", "sample")])
def test_guided_step_equals_composed(dev, model, target, keying):
    """A fractional mask: the bound of test_gpu_latent_guide.py::test_fused_equals_composed (seeded DDIM case) — bit for bit against the
    unguided step followed by Fn.latent_guide; x0_hist holds the model's x0."""
    from multimodal_diffusion_amd import functional as Fn
    z, zp, npr = video_case(dev, B=2) if target == "video" else audio_case(dev, B=2)
    known, soft = _h0(z, 4), soft_mask(tuple(z.shape[1:])).to(dev)
    eng = _sde(model, target, tuple(z.shape), npr) if keying == "sample" else _canvas(model, target, tuple(z.shape), npr, 2)
    eng.set_prompt(zp)
    tn, tp, tl = ts([981, 402], dev), ts([961, 382], dev), ts([999, 700], dev)
    h0 = _h0(z)
    eng.x0_hist.copy_(h0)
    base, hb = eng.step(z, tn, tp, t_last=tl).clone(), eng.x0_hist.clone()
    eng.set_known(known, soft, guide_seed=GSEED)
    eng.x0_hist.copy_(h0)
    out = eng.step(z, tn, tp, t_last=tl)
    assert torch.isfinite(out).all()
    assert torch.equal(out, Fn.latent_guide(known, tp, ABAR, z=base, mask=soft, seed=GSEED))
    assert torch.equal(eng.x0_hist, hb) and not torch.equal(out, base)
    # guide + cond-only: the single-branch eps through the elementwise update, then the blend
    eng.x0_hist.copy_(h0)
    outc = eng.step(z, tn, tp, t_last=tl, cond_only=True)
    ep = eng.eps_tokens()
    assert ep.shape[0] == z.shape[0]
    ref, href = _composed(eng, z, _untok(eng, ep), h0, tl, tn, tp)
    ref = Fn.latent_guide(known, tp, ABAR, z=ref, mask=soft, seed=GSEED)
    if target == "video":                                     # U is a permutation: the same arithmetic, bit for bit
        assert torch.equal(outc, ref) and torch.equal(eng.x0_hist, href)
    else:
        assert rel_err(outc.cpu(), ref.cpu()) <= 1e-6
    assert not torch.equal(outc, out)


@pytest.mark.parametrize("target,keying", [("video", "sample"), ("video", "canvas"), ("audio", "sample")])
def test_controlled_step_equals_composed(dev, model, target, keying):
    """Per-sample guidance with rescale: the bound of test_gpu_cfg_rescale.py's fused = composed check (relative L2 <= 1e-6) against
    eps tokens -> combine with g_b -> U -> Fn.cfg_rescale -> the elementwise SDE update."""
    from multimodal_diffusion_amd import functional as Fn
    g2, phi2 = [2.0, 5.0], [0.7, 0.3]
    z, zp, npr = video_case(dev, B=2) if target == "video" else audio_case(dev, B=2)
    kw = dict(guidance=g2, guidance_rescale=phi2)
    mk = partial(engine, model[1], target, tuple(z.shape), npr, solver="dpmpp_2m", eta=ETA, noise_seed=SEED)
    eng = mk(**kw) if keying == "sample" else mk(noise_keying="canvas", canvas_hop=2, **kw)
    eng.set_prompt(zp)
    tn, tp, tl = ts([981, 402], dev), ts([961, 382], dev), ts([999, 700], dev)
    h0 = _h0(z)
    eng.x0_hist.copy_(h0)
    out, hist = eng.step(z, tn, tp, t_last=tl).clone(), eng.x0_hist.clone()
    ep = eng.eps_tokens()
    ec, en = ep[:2], ep[2:]
    gt = torch.tensor(g2, device=dev).view(2, 1, 1)
    r = Fn.cfg_rescale(_untok(eng, ec), _untok(eng, en + gt * (ec - en)), phi2)
    ref, href = _composed(eng, z, r, h0, tl, tn, tp)
    assert torch.isfinite(out).all()
    assert float((out - ref).norm() / ref.norm()) <= 1e-6
    assert float((hist - href).norm() / href.norm()) <= 1e-6
    eng.set_cfg(guidance=G, rescale=0.0)
    eng.x0_hist.copy_(h0)
    assert not torch.equal(eng.step(z, tn, tp, t_last=tl), out)      # the control is live


@pytest.mark.parametrize("target,keying", [("video", "sample"), ("video", "canvas"), ("audio", "sample"), ("audio", "canvas")])
def test_cond_only_step_equals_composed(dev, model, cfg_rows, target, keying):
    """eps_tokens is [B, Nt, D] after a cond-only step; video: bit for bit as test_gpu_guidance_interval.py's composed check."""
    z, zp, npr = video_case(dev, B=3) if target == "video" else audio_case(dev, B=3)
    hop = 2 if target == "video" else 20
    eng = _sde(model, target, tuple(z.shape), npr, sample_offset=1) if keying == "sample" else \
        _canvas(model, target, tuple(z.shape), npr, hop, sample_offset=1)
    eng.set_prompt(zp)
    tn, tp, tl = ts(TN, dev), ts(TP, dev), ts(TL, dev)
    h0 = _h0(z)
    outs = []
    for rows in ((1, 0) if target == "video" else (1,)):
        cfg_rows(rows)
        eng.x0_hist.copy_(h0)
        out = eng.step(z, tn, tp, t_last=tl, cond_only=True)
        ep = eng.eps_tokens()
        assert ep.dim() == 3 and ep.shape[0] == z.shape[0]
        ref, href = _composed(eng, z, _untok(eng, ep), h0, tl, tn, tp)
        if target == "video":
            assert torch.equal(out, ref) and torch.equal(eng.x0_hist, href)
        else:
            assert rel_err(out.cpu(), ref.cpu()) <= 1e-6 and rel_err(eng.x0_hist.cpu(), href.cpu()) <= 1e-6
        outs.append(out.clone())
    assert all(torch.equal(o, outs[0]) for o in outs)
    eng.x0_hist.copy_(h0)
    assert not torch.equal(eng.step(z, tn, tp, t_last=tl), outs[0])  # the CFG step differs


# ------------------------------------------------------------------------------------------------- first order against DDIM
@pytest.mark.parametrize("target", ["video", "audio"])
def test_first_order_eta1_step_matches_seeded_ddim(dev, model, target):
    """Same seed, same normals; the coefficient expressions differ (exponential against DDIM's square roots).  The bound is the ODE
    twin's 2e-6.  Measured on the MI355X: rel_err 1.150e-07 (video), 1.330e-07 (audio); the fp32 numpy mirrors of the two updates
    differ by 6e-8 at these timesteps."""
    z, zp, npr = video_case(dev, B=2) if target == "video" else audio_case(dev, B=2)
    sde = _sde(model, target, tuple(z.shape), npr, eta=1.0, sample_offset=3)
    ddim = _engine(model[1], target, tuple(z.shape), npr, eta=1.0, noise_seed=SEED, sample_offset=3)
    for e in (sde, ddim):
        e.set_prompt(zp)
    tn, tp = ts([999, 500], dev), ts([950, 450], dev)
    a = sde.step(z, tn, tp)                                   # t_last = None: first order
    b = ddim.step(z, tn, tp)
    err = rel_err(a.cpu(), b.cpu())
    print(f"first-order SDE step vs seeded DDIM eta = 1 ({target}): rel_err {err:.3e}")
    assert err <= 2e-6
    sched = R.sampling_schedule(1000, 1)                      # [999, -1]: both return x0_s
    assert torch.equal(sde.run(z, sched), ddim.run(z, sched))


# ------------------------------------------------------------------------------------------------- graph = eager
@pytest.mark.parametrize("n_steps", [5, 6])
@pytest.mark.parametrize("keying", ["sample", "canvas"])
def test_graph_equals_eager(dev, model, keying, n_steps):
    z, za, npr = video_case(dev, B=3, W=16)
    sched = R.sampling_schedule(1000, n_steps)
    if keying == "sample":
        eng = _sde(model, "video", tuple(z.shape), npr)
    else:
        eng = _canvas(model, "video", tuple(z.shape), npr, 2)
        eng.set_window_consensus(2)
    eng.set_prompt(za)
    zg = eng.run(z, sched, graph=True)
    ze = eng.run(z, sched, graph=False)
    assert torch.isfinite(zg).all() and torch.equal(zg, ze)
    assert torch.equal(eng.run(z, sched, graph=True), zg)     # a second run starts first order again, and draws the same noise
    if keying == "canvas":
        assert W.overlaps_agree(zg.cpu().numpy(), 2)


def test_graph_equals_eager_guidance_interval(dev, model):
    z, za, npr = video_case(dev, B=3, W=16)
    sched = R.sampling_schedule(1000, 6)
    iv = (int(sched[4]), int(sched[1]))                       # steps 1 .. 4 are CFG steps, 0 and 5 cond-only: both kinds of pair
    eng = _sde(model, "video", tuple(z.shape), npr, guidance_interval=iv)
    eng.set_prompt(za)
    zg = eng.run(z, sched, graph=True)
    assert torch.equal(zg, eng.run(z, sched, graph=False))
    eng.set_guidance_interval(None)
    assert not torch.equal(eng.run(z, sched, graph=False), zg)


# ------------------------------------------------------------------------------------------------- split invariance
def test_split_invariance(dev, model):
    z, za, npr = video_case(dev, B=4, W=16)
    sched = R.sampling_schedule(1000, 4)

    def run(mk, lo, hi, off):
        eng = mk(model, "video", (hi - lo,) + tuple(z.shape[1:]), npr, matmul="f32", sample_offset=off)
        eng.set_prompt(za[lo:hi].contiguous())
        return eng.run(z[lo:hi].contiguous(), sched)

    whole = run(_sde, 0, 4, 0)
    assert torch.equal(whole, torch.cat([run(_sde, 0, 2, 0), run(_sde, 2, 4, 2)]))
    assert not torch.equal(whole[2:], run(_sde, 2, 4, 0))    # the offset keys the noise
    canvas = partial(_canvas, hop=2)
    cw = run(canvas, 0, 4, 0)                                 # windows 0 .. 3
    assert torch.equal(cw[2:], run(canvas, 2, 4, 2))          # a second engine starting at window 2
    assert not torch.equal(cw, whole)


# ------------------------------------------------------------------------------------------------- consensus at eta > 0
def test_consensus_at_eta_above_zero(dev, model):
    z, za, npr = video_case(dev, B=3, W=16)
    zw = torch.from_numpy(W.windows_from_canvas(torch.randn(8, 8, 16, 16, generator=torch.Generator().manual_seed(1)).numpy(), 4, 2)).to(dev)
    sched = R.sampling_schedule(1000, 4)
    outs = {}
    for eta in (ETA, 0.0):
        eng = _canvas(model, "video", tuple(z.shape), npr, 2, eta=eta)
        eng.set_prompt(za)
        eng.set_window_consensus(2)
        out = eng.run(zw, sched)
        o = out.cpu()
        assert torch.isfinite(out).all()
        assert torch.equal(o[0][:, 2:], o[1][:, :2]) and torch.equal(o[1][:, 2:], o[2][:, :2])      # neighbours agree on overlaps
        outs[eta] = out
    assert not torch.equal(outs[ETA], outs[0.0])


# ------------------------------------------------------------------------------------------------- trajectory vs the oracle
@pytest.mark.parametrize("mode", ["f32", "bf16x3"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_trajectory_vs_oracle(dev, model, target, mode):
    """6 steps against the CPU oracle's eps driven by the fp64 reference on the numpy stream's normals; the bound of the ODE solver's
    test_trajectory_vs_oracle (the SDE adds one elementwise term)."""
    ws, _ = model
    n_steps, off = 6, 2
    sched = R.sampling_schedule(1000, n_steps)
    if target == "video":
        z, zp, npr = video_case(dev, B=2, W=16)
    else:
        z, zp, npr = audio_case(dev, B=2)
    eng = _sde(model, target, tuple(z.shape), npr, eta=0.5, matmul=mode, sample_offset=off)
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
        noise = NR.normals(SEED, off, tn.numpy(), x[0].numel()).reshape(tuple(x.shape))
        y, hist = S.step_f64(x.numpy(), eps.numpy(), hist, ABAR.numpy(), [t_last] * 2, tn.numpy(), tp.numpy(), 0.5, noise)
        x, t_last = torch.from_numpy(y).float(), int(sched[i])
    ref = x.double()
    err = float((out - ref).norm() / ref.norm())
    print(f"SDE trajectory vs oracle ({target}, {mode}): relative error {err:.3e}")
    assert err < 1e-3


# ------------------------------------------------------------------------------------------------- stream_generate
def test_stream_generate(dev, model):
    from multimodal_diffusion_amd import stream_infer as SI
    with matmul_f32(model[1]):            # one kernel family whatever the batch
        vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND,
                                   sampling={"solver": "dpmpp_2m", "ddim_eta": 0.5})
        kw = dict(components(model[1], vae, codec, dev), cfg=cfg, shard=False, noise_seed=3, **audio_prompt())      # 4 windows
        whole = SI.stream_generate(**kw)
        per_window = SI.stream_generate(max_windows_per_batch=1, **kw)
        assert np.array_equal(whole["video"], per_window["video"])
        det = SI.stream_generate(**dict(kw, cfg=dict(cfg, sampling=dict(cfg["sampling"], ddim_eta=0.0))))
        assert not np.array_equal(det["video"], whole["video"])
        with pytest.raises(ValueError, match="eta"):          # the SDE form draws seeded noise only
            SI.stream_generate(**dict(kw, noise_seed=None))
        kc = dict(kw, consensus="uniform", noise_keying="canvas", return_latents=True)
        hop, _ = SI.latent_hop(cfg, "video")
        cons = SI.stream_generate(**kc)
        assert np.isfinite(cons["latents"]).all() and W.overlaps_agree(cons["latents"], hop)
        assert np.array_equal(SI.stream_generate(max_windows_per_batch=2, **kc)["latents"], cons["latents"])
        detc = SI.stream_generate(**dict(kc, cfg=dict(cfg, sampling=dict(cfg["sampling"], ddim_eta=0.0))))
        assert not np.array_equal(detc["latents"], cons["latents"])


# ------------------------------------------------------------------------------------------------- misuse
def test_misuse(dev, model):
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn
    z, za, npr = video_case(dev, B=3, W=16)
    shape = tuple(z.shape)
    eng = _sde(model, "video", shape, npr)
    eng.set_prompt(za)
    tn, tp = ts([900] * 3, dev), ts([800] * 3, dev)
    with pytest.raises(ValueError):
        eng.step(z, tn, tp, noise=torch.randn_like(z))
    with pytest.raises(ValueError, match="noise_keying='canvas'"):
        eng.set_window_consensus(2)                           # per-sample keyed: the mean would shrink the noise
    canvas = _canvas(model, "video", shape, npr, 2)
    with pytest.raises(ValueError, match="canvas_hop"):
        canvas.set_window_consensus(3)
    eng.x0_hist.copy_(z)
    with pytest.raises(L.AvdError):
        eng.step(eng.x0_hist, tn, tp)
    with pytest.raises(L.AvdError):
        eng.step(z, tn, tp, out=eng.x0_hist)
    for bad in ([999, 500, 500, -1], [999, 200, 500, -1]):
        with pytest.raises(ValueError, match="decreasing"):
            eng.run(z, torch.tensor(bad))
    with pytest.raises(ValueError, match="eta"):
        _engine(model[1], "video", shape, npr, solver="dpmpp_2m", eta=0.5)
    x = torch.randn(2, 64, device=dev)
    t2 = ts([900, 900], dev)
    with pytest.raises(ValueError, match="noise"):
        Fn.dpmpp_2m_sde_step(x, torch.randn_like(x), torch.zeros_like(x), t2, t2, t2, ABAR, 0.5)
    n = torch.randn_like(x)
    with pytest.raises(ValueError, match="noise"):
        Fn.dpmpp_2m_sde_step(x, torch.randn_like(x), n, t2, t2, t2, ABAR, 0.5, n)                  # noise over x0_hist
