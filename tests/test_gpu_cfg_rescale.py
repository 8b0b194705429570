"""The CFG control on the MI355X (include/avdiff_hip.h, avd_cfg_control): functional.cfg_rescale against the numpy mirror, the fused
controlled step against the composed path (eps tokens -> U -> cfg_rescale -> the elementwise update) for every solver, kernel form
and with / without a latent guide, bit-identity of rows / gather forms, graph replay with values changed in place, split_streams,
batch splits, all-equal arrays against the scalar and phi = 0 against the plain engine, trajectories against the CPU oracle, the
phi = 1 property, sample_one_direction's sampling.guidance_rescale, and misuse."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

import _cfg_ref as CR
from _kit import ABAR, Recorder, case, components, dev, engine, model, pipeline, ts  # noqa: F401  (dev / model are fixtures)
from _tune import cfg_rows  # noqa: F401  (fixture)
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
GS = 3.0
GSEED = 77
_engine = partial(engine, guidance=GS)        # engine(mods, target, shape, n_prompt, **kw) at this file's guidance


def _untok(eng, tok):
    """U: tokens [B, N, D] -> the latent's natural layout (tube un-patch / overlap-add mean)"""
    from multimodal_diffusion_amd import functional as Fn
    shape = eng.latent_shape
    if eng.target == "video":
        return Fn.tube_unpatch(tok.contiguous(), *shape[1:], *eng.tube)
    return Fn.audio_untokens(tok.contiguous(), shape[1], eng.chunk[0], shape[2], eng.chunk[1])


# ------------------------------------------------------------------------------------------------- elementwise = numpy mirror
def test_functional_matches_mirror(dev):
    from multimodal_diffusion_amd import functional as Fn
    B, per = 5, 70_001                                          # not a multiple of 4 or of the 1024-element chunk
    g = torch.Generator().manual_seed(1)
    c = torch.randn(B, per, generator=g)
    y = c * torch.tensor([[3.0], [0.5], [1.0], [2.0], [7.0]]) + 0.3 * torch.randn(B, per, generator=g)
    y[2] = 0.125                                                # sigma_y == 0: s = 1
    s_ref = CR.scale(c.numpy(), y.numpy())
    assert s_ref[2] == 1.0
    for phi in (0.0, 0.3, 0.7, 1.0, [0.0, 0.3, 0.7, 1.0, 0.5]):
        out, s = Fn.cfg_rescale(c.to(dev), y.to(dev), phi, return_scale=True)
        s = s.cpu().numpy()
        assert CR.ulps(s, s_ref).max() <= 2, (s, s_ref)
        assert np.array_equal(out.cpu().numpy(), CR.rescale_f32(y.numpy(), phi, s))     # r(e) is elementwise: exact given s
        if phi == 0.0:
            assert torch.equal(out.cpu(), y)
    # in place (out aliasing e_cfg) at the C entry
    from multimodal_diffusion_amd import _lib as L
    yd, cd = y.to(dev), c.to(dev)
    ref = Fn.cfg_rescale(cd, yd, 0.7)
    ph = torch.full((B,), 0.7, device=dev)
    nb = L.lib().avd_cfg_stats_bytes(B, per)
    st = torch.empty(nb, dtype=torch.uint8, device=dev)
    L.check(L.lib().avd_cfg_rescale_f32(cd.data_ptr(), yd.data_ptr(), ph.data_ptr(), st.data_ptr(), nb, yd.data_ptr(), B, per,
                                        L.stream_ptr(dev)))
    assert torch.equal(yd, ref)


def test_phi_one_restores_conditional_std(dev):
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(5)
    c = torch.randn(3, 8, 12, 32, 32, generator=g)
    y = 4.0 * c + torch.randn(c.shape, generator=g)
    out = Fn.cfg_rescale(c.to(dev), y.to(dev), 1.0).cpu().double()
    for b in range(3):
        sc = float(c[b].double().std())
        assert abs(float(out[b].std()) - sc) <= 1e-5 * sc


# ------------------------------------------------------------------------------------------------- fused = composed
SOLVERS = [{}, dict(eta=0.7, noise_seed=5), dict(solver="dpmpp_2m")]
G2, PHI2 = [2.0, 5.0], [0.7, 0.3]


def _check_fused_equals_composed(dev, eng, cfg_rows, z, known, mask, kw, check_scale=False):
    """the body of test_fused_equals_composed for an engine built with guidance G2, rescale PHI2 and the solver keywords kw, its
    prompt set: B = 2; mask None = no guide.  check_scale: s_b of the composed path also against the numpy mirror, within the 2 ulp
    of test_functional_matches_mirror.  test_gpu_token_geometry runs it at the other geometries."""
    from multimodal_diffusion_amd import functional as Fn
    B, target = z.shape[0], eng.target
    dpm = kw.get("solver") == "dpmpp_2m"
    if mask is not None:
        eng.set_known(known, mask, guide_seed=GSEED)
    h0 = torch.randn(z.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    tn, tp = ts([981, 402], dev), ts([961, 382], dev)
    tl = ts([999, 700], dev) if dpm else None

    def fused():
        if dpm:
            eng.x0_hist.copy_(h0)
        return eng.step(z, tn, tp, t_last=tl).clone(), (eng.x0_hist.clone() if dpm else None)

    out, hist = fused()
    if target == "video":                                       # the gather form: bit-identical to the rows form
        cfg_rows(0)
        out0, hist0 = fused()
        cfg_rows(1)
        assert torch.equal(out0, out)
        if dpm:
            assert torch.equal(hist0, hist)
    # composed: eps tokens -> U -> cfg_rescale -> the elementwise update (-> the guide's blend)
    ep = eng.eps_tokens()
    ec, en = ep[:B], ep[B:]
    gt = torch.tensor(G2, device=dev).view(B, 1, 1)
    c, y = _untok(eng, ec), _untok(eng, en + gt * (ec - en))
    r, s = Fn.cfg_rescale(c, y, PHI2, return_scale=True)
    if check_scale:
        s_ref = CR.scale(c.cpu().numpy(), y.cpu().numpy())
        assert CR.ulps(s.cpu().numpy(), s_ref).max() <= 2, (s, s_ref)
    if dpm:
        h = h0.clone()
        ref = Fn.dpmpp_2m_step(z, r, h, tl, tn, tp, ABAR)
        assert float((hist - h).norm() / h.norm()) <= 1e-6
    elif kw:
        ref = Fn.ddim_step(z, tn, tp, r, ABAR, eta=0.7, noise=Fn.gaussian_noise(5, 0, tn, tuple(z.shape)))
    else:
        ref = Fn.ddim_step(z, tn, tp, r, ABAR)
    if mask is not None:
        ref = Fn.latent_guide(known, tp, ABAR, z=ref, mask=mask, seed=GSEED)
    assert torch.isfinite(out).all()
    assert float((out - ref).norm() / ref.norm()) <= 1e-6
    # and the control did something: the plain step at the scalar guidance differs
    eng.set_cfg(guidance=GS, rescale=0.0)
    if dpm:
        eng.x0_hist.copy_(h0)
    assert not torch.equal(eng.step(z, tn, tp, t_last=tl), out)


@pytest.mark.parametrize("guided", [False, True])
@pytest.mark.parametrize("kw", SOLVERS, ids=["ddim", "seeded", "dpmpp_2m"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_fused_equals_composed(dev, model, cfg_rows, target, kw, guided):
    z, zp, npr, known = case(dev, target)
    eng = _engine(model[1], target, tuple(z.shape), npr, guidance=G2, guidance_rescale=PHI2, **kw)
    eng.set_prompt(zp)
    mask = None
    if guided:
        mask = torch.rand(tuple(z.shape[1:]), generator=torch.Generator().manual_seed(3))
        mask[mask < 0.35] = 0.0
        mask = mask.to(dev)
    _check_fused_equals_composed(dev, eng, cfg_rows, z, known, mask, kw)


# ------------------------------------------------------------------------------------------------- bit-identities
def test_graph_replay_follows_set_cfg(dev, model):
    from multimodal_diffusion_amd import _lib as L
    z, zp, npr, _ = case(dev, "video")
    B = z.shape[0]
    sched = R.sampling_schedule(1000, 5)
    A_, B_ = dict(guidance=[2.0, 5.0], rescale=[0.7, 0.0]), dict(guidance=[4.0, 1.5], rescale=[0.2, 1.0])
    eng = _engine(model[1], "video", tuple(z.shape), npr, guidance=A_["guidance"], guidance_rescale=A_["rescale"])
    eng.set_prompt(zp)
    # eager: values A for steps 0..2, B for steps 3..4
    x = z.clone()
    for i in range(5):
        eng.set_cfg(**(A_ if i < 3 else B_))
        x = eng.step(x, sched[i].repeat(B), sched[i + 1].repeat(B))
    eager = x
    # graph: one capture, values changed in place between replays
    eng.set_cfg(**A_)
    gen = eng._generation
    eng.begin(sched)
    za, zb = z.clone(), torch.empty_like(z)
    eng.advance(za, zb)
    za, zb = zb, za
    pair = eng.capture_pair(za, zb)
    pair.replay()                                               # steps 1, 2
    eng.set_cfg(**B_)
    pair.replay()                                               # steps 3, 4
    assert eng._generation == gen
    assert torch.equal(za, eager)
    # run(): graph against eager
    assert torch.equal(eng.run(z, sched, graph=True), eng.run(z, sched, graph=False))
    # back to the plain step: a new generation, the pair is refused
    eng.set_cfg(guidance=GS, rescale=0.0)
    assert eng._generation == gen + 1 and eng._ctl is None
    with pytest.raises(L.AvdError, match="stale"):
        pair.replay()


@pytest.mark.parametrize("target", ["video", "audio"])
def test_split_streams_and_defaults(dev, model, target):
    z, zp, npr, _ = case(dev, target)
    tn, tp = ts([981, 402], dev), ts([961, 382], dev)

    def step(**kw):
        eng = _engine(model[1], target, tuple(z.shape), npr, **kw)
        eng.set_prompt(zp)
        return eng, eng.step(z, tn, tp)

    _, on = step(guidance=G2, guidance_rescale=PHI2, matmul="f16x2", split_streams=True)
    _, off = step(guidance=G2, guidance_rescale=PHI2, matmul="f16x2", split_streams=False)
    assert torch.equal(on, off)
    e0, plain = step()
    assert e0._ctl is None and e0._cfg_stats is None
    e1, zero = step(guidance_rescale=0.0)                       # phi = 0 with a scalar guidance: the plain step itself
    assert e1._ctl is None and torch.equal(zero, plain)
    e2, arr = step(guidance=[GS, GS])                           # an all-equal array: the controlled kernel, the scalar's bits
    assert e2._ctl is not None and not e2._ctl.rescale and torch.equal(arr, plain)
    e3, arr0 = step(guidance=[GS, GS], guidance_rescale=[0.0, 0.0])    # phi = 0 everywhere: no statistics pass
    assert not e3._ctl.rescale and torch.equal(arr0, plain)
    e4, half = step(guidance_rescale=[0.0, 0.5])                # the statistics pass runs; phi_0 = 0 selects y
    assert e4._ctl.rescale and torch.equal(half[0], plain[0]) and not torch.equal(half[1], plain[1])
    _, per = step(guidance=[GS, 6.0])
    assert torch.equal(per[0], plain[0]) and not torch.equal(per[1], plain[1])


def test_batch_split(dev, model):
    z, zp, npr, _ = case(dev, "video", B=4)
    g4, p4 = [2.0, 5.0, 3.0, 1.5], [0.7, 0.0, 1.0, 0.3]
    sched = R.sampling_schedule(1000, 4)

    def run(sl, **kw):
        eng = _engine(model[1], "video", (sl.stop - sl.start,) + tuple(z.shape[1:]), npr, matmul="f32", **kw)
        eng.set_prompt(zp[sl].contiguous())
        return eng.run(z[sl].contiguous(), sched)

    halves = (slice(0, 2), slice(2, 4))
    whole = run(slice(0, 4), guidance=g4, guidance_rescale=p4)
    parts = torch.cat([run(s, guidance=g4[s], guidance_rescale=p4[s]) for s in halves])
    plain4 = run(slice(0, 4))
    plain2 = torch.cat([run(s) for s in halves])
    if torch.equal(plain4, plain2):
        # the model itself is batch-invariant here: then the control must be too (s_b depends on the sample alone)
        assert torch.equal(whole, parts)
    else:
        assert float((whole - parts).norm() / whole.norm()) < 1e-5


# ------------------------------------------------------------------------------------------------- trajectory vs the oracle
def _oracle_step(ws, target, x, zp, tn, tp, g, phi):
    B = x.shape[0]
    if target == "video":
        tok_t, tok_p = R.tube_patch(x, 2, 4, 4), R.audio_tokens(zp, 4, 4)
        at, ap = ws["adapt_v"], ws["adapt_a"]
    else:
        tok_t, tok_p = R.audio_tokens(x, 4, 4), R.tube_patch(zp, 2, 4, 4)
        at, ap = ws["adapt_a"], ws["adapt_v"]
    Xt = R.embed_with_time(tok_t, at["proj.weight"], at["proj.bias"], tn, 256)
    Xp = R.embed_with_time(tok_p, ap["proj.weight"], ap["proj.bias"], torch.zeros_like(tn), 256)
    ec, en = R.eps_pair(Xt, Xp, target == "video", ws["core"], ws["head"], target, 2, 8)
    y_tok = torch.from_numpy(CR.combine_f32(ec.numpy(), en.numpy(), g))
    if target == "video":
        U = lambda t: R.tube_unpatch(t, *x.shape[1:], 2, 4, 4)          # noqa: E731
    else:
        U = lambda t: R.audio_untokens(t, x.shape[1], 4, x.shape[2], 4)  # noqa: E731
    r = CR.cfg_rescale(U(ec).numpy(), U(y_tok).numpy(), phi)
    return R.ddim_update(x, tn, tp, torch.from_numpy(r), ABAR)


@pytest.mark.parametrize("target", ["video", "audio"])
def test_trajectory_vs_oracle(dev, model, target):
    ws, _ = model
    n_steps = 8
    g, phi = [2.0, 5.0], [0.7, 0.0]
    sched = R.sampling_schedule(1000, n_steps)
    gen = torch.Generator().manual_seed(2)
    if target == "video":
        z, zp, npr = torch.randn(2, 8, 4, 16, 16, generator=gen), torch.randn(2, 8, 40, generator=gen), 10
    else:
        z, zp, npr = torch.randn(2, 8, 40, generator=gen), torch.randn(2, 8, 4, 8, 8, generator=gen), 8
    eng = _engine(model[1], target, tuple(z.shape), npr, guidance=g, guidance_rescale=phi, matmul="f32")
    eng.set_prompt(zp.to(dev))
    out = eng.run(z.to(dev), sched).cpu().double()
    x = z.clone()
    for i in range(n_steps):
        x = _oracle_step(ws, target, x, zp, sched[i].repeat(2), sched[i + 1].repeat(2), g, phi)
    ref = x.double()
    assert float((out - ref).norm() / ref.norm()) < 1e-3


# ------------------------------------------------------------------------------------------------- sample_one_direction
def test_sample_one_direction_guidance_rescale(dev, model):
    import multimodal_diffusion_amd as A
    vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=1.0, sampler_steps=5,
                               sampling={"guidance_scale": {"video": 4.0, "audio": 4.0}})
    vae = Recorder(vae)
    wav = (0.1 * torch.randn(16000, generator=torch.Generator().manual_seed(9))).numpy()
    kw = dict(components(model[1], vae, codec, dev), prompt_modality="audio", prompt_video=None, prompt_audio=wav)
    noise = torch.randn(1, 8, 4, 4, 4, generator=torch.Generator().manual_seed(4))
    a = A.sample_one_direction(cfg=cfg, init_noise=noise, **kw)
    za = vae.last
    cfg0 = dict(cfg, sampling=dict(cfg["sampling"], guidance_rescale={"video": 0.0}))
    b = A.sample_one_direction(cfg=cfg0, init_noise=noise, **kw)
    assert np.array_equal(a["video"], b["video"]) and torch.equal(vae.last, za)
    cfg7 = dict(cfg, sampling=dict(cfg["sampling"], guidance_rescale={"video": 0.7}))
    c = A.sample_one_direction(cfg=cfg7, init_noise=noise, **kw)
    assert c["video"].shape == a["video"].shape
    assert torch.isfinite(vae.last).all() and not torch.equal(vae.last, za)


# ------------------------------------------------------------------------------------------------- misuse
def test_misuse(dev, model):
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn
    z, zp, npr, _ = case(dev, "video")
    for bad in (dict(guidance_rescale=1.5), dict(guidance_rescale=float("nan")), dict(guidance_rescale=[0.2, -0.1]),
                dict(guidance=[1.0, 2.0, 3.0]), dict(guidance=[1.0, float("inf")])):
        with pytest.raises(ValueError):
            _engine(model[1], "video", tuple(z.shape), npr, **bad)
    eng = _engine(model[1], "video", tuple(z.shape), npr, solver="dpmpp_2m", guidance_rescale=0.5)
    eng.set_prompt(zp)
    gen = eng._generation
    with pytest.raises(ValueError, match="guidance_rescale"):
        eng.set_cfg(guidance=[2.0, 3.0], rescale=2.0)
    assert eng._generation == gen and eng._g_per_sample is False          # nothing changed
    with pytest.raises(ValueError, match="phi"):
        Fn.cfg_rescale(z, z, 1.01)
    with pytest.raises(ValueError):
        Fn.cfg_rescale(z[:, :1, :1, :1, :1].contiguous(), z[:, :1, :1, :1, :1].contiguous(), 0.5)    # one element per sample
    # unseeded eta > 0 with a control
    ddim = _engine(model[1], "video", tuple(z.shape), npr, eta=0.5, guidance=[2.0, 3.0])
    ddim.set_prompt(zp)
    tn, tp = ts([900, 900], dev), ts([800, 800], dev)
    with pytest.raises(ValueError, match="noise_seed"):
        ddim.step(z, tn, tp)
    # the stats scratch overlapping z_out / x0_hist, or too small, at the C entry: refused before any launch
    out = torch.full_like(z, 7.0)
    ctl = eng._ctl

    def call(c, o=out):
        return L.lib().avd_denoise_step_cfg_f32(C.byref(eng.desc), C.byref(c), None, None, eng._no_hist.data_ptr(), eng.x0_hist.data_ptr(),
                                                z.data_ptr(), eng.Xp.data_ptr(), tn.data_ptr(), tp.data_ptr(), o.data_ptr(),
                                                eng.workspace.data_ptr(), eng.workspace.numel(), L.stream_ptr(dev))
    assert call(L.CfgControl(ctl.guidance, ctl.rescale, out.data_ptr(), ctl.stats_bytes)) == L.EINVAL
    assert call(L.CfgControl(ctl.guidance, ctl.rescale, eng.x0_hist.data_ptr(), ctl.stats_bytes)) == L.EINVAL
    assert call(L.CfgControl(ctl.guidance, ctl.rescale, ctl.stats, ctl.stats_bytes - 16)) == L.EINVAL
    assert call(L.CfgControl(ctl.guidance, ctl.rescale, None, 0)) == L.EINVAL
    assert call(L.CfgControl(ctl.guidance, ctl.rescale, ctl.stats + 8, ctl.stats_bytes)) == L.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call(ctl) == 0                                                 # the engine's own control goes through
