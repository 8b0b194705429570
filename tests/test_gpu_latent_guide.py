"""The latent guide on the MI355X (include/avdiff_hip.h, avd_latent_guide): the elementwise blend against the numpy mirror, the fused
guided step against the unguided step followed by the elementwise blend (bit for bit, every solver and kernel form), the mask's
select cases, graph replay against eager launches, guided trajectories against the CPU oracle, batch / sample_offset invariance,
sample_one_direction's init / strength / mask arguments, and misuse."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

import _guide_ref as G
from _kit import ABAR, Recorder, case, components, dev, engine, model, pipeline, soft_mask, ts  # noqa: F401  (dev / model are fixtures)
from _tune import cfg_rows  # noqa: F401  (fixture)
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
GS = 3.0
GSEED = 77
_engine = partial(engine, guidance=GS)        # engine(mods, target, shape, n_prompt, **kw) at this file's guidance


# ------------------------------------------------------------------------------------------------- elementwise = numpy mirror
def test_elementwise_matches_reference(dev):
    from multimodal_diffusion_amd import functional as Fn
    B, per = 6, 65_539                                        # not a multiple of 4
    g = torch.Generator().manual_seed(1)
    known, z = torch.randn(B, per, generator=g), torch.randn(B, per, generator=g)
    m = soft_mask((per,))
    tau = [999, 500, 17, 0, -1, 1500]
    got = Fn.latent_guide(known.to(dev), ts(tau, dev), ABAR, z=z.to(dev), mask=m.to(dev), seed=GSEED, sample_offset=9).cpu()
    q = G.q_f64(known.numpy(), tau, ABAR.numpy(), GSEED, 9)
    ref = G.blend_f64(m.numpy(), q, z.numpy())
    assert np.abs(got.double().numpy() - ref).max() < 2e-5
    keep, free = (m == 1).expand(B, per), (m == 0).expand(B, per)
    assert torch.equal(got[free], z[free])
    assert torch.equal(got[4][keep[4]], known[4][keep[4]])    # tau < 0: known bit for bit
    pure = Fn.latent_guide(known.to(dev), ts(tau, dev), ABAR, seed=GSEED, sample_offset=9).cpu()
    assert np.abs(pure.double().numpy() - q).max() < 2e-5
    assert torch.equal(pure[4], known[4])
    per_sample = soft_mask((B, per), seed=4)
    got2 = Fn.latent_guide(known.to(dev), ts(tau, dev), ABAR, z=z.to(dev), mask=per_sample.to(dev), seed=GSEED, sample_offset=9).cpu()
    assert np.abs(got2.double().numpy() - G.blend_f64(per_sample.numpy(), q, z.numpy())).max() < 2e-5


# ------------------------------------------------------------------------------------------------- fused = composed
VARIANTS = [("video", 1, {}), ("video", 0, {}), ("audio", 1, {}),
            ("video", 1, dict(eta=0.7, noise_seed=5)), ("video", 0, dict(eta=0.7, noise_seed=5)), ("audio", 1, dict(eta=0.7, noise_seed=5)),
            ("video", 1, dict(solver="dpmpp_2m")), ("video", 0, dict(solver="dpmpp_2m")), ("audio", 1, dict(solver="dpmpp_2m")),
            ("video", 1, dict(matmul="f16x2", split_streams=True))]


@pytest.mark.parametrize("target,rows,kw", VARIANTS)
def test_fused_equals_composed(dev, model, cfg_rows, target, rows, kw):
    from multimodal_diffusion_amd import functional as Fn
    cfg_rows(rows)
    z, zp, npr, known = case(dev, target)
    eng = _engine(model[1], target, tuple(z.shape), npr, **kw)
    eng.set_prompt(zp)
    dpm = kw.get("solver") == "dpmpp_2m"
    h0 = torch.randn(z.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    tn, tp = ts([981, 402], dev), ts([961, 382], dev)
    tls = [None, ts([999, 700], dev)] if dpm else [None]       # DPM: first and second order
    soft = soft_mask(tuple(z.shape[1:])).to(dev)
    for tl in tls:
        def plain():
            eng.clear_known()
            if dpm:
                eng.x0_hist.copy_(h0)
            return eng.step(z, tn, tp, t_last=tl).clone(), (eng.x0_hist.clone() if dpm else None)

        def guided(mask):
            eng.set_known(known, mask, guide_seed=GSEED)
            if dpm:
                eng.x0_hist.copy_(h0)
            return eng.step(z, tn, tp, t_last=tl).clone(), (eng.x0_hist.clone() if dpm else None)

        base, hb = plain()
        out, hg = guided(soft)
        ref = Fn.latent_guide(known, tp, ABAR, z=base, mask=soft, seed=GSEED)
        assert torch.isfinite(out).all()
        assert torch.equal(out, ref)
        if dpm:
            assert torch.equal(hg, hb)                        # x0_hist holds the model's x0, not a blended value
        zero, _ = guided(torch.zeros_like(soft))
        assert torch.equal(zero, base)                        # an all-zero mask is the unguided step
        one, _ = guided(torch.ones_like(soft))
        assert torch.equal(one, Fn.latent_guide(known, tp, ABAR, seed=GSEED))
        nomask, _ = guided(None)
        assert torch.equal(nomask, one)


def test_full_run_keeps_known_frames(dev, model):
    import multimodal_diffusion_amd as A
    for target, kw in (("video", {}), ("video", dict(solver="dpmpp_2m")), ("audio", dict(eta=0.5, noise_seed=3))):
        z, zp, npr, known = case(dev, target)
        eng = _engine(model[1], target, tuple(z.shape), npr, **kw)
        eng.set_prompt(zp)
        m = A.frame_mask(tuple(z.shape[1:]), 0, 2)
        eng.set_known(known, m, guide_seed=GSEED)
        sched = R.sampling_schedule(1000, 5)
        z0, sk = eng.start_latent(z, sched, 1.0)
        assert torch.equal(sk, sched.to(torch.long))
        out = eng.run(z0, sk)
        keep = m.to(dev).bool().expand(z.shape)
        assert torch.equal(out[keep], known[keep])
        assert not torch.equal(out[~keep], known[~keep])


# ------------------------------------------------------------------------------------------------- graph = eager
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("n_steps", [5, 6])
def test_graph_equals_eager(dev, model, solver, n_steps):
    z, zp, npr, known = case(dev, "video")
    sched = R.sampling_schedule(1000, n_steps)
    eng = _engine(model[1], "video", tuple(z.shape), npr, solver=solver)
    eng.set_prompt(zp)
    eng.set_known(known, soft_mask(tuple(z.shape[1:])), guide_seed=GSEED)
    zg = eng.run(z, sched, graph=True)
    ze = eng.run(z, sched, graph=False)
    assert torch.equal(zg, ze)
    # new values behind the same buffers: no reallocation, the graph path follows them
    gen = eng._generation
    eng.set_known(known.flip(0), soft_mask(tuple(z.shape[1:]), seed=5), guide_seed=GSEED)
    assert eng._generation == gen
    assert torch.equal(eng.run(z, sched, graph=True), eng.run(z, sched, graph=False))
    eng.clear_known()
    assert eng._generation == gen + 1
    assert not torch.equal(eng.run(z, sched, graph=True), zg)


# ------------------------------------------------------------------------------------------------- trajectory vs the oracle
@pytest.mark.parametrize("target", ["video", "audio"])
def test_trajectory_vs_oracle(dev, model, target):
    ws, _ = model
    n_steps = 8
    sched = R.sampling_schedule(1000, n_steps)
    g = torch.Generator().manual_seed(2)
    if target == "video":
        z, zp, npr = torch.randn(2, 8, 4, 16, 16, generator=g), torch.randn(2, 8, 40, generator=g), 10
    else:
        z, zp, npr = torch.randn(2, 8, 40, generator=g), torch.randn(2, 8, 4, 8, 8, generator=g), 8
    known = torch.randn(z.shape, generator=g)
    m = soft_mask(tuple(z.shape[1:]), seed=6)
    eng = _engine(model[1], target, tuple(z.shape), npr, matmul="f32")
    eng.set_prompt(zp.to(dev))
    eng.set_known(known.to(dev), m, guide_seed=GSEED)
    out = eng.run(z.to(dev), sched).cpu().double()
    kw = dict(adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"], head=ws["head"], n_layers=2, n_heads=8, guidance=GS, eta=0.0)
    x = z.clone()
    for i in range(n_steps):
        tn, tp = sched[i].repeat(2), sched[i + 1].repeat(2)
        step = R.denoise_step_a2v if target == "video" else R.denoise_step_v2a
        y = step(x, zp, tn, tp, ABAR, **kw)
        y = G.blend_f64(m.numpy(), G.q_f64(known.numpy(), tp.numpy(), ABAR.numpy(), GSEED), y.double().numpy())
        x = torch.from_numpy(y).float()
    ref = x.double()
    assert float((out - ref).norm() / ref.norm()) < 1e-3


# ------------------------------------------------------------------------------------------------- batch / offset invariance
def test_batch_offset_invariance(dev, model):
    from multimodal_diffusion_amd import functional as Fn
    z, zp, npr, known = case(dev, "video", B=4)
    m = soft_mask(tuple(z.shape), seed=8).to(dev)             # one mask per sample
    sched = R.sampling_schedule(1000, 4)
    tau = ts([961, 382, 17, -1], dev)
    # the guide itself: a batch of 4 is two batches of 2 at sample_offset 0 and 2, bit for bit
    whole = Fn.latent_guide(known, tau, ABAR, z=z, mask=m, seed=GSEED)
    halves = torch.cat([Fn.latent_guide(known[s], tau[s], ABAR, z=z[s], mask=m[s], seed=GSEED, sample_offset=o)
                        for s, o in ((slice(0, 2), 0), (slice(2, 4), 2))])
    assert torch.equal(whole, halves)

    def run(sl, off):
        eng = _engine(model[1], "video", (sl.stop - sl.start,) + tuple(z.shape[1:]), npr, matmul="f32", noise_seed=1, sample_offset=off)
        eng.set_prompt(zp[sl].contiguous())
        eng.set_known(known[sl].contiguous(), m[sl].contiguous(), guide_seed=GSEED)
        z0, sk = eng.start_latent(z[sl].contiguous(), sched, 0.75)
        return z0, eng.run(z0, sk)

    (s4, o4), parts = run(slice(0, 4), 0), [run(slice(0, 2), 0), run(slice(2, 4), 2)]
    assert torch.equal(s4, torch.cat([p[0] for p in parts]))   # the SDEdit start: the guide's stream alone
    o2 = torch.cat([p[1] for p in parts])
    # the model's GEMMs may round differently at another batch size: the trajectories agree to fp32 level, the kept region exactly
    assert float((o4 - o2).norm() / o4.norm()) < 1e-5
    keep = m == 1
    assert torch.equal(o4[keep], known[keep]) and torch.equal(o2[keep], known[keep])


# ------------------------------------------------------------------------------------------------- sample_one_direction
@pytest.fixture(scope="module")
def a2v_setup(dev, model):
    vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=1.0, sampler_steps=5)
    wav = (0.1 * torch.randn(16000, generator=torch.Generator().manual_seed(9))).numpy()
    clip = np.random.default_rng(3).integers(0, 256, size=(16, 32, 32, 3), dtype=np.uint8)
    kw = dict(components(model[1], Recorder(vae), codec, dev), cfg=cfg, prompt_modality="audio", prompt_video=None, prompt_audio=wav)
    return kw, clip, vae


def test_sample_one_direction_init_strength_mask(dev, a2v_setup):
    import multimodal_diffusion_amd as A
    kw, clip, vae = a2v_setup
    with torch.no_grad():
        known = vae.encode((torch.from_numpy(clip).to(dev).float() / 255.0).permute(3, 0, 1, 2).unsqueeze(0).contiguous())
    lat = tuple(known.shape)
    noise = torch.randn(lat, generator=torch.Generator().manual_seed(4))
    m = A.frame_mask(lat[1:], 0, 2)
    out = A.sample_one_direction(init_noise=noise, init_video=clip, strength=0.6, mask=m, **kw)
    assert out["video"].shape == clip.shape and out["video"].dtype == np.uint8
    z_final = kw["vid_vae"].last
    keep = m.to(dev).bool().unsqueeze(0).expand(lat)
    assert torch.equal(z_final[keep], known[keep])
    # the defaults change nothing
    a = A.sample_one_direction(init_noise=noise, **kw)
    b = A.sample_one_direction(init_noise=noise, strength=1.0, mask=None, **kw)
    assert np.array_equal(a["video"], b["video"])
    # strength 0: the decode of the encoded clip
    s0 = A.sample_one_direction(init_noise=noise, init_video=clip, strength=0.0, **kw)
    assert torch.equal(kw["vid_vae"].last, known)
    with torch.no_grad():
        ref = (vae.decode(known).clamp(0, 1)[0].permute(1, 2, 3, 0).cpu().numpy() * 255.0).astype(np.uint8)
    assert np.array_equal(s0["video"], ref)
    # SDEdit without a mask: a variation of the clip, not the clip and not the unguided sample
    sd = A.sample_one_direction(init_noise=noise, init_video=clip, strength=0.6, **kw)
    assert not np.array_equal(sd["video"], a["video"]) and not np.array_equal(sd["video"], s0["video"])


# ------------------------------------------------------------------------------------------------- misuse
def test_misuse(dev, model, a2v_setup):
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import _lib as L
    z, zp, npr, known = case(dev, "video")
    eng = _engine(model[1], "video", tuple(z.shape), npr, solver="dpmpp_2m")
    eng.set_prompt(zp)
    with pytest.raises(ValueError, match="mask"):
        eng.set_known(known, torch.ones(3, 3))
    with pytest.raises(ValueError, match="mask"):
        eng.set_known(known, torch.full(tuple(z.shape[1:]), 1.5))
    with pytest.raises(ValueError, match="shape"):
        eng.set_known(known[:1])
    eng.set_known(known, None, guide_seed=GSEED)
    tn, tp = ts([900, 900], dev), ts([800, 800], dev)
    with pytest.raises(ValueError, match="overlap"):
        eng.step(z, tn, tp, out=eng._known)                   # known aliases z_out
    # known aliasing x0_hist, at the C entry
    g = L.LatentGuide(eng.x0_hist.data_ptr(), None, 0, L.NoiseKey(1, 0))
    out = torch.empty_like(z)
    rc = L.lib().avd_denoise_step_guided_f32(C.byref(eng.desc), C.byref(g), None, eng._no_hist.data_ptr(), eng.x0_hist.data_ptr(),
                                             z.data_ptr(), eng.Xp.data_ptr(), tn.data_ptr(), tp.data_ptr(), out.data_ptr(),
                                             eng.workspace.data_ptr(), eng.workspace.numel(), L.stream_ptr(dev))
    assert rc == L.EINVAL
    # unseeded eta > 0 with a guide
    ddim = _engine(model[1], "video", tuple(z.shape), npr, eta=0.5)
    ddim.set_prompt(zp)
    ddim.set_known(known, None)
    with pytest.raises(ValueError, match="noise_seed"):
        ddim.step(z, tn, tp)
    ddim.clear_known()
    with pytest.raises(ValueError, match="set_known"):
        ddim.start_latent(z, R.sampling_schedule(1000, 4), 0.5)
    # a wrong-modality or wrong-shape init
    kw, clip, _ = a2v_setup
    with pytest.raises(ValueError):
        A.sample_one_direction(init_audio=np.zeros(16000, dtype=np.float32), **kw)
    with pytest.raises(ValueError, match="latent"):
        A.sample_one_direction(init_video=clip[:8], **kw)
    with pytest.raises(ValueError, match="mask"):
        A.sample_one_direction(init_video=clip, mask=np.ones((8, 1, 4, 4), dtype=np.float32), **kw)
