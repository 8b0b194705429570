"""The guidance interval on the MI355X (include/avdiff_hip.h, "guidance interval"): the single-branch fused kernels against the composed
functional ops (bit for bit, every solver state, rows / gather / audio forms), the single-branch front end against the cond half of the
two-branch one, the cond-only step against the oracle's conditional prediction, trajectories under an interval against the oracle
stepped at guidance g inside and 1.0 outside, graph replay against eager launches, invariances, the entry points and misuse."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

import _interval_ref as IR
from _kit import (ABAR, Recorder, case, components, dev, engine, full, model, pipeline, soft_mask,  # noqa: F401  (dev / model / full are fixtures)
                  ts)
from _tune import cfg_rows, tune, tuned  # noqa: F401  (cfg_rows is a fixture)
from conftest import rel_err
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
TOL = 1e-4                      # the project's one-step tolerance (test_gpu_parity.TOL)
GS = 3.0
GSEED, NSEED = 77, 5
_engine = partial(engine, guidance=GS)        # engine(mods, target, shape, n_prompt, **kw) at this file's guidance


# ------------------------------------------------------------------------------------------------- 1. kernels = composed ops
STATES = ["plain", "noise", "seeded", "dpm1", "dpm2"]


def _fused(dev, target, eps, z, tn, tp, state, guide, h, geom=None):
    """avd_eps_unpatch_ddim_f32 / avd_eps_untoken_ddim_audio_f32 -> (z_out, x0_hist); geom: the tube (t, h, w) resp. the chunk
    (len, stride), None = 2 x 4 x 4 resp. 4 / 4 (test_gpu_token_geometry passes the others)"""
    from multimodal_diffusion_amd import _lib as L, functional as Fn
    B = z.shape[0]
    eta = 0.7 if state in ("noise", "seeded") else 0.0
    noise = Fn.gaussian_noise(NSEED, 4, tn, tuple(z.shape)) if state == "noise" else None
    key = Fn.noise_key(NSEED, 4) if state == "seeded" else None
    tl = {"dpm1": ts([-1] * B, dev), "dpm2": ts([999, 700, 850][:B], dev)}.get(state)
    hist = h.clone() if tl is not None else None
    out = torch.empty_like(z)
    ab = ABAR.to(dev)
    head = (eps.data_ptr(), z.data_ptr(), tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), ab.numel(), eta, L.ptr(noise), out.data_ptr(), B)
    tail = (None if key is None else C.byref(key), L.ptr(tl), L.ptr(hist), None if guide is None else C.byref(guide), L.stream_ptr(dev))
    if target == "video":
        L.check(L.lib().avd_eps_unpatch_ddim_f32(*head, *z.shape[1:], *(geom or (2, 4, 4)), *tail))
    else:
        L.check(L.lib().avd_eps_untoken_ddim_audio_f32(*head, z.shape[1], z.shape[2], *(geom or (4, 4)), *tail))
    return out, hist


def _composed(dev, target, eps, z, tn, tp, state, known, mask, h, geom=None):
    """tube_unpatch / audio_untokens, then ddim_step / dpmpp_2m_step, then latent_guide: the existing functional ops; geom as _fused"""
    from multimodal_diffusion_amd import functional as Fn
    B = z.shape[0]
    if target == "video":
        lat = Fn.tube_unpatch(eps, *z.shape[1:], *(geom or (2, 4, 4)))
    else:
        ln, st = geom or (4, 4)
        lat = Fn.audio_untokens(eps, z.shape[1], ln, z.shape[2], st)
    hist = None
    if state in ("dpm1", "dpm2"):
        hist = h.clone()
        tl = ts([-1] * B, dev) if state == "dpm1" else ts([999, 700, 850][:B], dev)
        out = Fn.dpmpp_2m_step(z, lat, hist, tl, tn, tp, ABAR)
    elif state == "plain":
        out = Fn.ddim_step(z, tn, tp, lat, ABAR)
    else:       # the seeded kernel draws what gaussian_noise hands out
        out = Fn.ddim_step(z, tn, tp, lat, ABAR, 0.7, Fn.gaussian_noise(NSEED, 4, tn, tuple(z.shape)))
    if known is not None:
        out = Fn.latent_guide(known, tp, ABAR, z=out, mask=mask, seed=GSEED, sample_offset=4)
    return out, hist


# GT = 8 (W = 32), GT = 4 (W = 16), the gather fallback (W = 8: two tokens per row), audio
GEOMS = [("video", (8, 4, 16, 32)), ("video", (8, 4, 16, 16)), ("video", (8, 4, 16, 8)), ("audio", (8, 40))]


# every solver state with and without a latent guide; a guide takes seeded noise only (unseeded noise with it is refused: test_misuse)
KCASES = [(t, lat, st, gd) for t, lat in GEOMS for st in STATES for gd in (False, True) if not (gd and st == "noise")]


def _check_kernels_equal_composed(dev, cfg_rows, target, lat, state, guided, seed, n_tok, geom=None):
    """the body of test_kernels_equal_composed_ops for one latent (lat, without the batch), its token count and its geometry (as
    _fused); test_gpu_token_geometry runs it at the other geometries"""
    from multimodal_diffusion_amd import functional as Fn
    B = 3
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(B, *lat, generator=g).to(dev)
    eps = torch.randn(B, *n_tok, generator=g).to(dev)
    known, h = torch.randn(z.shape, generator=g).to(dev), torch.randn(z.shape, generator=g).to(dev)
    mask = soft_mask(tuple(z.shape[1:])).to(dev)
    tn, tp = ts([981, 402, 40], dev), ts([961, 382, -1], dev)
    guide = Fn.latent_guide_desc(known, mask, GSEED, 4) if guided else None
    ref, href = _composed(dev, target, eps, z, tn, tp, state, known if guided else None, mask, h, geom)
    outs = []
    for rows in ((1, 0) if target == "video" else (1,)):
        cfg_rows(rows)
        out, hist = _fused(dev, target, eps, z, tn, tp, state, guide, h, geom)
        assert torch.isfinite(out).all()
        assert torch.equal(out, ref), (rows, float((out - ref).abs().max()))
        if hist is not None:
            assert torch.equal(hist, href)                     # x0_hist: the model's x0, also under a guide
        outs.append(out)
    if len(outs) == 2:
        assert torch.equal(outs[0], outs[1])                   # rows form == gather form


@pytest.mark.parametrize("target,lat,state,guided", KCASES)
def test_kernels_equal_composed_ops(dev, cfg_rows, target, lat, state, guided):
    n_tok = ((lat[1] // 2) * (lat[2] // 4) * (lat[3] // 4), lat[0] * 32) if target == "video" else ((lat[1] - 4) // 4 + 1, lat[0] * 4)
    _check_kernels_equal_composed(dev, cfg_rows, target, lat, state, guided, len(lat) * 100 + lat[-1], n_tok)


# ------------------------------------------------------------------------------------------------- 2. front end
@pytest.mark.parametrize("temb_mode", ["concat", "add"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_front_end_equals_cond_half(dev, model, target, temb_mode):
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import _lib as L
    _, (core, head, av, aa) = model
    z, zp, npr, _ = case(dev, target, B=3)
    adapters = dict(adapt_v=av, adapt_a=aa)
    if temb_mode == "add":      # the trainer's embedding needs d-wide adapters
        torch.manual_seed(1)
        adapters = dict(adapt_v=A.LinearAdapter(256, 512).to(dev), adapt_a=A.LinearAdapter(32, 512).to(dev))
    eng = A.DenoiseEngine(core=core, head=head, tstep_dim=256, target=target, latent_shape=tuple(z.shape), prompt_tokens=npr,
                          alpha_bar=ABAR, guidance=GS, temb_mode=temb_mode, **adapters)
    Xp = eng.set_prompt(zp)
    e, B, N, d = eng.embed, 3, eng.N, eng.d
    tn = ts([981, 402, 0], dev)
    nws = L.lib().avd_embed_workspace_floats(C.byref(e))
    tok = torch.empty(nws, device=dev)
    X2 = torch.full((2 * B, N, d), float("nan"), device=dev)
    L.check(L.lib().avd_embed_cfg_pair_f32(C.byref(e), z.data_ptr(), eng._aw.data_ptr(), eng._ab.data_ptr(), tn.data_ptr(), Xp.data_ptr(),
                                           tok.data_ptr(), X2.data_ptr(), L.stream_ptr(dev)))
    X1 = torch.full((B + 1, N, d), float("nan"), device=dev)           # one sample of slack: nothing may be written past B*N rows
    ss = torch.full((B * N + 8,), float("nan"), device=dev)
    L.check(L.lib().avd_embed_cond_f32(C.byref(e), z.data_ptr(), eng._aw.data_ptr(), eng._ab.data_ptr(), tn.data_ptr(), Xp.data_ptr(),
                                       tok.data_ptr(), X1.data_ptr(), ss.data_ptr(), L.stream_ptr(dev)))
    assert torch.isfinite(X2).all()
    assert torch.equal(X1[:B], X2[:B])
    assert torch.isnan(X1[B]).all() and torch.isnan(ss[B * N:]).all()
    # ss: the table the two-branch front end leaves in the step's workspace (right before the trailing eps region)
    D_ = eng.head.output_dims[target]
    eps_b = ((2 * B * e.Nt * D_ * 4 + 255) // 256) * 256
    ss_b = ((2 * B * N * 4 + 255) // 256) * 256
    out = eng.step(z, tn, ts([961, 382, -1], dev))
    end = eng.workspace.numel() - eps_b
    ss2 = eng.workspace[end - ss_b:end][: 2 * B * N * 4].view(torch.float32).clone()
    if temb_mode == "concat":
        assert torch.equal(ss[:B * N], ss2[:B * N])
        assert rel_err(ss[:B * N].cpu(), X1[:B].double().pow(2).sum(-1).reshape(-1).cpu()) < 1e-5
    else:
        assert torch.isnan(ss).all()                            # not written with temb_add
    assert torch.isfinite(out).all()


# ------------------------------------------------------------------------------------------------- 3. the step
def _oracle_eps_cond(ws, target, z, zp, tn, n_layers):
    """the oracle's conditional prediction: eps_pair(...)[0]"""
    tok_v = R.tube_patch(z if target == "video" else zp, 2, 4, 4)
    tok_a = R.audio_tokens(zp if target == "video" else z, 4, 4)
    t0 = torch.zeros_like(tn)
    Xv = R.embed_with_time(tok_v, ws["adapt_v"]["proj.weight"], ws["adapt_v"]["proj.bias"], tn if target == "video" else t0, 256)
    Xa = R.embed_with_time(tok_a, ws["adapt_a"]["proj.weight"], ws["adapt_a"]["proj.bias"], t0 if target == "video" else tn, 256)
    if target == "video":
        return R.eps_pair(Xv, Xa, True, ws["core"], ws["head"], "video", n_layers, 8)[0]
    return R.eps_pair(Xa, Xv, False, ws["core"], ws["head"], "audio", n_layers, 8)[0]


def _composed_from_tokens(dev, eng, target, eps, z, tn, tp):
    from multimodal_diffusion_amd import functional as Fn
    lat = Fn.tube_unpatch(eps, *z.shape[1:], 2, 4, 4) if target == "video" else Fn.audio_untokens(eps, z.shape[1], 4, z.shape[2], 4)
    return Fn.ddim_step(z, tn, tp, lat, ABAR)


def _check_cond_step(dev, model, n_layers, target, mode, z, zp, npr):
    ws = model[0]
    B = z.shape[0]
    tn, tp = ts([982, 500, 16, 999][:B], dev), ts([966, 480, -1, 979][:B], dev)
    with tuned("s3_min_rows"):
        if mode != "f32":
            tune("s3_min_rows", 0)             # let the split-operand kernels engage at these row counts
        eng = _engine(model[1], target, tuple(z.shape), npr, matmul=mode)
        eng.set_prompt(zp)
        out = eng.step(z, tn, tp, cond_only=True)
        eps = eng.eps_tokens()
        assert tuple(eps.shape) == (B, eng.embed.Nt, eng.head.output_dims[target])
        assert torch.equal(out, _composed_from_tokens(dev, eng, target, eps, z, tn, tp))
        ref = _oracle_eps_cond(ws, target, z.cpu(), zp.cpu(), tn.cpu(), n_layers)
        err = rel_err(eps.cpu(), ref)
        print(f"cond-only eps vs oracle eps_pair[0]: {target} {mode} L={n_layers} B={B}: rel_err {err:.3e}")
        assert err < TOL, (target, mode, err)
        # without the flag an engine that has an interval steps exactly as one that has none
        cfg = eng.step(z, tn, tp).clone()
        assert tuple(eng.eps_tokens().shape)[0] == 2 * B
        eng2 = _engine(model[1], target, tuple(z.shape), npr, matmul=mode, guidance_interval=(300, 700))
        eng2.set_prompt(zp)
        assert torch.equal(eng2.step(z, tn, tp), cfg)
        assert torch.equal(eng2.step(z, tn, tp, cond_only=True), out)
        assert not torch.equal(out, cfg)


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "f16x2"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_cond_step_small(dev, model, target, mode):
    z, zp, npr, _ = case(dev, target, B=2)
    _check_cond_step(dev, model, 2, target, mode, z, zp, npr)


@pytest.mark.parametrize("mode", ["f32", "bf16x3", "f16x2"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_cond_step_full_c3(dev, full, target, mode):
    """the C3 shape (256 x 256: 384 video + 37 audio tokens, d = 512, L = 8), both directions"""
    g = torch.Generator().manual_seed(256)
    zv, za = torch.randn(2, 8, 12, 32, 32, generator=g).to(dev), torch.randn(2, 8, 150, generator=g).to(dev)
    if target == "video":
        _check_cond_step(dev, full, 8, "video", mode, zv, za, 37)
    else:
        _check_cond_step(dev, full, 8, "audio", mode, za, zv, 384)


# ------------------------------------------------------------------------------------------------- 4. trajectories vs the oracle
def _oracle_traj(ws, target, z, zp, sched, interval, *, g=GS, solver="ddim", eta=0.0, noise=None):
    """step by step: guidance g inside the interval, 1.0 outside (e_n + 1 (e_c - e_n) = e_c up to a few ulp)"""
    import _dpm_ref as D
    B = z.shape[0]
    x, hist, t_last = z.clone(), np.zeros(tuple(z.shape)), -1
    kw = dict(adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"], head=ws["head"], n_layers=2, n_heads=8, eta=0.0,
              return_eps=True)
    kinds = IR.step_kinds(sched, interval)
    for i, cfg in enumerate(kinds):
        tn, tp = sched[i].repeat(B), sched[i + 1].repeat(B)
        step = R.denoise_step_a2v if target == "video" else R.denoise_step_v2a
        y, eps_tok = step(x, zp, tn, tp, ABAR, guidance=g if cfg else 1.0, **kw)
        if solver == "dpmpp_2m" or eta > 0:
            eps = R.tube_unpatch(eps_tok, *x.shape[1:], 2, 4, 4) if target == "video" else R.audio_untokens(eps_tok, x.shape[1], 4, x.shape[2], 4)
            if solver == "dpmpp_2m":
                y, hist = D.step_f64(x.numpy(), eps.numpy(), hist, ABAR.numpy(), [t_last] * B, tn.numpy(), tp.numpy())
                y = torch.from_numpy(y).float()
            else:
                y = R.ddim_update(x, tn, tp, eps, ABAR, eta=eta, noise=noise(tn))
        x, t_last = y, int(sched[i])
    return x.double()


TRAJ = [("ddim", 0.0), ("seeded", 0.6), ("dpmpp_2m", 0.0)]


@pytest.mark.parametrize("kind,eta", TRAJ)
@pytest.mark.parametrize("target", ["video", "audio"])
def test_trajectory_vs_oracle(dev, model, target, kind, eta):
    from multimodal_diffusion_amd import functional as Fn
    ws, _ = model
    n_steps = 8
    sched = R.sampling_schedule(1000, n_steps)                 # 999, 874, 749, 624, 499, 374, 249, 124, -1
    z, zp, npr, _ = case(dev, target, B=2, seed=2, W=16)
    kw = dict(matmul="f32")
    if kind == "seeded":
        kw.update(eta=eta, noise_seed=NSEED, sample_offset=3)
    if kind == "dpmpp_2m":
        kw.update(solver="dpmpp_2m")
    noise = (lambda tn: Fn.gaussian_noise(NSEED, 3, tn.to(dev), tuple(z.shape)).cpu()) if kind == "seeded" else None
    solver = "dpmpp_2m" if kind == "dpmpp_2m" else "ddim"
    plain = _engine(model[1], target, tuple(z.shape), npr, **kw)
    plain.set_prompt(zp)
    base = plain.run(z, sched)
    outs = {}
    for name, iv in (("middle", (300, 700)), ("all", (0, 999)), ("empty", (1000, 2000))):
        eng = _engine(model[1], target, tuple(z.shape), npr, guidance_interval=iv, **kw)
        eng.set_prompt(zp)
        out = eng.run(z, sched)
        outs[name] = out
        ref = _oracle_traj(ws, target, z.cpu(), zp.cpu(), sched, iv, solver=solver, eta=eta, noise=noise)
        l2 = float((out.cpu().double() - ref).norm() / ref.norm())
        print(f"trajectory {target} {kind} interval {name}: l2 {l2:.3e}")
        assert torch.isfinite(out).all() and l2 < 1e-3, (name, l2)      # chained tolerance of the existing trajectory tests
    assert torch.equal(outs["all"], base)                       # an interval covering everything is no interval, bit for bit
    assert not torch.equal(outs["middle"], base) and not torch.equal(outs["empty"], outs["middle"])
    if kind == "ddim":                                          # an empty interval is plain conditional sampling
        skw = dict(adapt_v=ws["adapt_v"], adapt_a=ws["adapt_a"], core=ws["core"], head=ws["head"], n_layers=2, n_heads=8, guidance=1.0)
        ref1 = (R.sample_a2v if target == "video" else R.sample_v2a)(z.cpu(), zp.cpu(), sched, ABAR, **skw).double()
        assert float((outs["empty"].cpu().double() - ref1).norm() / ref1.norm()) < 1e-3


# ------------------------------------------------------------------------------------------------- 5. graph = eager
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_graph_equals_eager(dev, model, solver):
    """segments of lengths 1, 2, an odd and an even number >= 3; plain, with a latent guide, with rescale active on the CFG steps"""
    from multimodal_diffusion_amd import schedule_utils as su
    z, zp, npr, known = case(dev, "video")
    if solver == "ddim":        # one run with four segments (DDIM takes any schedule)
        runs = [(torch.tensor([990, 900, 880, 400, 390, 380, 370, 360, 700, 650, 600, 550, -1]), (500, 950), [1, 2, 5, 4])]
    else:                       # a decreasing schedule has at most three segments: two intervals
        sched = torch.tensor([990, 900, 880, 840, 830, 820, 810, 800, -1])
        runs = [(sched, (860, 950), [1, 2, 5]), (sched, (0, 835), [4, 4])]
    eng = _engine(model[1], "video", tuple(z.shape), npr, solver=solver)
    eng.set_prompt(zp)
    last = None
    for setup in ("plain", "guide", "rescale"):
        if setup == "guide":
            eng.set_known(known, soft_mask(tuple(z.shape[1:])), guide_seed=GSEED)
        if setup == "rescale":
            eng.set_cfg(rescale=0.7)                            # acts on the CFG steps only
        for sched, iv, lens in runs:
            assert [b - a for a, b, _ in su.guidance_segments(sched, iv)] == lens
            gen = eng._generation
            eng.set_guidance_interval(iv)                       # the next run follows it; a host-side choice: no new generation
            assert eng._generation == gen
            zg = eng.run(z, sched, graph=True)
            ze = eng.run(z, sched, graph=False)
            assert torch.isfinite(zg).all() and torch.equal(zg, ze), (setup, iv)
            assert last is None or not torch.equal(zg, last)
            last = zg
    # back to no interval: today's run, bit for bit
    sched = runs[0][0]
    eng.set_guidance_interval(None)
    ref = _engine(model[1], "video", tuple(z.shape), npr, solver=solver, guidance_rescale=0.7)
    ref.set_prompt(zp)
    ref.set_known(known, soft_mask(tuple(z.shape[1:])), guide_seed=GSEED)
    assert torch.equal(eng.run(z, sched, graph=True), ref.run(z, sched, graph=True))


# ------------------------------------------------------------------------------------------------- 6. composition, invariance
@pytest.mark.parametrize("kw", [{}, dict(eta=0.7, noise_seed=NSEED), dict(solver="dpmpp_2m")])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_zero_mask_guide_is_no_guide(dev, model, target, kw):
    z, zp, npr, known = case(dev, target)
    eng = _engine(model[1], target, tuple(z.shape), npr, **kw)
    eng.set_prompt(zp)
    tn, tp = ts([981, 402], dev), ts([961, 382], dev)
    base = eng.step(z, tn, tp, cond_only=True).clone()
    eng.set_known(known, torch.zeros(tuple(z.shape[1:])), guide_seed=GSEED)
    assert torch.equal(eng.step(z, tn, tp, cond_only=True), base)
    eng.set_known(known, None, guide_seed=GSEED)               # all-one mask: q(t_prev)
    from multimodal_diffusion_amd import functional as Fn
    assert torch.equal(eng.step(z, tn, tp, cond_only=True), Fn.latent_guide(known, tp, ABAR, seed=GSEED))


def test_batch_offset_invariance(dev, model):
    """as test_gpu_latent_guide / test_gpu_seeded_noise: a batch of 4 is two batches of 2 at sample_offset 0 and 2"""
    z, zp, npr, known = case(dev, "video", B=4)
    m = soft_mask(tuple(z.shape), seed=8).to(dev)
    sched = R.sampling_schedule(1000, 4)

    def run(sl, off):
        eng = _engine(model[1], "video", (sl.stop - sl.start,) + tuple(z.shape[1:]), npr, matmul="f32", eta=0.5, noise_seed=1,
                      sample_offset=off, guidance_interval=(400, 800))
        eng.set_prompt(zp[sl].contiguous())
        eng.set_known(known[sl].contiguous(), m[sl].contiguous(), guide_seed=GSEED)
        return eng.run(z[sl].contiguous(), sched)

    o4 = run(slice(0, 4), 0)
    o2 = torch.cat([run(slice(0, 2), 0), run(slice(2, 4), 2)])
    # the model's GEMMs may round differently at another batch size: fp32 level; the kept region exactly
    assert float((o4 - o2).norm() / o4.norm()) < 1e-5
    keep = m == 1
    assert torch.equal(o4[keep], known[keep]) and torch.equal(o2[keep], known[keep])
    # the noise of a trajectory does not depend on the interval: a cond-only step draws what the CFG step would
    from multimodal_diffusion_amd import functional as Fn
    eng = _engine(model[1], "video", tuple(z.shape), npr, eta=0.5, noise_seed=1, sample_offset=6)
    eng.set_prompt(zp)
    tn, tp = ts([981, 402, 40, 700], dev), ts([961, 382, -1, 650], dev)
    out = eng.step(z, tn, tp, cond_only=True)
    lat = Fn.tube_unpatch(eng.eps_tokens(), *z.shape[1:], 2, 4, 4)
    assert torch.equal(out, Fn.ddim_step(z, tn, tp, lat, ABAR, 0.5, Fn.gaussian_noise(1, 6, tn, tuple(z.shape))))


@pytest.mark.parametrize("mode", ["f32", "f16x2"])
def test_split_streams_is_one_chain(dev, model, mode):
    z, zp, npr, _ = case(dev, "video")
    tn, tp = ts([981, 402], dev), ts([961, 382], dev)
    outs = []
    for split in (False, True):
        eng = _engine(model[1], "video", tuple(z.shape), npr, matmul=mode, split_streams=split)
        eng.set_prompt(zp)
        outs.append((eng.step(z, tn, tp, cond_only=True).clone(), eng.eps_tokens()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ------------------------------------------------------------------------------------------------- 7. entry points, misuse
@pytest.fixture(scope="module")
def a2v_setup(dev, model):
    vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=1.0, sampler_steps=6,
                               streaming={"window_seconds": 1.0, "hop_seconds": 0.5, "crossfade_seconds": 0.25},
                               sampling={"guidance_interval": {"video": [300, 700]}})
    wav = (0.1 * torch.randn(16000, generator=torch.Generator().manual_seed(9))).numpy()
    kw = dict(components(model[1], Recorder(vae), codec, dev), cfg=cfg, prompt_modality="audio", prompt_video=None, prompt_audio=wav)
    return kw, codec


def test_entry_points_follow_the_config_key(dev, model, a2v_setup):
    import copy
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import stream_infer as S
    kw, codec = a2v_setup
    lat = (1, 8, 4, 4, 4)
    noise = torch.randn(lat, generator=torch.Generator().manual_seed(4))
    A.sample_one_direction(init_noise=noise, **kw)
    got = kw["vid_vae"].last.clone()
    # the engine driven by hand
    with torch.no_grad():
        z_p = codec.encode(torch.from_numpy(kw["prompt_audio"]).to(dev).view(1, 1, -1)).float()
    sched = A.schedule_utils.make_sampling_schedule(1000, 6)
    eng = _engine(model[1], "video", lat, (z_p.shape[-1] - 4) // 4 + 1, guidance=2.0, guidance_interval=(300, 700))
    eng.set_prompt(z_p)
    hand = eng.run(noise.to(dev), sched)
    assert torch.equal(got, hand)
    # the argument wins over the key; no key and no argument is today's sampler
    nokey = copy.deepcopy(kw["cfg"])
    del nokey["sampling"]["guidance_interval"]
    kw2 = dict(kw, cfg=nokey)
    A.sample_one_direction(init_noise=noise, guidance_interval=(300, 700), **kw2)
    assert torch.equal(kw["vid_vae"].last, hand)
    A.sample_one_direction(init_noise=noise, **kw2)
    eng.set_guidance_interval(None)
    assert torch.equal(kw["vid_vae"].last, eng.run(noise.to(dev), sched)) and not torch.equal(kw["vid_vae"].last, hand)
    # stream_generate(shard=False): one window here, the same latent
    wav = kw["prompt_audio"]
    S.stream_generate(init_noise=noise, shard=False, **kw)
    assert torch.equal(kw["vid_vae"].last, hand)


def test_misuse(dev, model):
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import _lib as L, functional as Fn
    z, zp, npr, known = case(dev, "video")
    with pytest.raises(ValueError, match="guidance_interval"):
        _engine(model[1], "video", tuple(z.shape), npr, guidance_interval=(700, 300))
    eng = _engine(model[1], "video", tuple(z.shape), npr, solver="dpmpp_2m")
    eng.set_prompt(zp)
    with pytest.raises(ValueError, match="guidance_interval"):
        eng.set_guidance_interval((-3, 10))
    assert eng.guidance_interval is None
    tn, tp = ts([900, 900], dev), ts([800, 800], dev)
    out = torch.full_like(z, float("nan"))

    def cond(e, *, g=None, key=None, tl=None, h=None, noise=None, z_=None, out_=None):
        return L.lib().avd_denoise_step_cond_f32(C.byref(e.desc), None if g is None else C.byref(g), None if key is None else C.byref(key),
                                                 L.ptr(tl), L.ptr(h), (z if z_ is None else z_).data_ptr(), e.Xp.data_ptr(), tn.data_ptr(),
                                                 tp.data_ptr(), L.ptr(noise), (out if out_ is None else out_).data_ptr(),
                                                 e.workspace.data_ptr(), e.workspace.numel(), L.stream_ptr(dev))
    # wrong pointer combinations: t_last without x0_hist and the reverse; x0_hist aliasing z / z_out / the guide's known latent
    assert cond(eng, tl=eng._no_hist) == L.EINVAL
    assert cond(eng, h=eng.x0_hist) == L.EINVAL
    assert cond(eng, tl=eng._no_hist, h=z) == L.EINVAL
    assert cond(eng, tl=eng._no_hist, h=out) == L.EINVAL
    g = L.LatentGuide(eng.x0_hist.data_ptr(), None, 0, L.NoiseKey(1, 0))
    assert cond(eng, g=g, tl=eng._no_hist, h=eng.x0_hist) == L.EINVAL
    assert cond(eng, z_=out) == L.EINVAL                        # z_out aliases z
    with pytest.raises(L.AvdError, match="x0_hist"):
        eng.step(z, tn, tp, out=eng.x0_hist, cond_only=True)
    # eta > 0: no noise and no key; a guide without a key; noise together with a key or a guide
    ddim = _engine(model[1], "video", tuple(z.shape), npr, eta=0.5)
    ddim.set_prompt(zp)
    nz, key = torch.randn_like(z), Fn.noise_key(3, 0)
    gd = Fn.latent_guide_desc(known, None, GSEED, 0)
    assert cond(ddim) == L.EINVAL
    assert cond(ddim, g=gd) == L.EINVAL
    assert cond(ddim, g=gd, noise=nz) == L.EINVAL
    assert cond(ddim, key=key, noise=nz) == L.EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                               # nothing was launched
    assert cond(ddim, noise=nz) == 0 and torch.isfinite(out).all()      # unseeded noise without a guide is accepted
    assert torch.equal(out, ddim.step(z, tn, tp, noise=nz, cond_only=True))
    ddim.set_known(known, None)
    with pytest.raises(ValueError, match="noise_seed"):
        ddim.step(z, tn, tp, cond_only=True)
    # the kernel entries
    ab = ABAR.to(dev)
    eps = torch.randn(2, 64, 256, device=dev)

    def kern(eta, noise=None, key=None, tl=None, h=None, g=None, o=None):
        return L.lib().avd_eps_unpatch_ddim_f32(eps.data_ptr(), z.data_ptr(), tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), ab.numel(), eta,
                                                L.ptr(noise), (out if o is None else o).data_ptr(), 2, *z.shape[1:], 2, 4, 4,
                                                None if key is None else C.byref(key), L.ptr(tl), L.ptr(h),
                                                None if g is None else C.byref(g), L.stream_ptr(dev))
    out.fill_(float("nan"))
    assert kern(0.5) == L.EINVAL and kern(0.5, g=gd) == L.EINVAL and kern(0.0, tl=eng._no_hist) == L.EINVAL
    assert kern(0.0, h=eng.x0_hist) == L.EINVAL and kern(0.5, tl=eng._no_hist, h=eng.x0_hist) == L.EINVAL
    assert kern(0.0, tl=eng._no_hist, h=z) == L.EINVAL and kern(0.0, o=z) == L.EINVAL
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
    # eps_tokens after a cond-only step hands out no null rows
    eng.step(z, tn, tp, cond_only=True)
    assert eng.eps_tokens().shape[0] == 2
    eng.step(z, tn, tp)
    assert eng.eps_tokens().shape[0] == 4
