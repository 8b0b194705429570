"""Adaptive projected guidance on the MI355X (include/avdiff_hip.h, "adaptive projected guidance"): functional.apg_guidance against
the numpy mirror, the fused APG step against the composed path (eps tokens -> U -> apg_guidance -> the elementwise update -> the guide)
bit for bit over two steps for every solver, kernel form, noise, guide, momentum and guidance kind, canvas keying under a window
consensus, invariance to batching / split_streams / graph replay, non-interference with the steps that existed, the neutral
parameters against plain CFG within a derived rounding bound, a trajectory against the CPU oracle, the two pipelines, and misuse."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

import _apg_ref as AR
from _kit import (ABAR, STREAM_HALF_SECOND, Recorder, audio_prompt, case, components, dev, engine, matmul_f32, model,  # noqa: F401  (dev / model are fixtures)
                  pipeline, ts, video_case, with_sampling)
from _tune import cfg_rows  # noqa: F401  (fixture)
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
GS = 3.5
G2 = [2.0, 5.0]
GSEED = 77
APG = dict(norm_threshold=2.0, eta_parallel=0.25, momentum=-0.5)       # every part live at the kit's cases (|d| is 5 to 12 there)
_engine = partial(engine, guidance=GS)        # engine(mods, target, shape, n_prompt, **kw) at this file's guidance


def _untok(eng, tok):
    """U: tokens [B, N, D] -> the latent's natural layout (tube un-patch / overlap-add mean)"""
    from multimodal_diffusion_amd import functional as Fn
    shape = eng.latent_shape
    if eng.target == "video":
        return Fn.tube_unpatch(tok.contiguous(), *shape[1:], *eng.tube)
    return Fn.audio_untokens(tok.contiguous(), shape[1], eng.chunk[0], shape[2], eng.chunk[1])


def _pair(B, per, seed):
    """null = 0.5 cond + 0.5 xi with xi an independent normal (the coefficient checks' inputs)"""
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(B, per, generator=g)
    return c, 0.5 * c + 0.5 * torch.randn(B, per, generator=g)


# ------------------------------------------------------------------------------------------------- elementwise = numpy mirror
def test_functional_matches_mirror(dev):
    from multimodal_diffusion_amd import functional as Fn
    B, per = 3, 70_001                                          # not a multiple of 4 or of the 1024-element chunk
    c, u = _pair(B, per, 1)
    m0 = torch.randn(B, per, generator=torch.Generator().manual_seed(2))
    norm = float(np.sqrt(AR.moments(c.numpy(), AR.direction(c.numpy(), u.numpy()))[0]).mean())
    for g in (GS, [1.5, 3.5, 7.0]):
        for r, eta_p, beta in ((0.0, 0.0, 0.0), (0.5 * norm, 0.3, 0.0), (0.5 * norm, 0.5, -0.5), (4.0 * norm, 1.0, 0.75)):
            mom = m0.to(dev) if beta else None
            e_ref, d_ref, coef_ref = AR.apg(c.numpy(), u.numpy(), g, r, eta_p, beta, m0.numpy() if beta else None)
            assert AR.cancellation_free(c.numpy(), d_ref)
            out, coef = Fn.apg_guidance(c.to(dev), u.to(dev), g, norm_threshold=r, eta_parallel=eta_p, momentum=beta, momentum_buf=mom,
                                        return_coef=True)
            s, k, w = (t.cpu().numpy() for t in coef)
            for name, got, ref in zip("skw", (s, k, w), coef_ref):
                assert AR.ulps(got, ref).max() <= 2, (name, got, ref)
            if r == 0.0:
                assert (s == 1).all()
            if eta_p == 1.0:
                assert (k == 0).all()
            # the combine is elementwise: exact given the device's coefficients; so is the buffer's new content
            assert np.array_equal(out.cpu().numpy(), AR.combine_f32(c.numpy(), d_ref, w, k))
            if beta:
                assert np.array_equal(mom.cpu().numpy(), d_ref)
    # degenerate sums: c == 0 (S_cc == 0: k = 0) and c == u (S_dd == 0: s = 1)
    z = torch.zeros(2, 4096)
    out, (s, k, w) = Fn.apg_guidance(z.to(dev), u[:2, :4096].to(dev), GS, norm_threshold=1.0, return_coef=True)
    assert (k == 0).all() and torch.isfinite(out).all()
    out, (s, k, w) = Fn.apg_guidance(c[:2, :4096].to(dev), c[:2, :4096].to(dev), GS, norm_threshold=1.0, return_coef=True)
    assert (s == 1).all() and torch.equal(out.cpu(), c[:2, :4096])


def test_functional_is_batch_invariant(dev):
    from multimodal_diffusion_amd import functional as Fn
    c, u = _pair(4, 8 * 2 * 12 * 12, 3)                         # 2304 elements: two whole chunks and a ragged third
    m = torch.randn(c.shape, generator=torch.Generator().manual_seed(4))
    g4 = [2.0, 5.0, 3.0, 1.5]
    kw = dict(norm_threshold=20.0, eta_parallel=0.25, momentum=-0.5)

    def run(sl):
        mom = m[sl].to(dev).contiguous()
        out, coef = Fn.apg_guidance(c[sl].to(dev), u[sl].to(dev), g4[sl], momentum_buf=mom, return_coef=True, **kw)
        return [out, mom, *coef]

    whole = run(slice(0, 4))
    parts = [run(slice(0, 2)), run(slice(2, 4))]
    for i, t in enumerate(whole):
        assert torch.equal(t, torch.cat([p[i] for p in parts]))


# ------------------------------------------------------------------------------------------------- fused = composed, bit for bit
SOLVERS = {"ddim": {}, "ddim-seeded": dict(eta=0.7, noise_seed=5), "dpmpp_2m": dict(solver="dpmpp_2m"),
           "dpmpp_2m-sde": dict(solver="dpmpp_2m", eta=0.7, noise_seed=5)}
VARIANTS = [(0.0, GS), (-0.5, G2), (-0.5, GS), (0.0, G2)]      # (beta, guidance): no buffer / a buffer, scalar / per-sample


def _composed_step(eng, z, tn, tp, tl, h, mom, g, apg, kw, known, mask, noise=None):
    """one step of the composed path on the eps tokens the fused step left behind; h and mom are updated in place as the fused
    kernel updates x0_hist and the momentum buffer; returns (z_out, coefficients)"""
    from multimodal_diffusion_amd import functional as Fn
    B = z.shape[0]
    ep = eng.eps_tokens()
    c, u = _untok(eng, ep[:B]), _untok(eng, ep[B:])
    e, coef = Fn.apg_guidance(c, u, g, momentum_buf=mom, return_coef=True, **apg)
    eta = kw.get("eta", 0.0)
    if eta and noise is None:
        noise = Fn.gaussian_noise(kw["noise_seed"], 0, tn, tuple(z.shape))
    if kw.get("solver") == "dpmpp_2m":
        ref = Fn.dpmpp_2m_sde_step(z, e, h, tl, tn, tp, ABAR, eta, noise) if eta else Fn.dpmpp_2m_step(z, e, h, tl, tn, tp, ABAR)
    else:
        ref = Fn.ddim_step(z, tn, tp, e, ABAR, eta=eta, noise=noise)
    if mask is not None:
        ref = Fn.latent_guide(known, tp, ABAR, z=ref, mask=mask, seed=GSEED)
    return ref, (c, u, coef)


def _check_two_steps(dev, eng, cfg_rows, z, known, mask, kw, beta, g):
    """two consecutive fused APG steps against the composed path: z_out, the momentum buffer and x0_hist after each, bit for bit, in
    both video kernel forms; the second step reads the buffer the first one wrote"""
    dpm = kw.get("solver") == "dpmpp_2m"
    apg = dict(APG, momentum=beta)
    eng.set_cfg(guidance=g)
    eng.set_apg(**apg)
    if beta:
        eng.apg_momentum.zero_()
    h = torch.randn(z.shape, generator=torch.Generator().manual_seed(7)).to(dev) if dpm else None
    mom = torch.zeros_like(z) if beta else None
    steps = [(ts([981, 402], dev), ts([961, 382], dev), ts([999, 700], dev)), (ts([961, 382], dev), ts([941, 362], dev), ts([981, 402], dev))]
    x = z
    for i, (tn, tp, tl) in enumerate(steps):
        before = eng.apg_momentum.clone() if beta else None

        def fused():
            if dpm:
                eng.x0_hist.copy_(h)
            if beta:
                eng.apg_momentum.copy_(before)
            out = eng.step(x, tn, tp, t_last=tl if dpm else None).clone()
            return out, (eng.x0_hist.clone() if dpm else None), (eng.apg_momentum.clone() if beta else None)

        out, hist, m_after = fused()
        if eng.target == "video":                               # the gather form: bit-identical to the rows form
            cfg_rows(0)
            out0, hist0, m0 = fused()
            cfg_rows(1)
            assert torch.equal(out0, out)
            assert hist is None or torch.equal(hist0, hist)
            assert m_after is None or torch.equal(m0, m_after)
        ref, (c, u, coef) = _composed_step(eng, x, tn, tp, tl, h, mom, g, apg, kw, known, mask)
        assert torch.isfinite(out).all()
        assert torch.equal(out, ref), (i, float((out - ref).abs().max()))
        if beta:
            assert torch.equal(m_after, mom)
            assert i == 0 or not torch.equal(m_after, c - u)    # the second step read a non-zero buffer
        if dpm:
            assert torch.equal(hist, h)
        s, k, w = coef
        assert bool((s < 1).any()) and bool((k != 0).all())     # the cap and the projection are live at these inputs
        x = out
    return out


@pytest.mark.parametrize("guided", [False, True], ids=["free", "guided"])
@pytest.mark.parametrize("solver", list(SOLVERS))
@pytest.mark.parametrize("target", ["video", "audio"])
def test_fused_equals_composed(dev, model, cfg_rows, target, solver, guided):
    kw = SOLVERS[solver]
    z, zp, npr, known = case(dev, target)
    eng = _engine(model[1], target, tuple(z.shape), npr, apg=APG, **kw)
    eng.set_prompt(zp)
    mask = None
    if guided:
        mask = torch.rand(tuple(z.shape[1:]), generator=torch.Generator().manual_seed(3))
        mask[mask < 0.35] = 0.0
        mask = mask.to(dev)
        eng.set_known(known, mask, guide_seed=GSEED)
    outs = [_check_two_steps(dev, eng, cfg_rows, z, known, mask, kw, beta, g) for beta, g in VARIANTS]
    assert not torch.equal(outs[0], outs[2]) and not torch.equal(outs[0], outs[3])      # momentum and the per-sample scale are live


def test_fused_equals_composed_ragged_chunks(dev, model, cfg_rows):
    """a video latent of 2304 elements per sample: two whole 1024-element chunks and a ragged third (the gather form: no latent the
    whole-line kernel takes has a per_sample that is not a multiple of 1024 at this head width)"""
    g = torch.Generator().manual_seed(6)
    shape = (2, 8, 2, 12, 12)
    z, zp, known = (torch.randn(s, generator=g).to(dev) for s in (shape, (2, 8, 40), shape))
    assert int(np.prod(shape[1:])) % 1024 == 256
    eng = _engine(model[1], "video", shape, 10, apg=APG, solver="dpmpp_2m")
    eng.set_prompt(zp)
    _check_two_steps(dev, eng, cfg_rows, z, known, None, SOLVERS["dpmpp_2m"], -0.5, G2)


# ------------------------------------------------------------------------------------------------- canvas keying
def test_canvas_keyed_consensus_step_equals_composed(dev, model):
    from multimodal_diffusion_amd import functional as Fn
    z, za, npr = video_case(dev, B=3, W=16)
    hop, seed, eta = 2, 0xDEADBEEF12345678, 0.5
    tn, tp = ts([900] * 3, dev), ts([700] * 3, dev)
    kw = dict(eta=eta, noise_seed=seed)
    eng = _engine(model[1], "video", tuple(z.shape), npr, noise_keying="canvas", canvas_hop=hop, apg=APG, guidance=[2.0, 3.5, 5.0], **kw)
    eng.set_prompt(za)
    eng.set_window_consensus(hop)
    out = eng.step(z, tn, tp)
    mom = torch.zeros_like(z)
    ref, _ = _composed_step(eng, z, tn, tp, None, None, mom, [2.0, 3.5, 5.0], APG, kw, None, None,
                            noise=Fn.canvas_noise(seed, tn, tuple(z.shape), hop))
    assert torch.equal(out, Fn.window_consensus(ref, hop))
    assert torch.equal(eng.apg_momentum, mom)                   # the buffer stays per window: no consensus touches it


# ------------------------------------------------------------------------------------------------- invariance
def test_batch_split_with_sample_offset(dev, model):
    z, zp, npr, _ = case(dev, "video", B=4)
    g4 = [2.0, 5.0, 3.0, 1.5]
    sched = R.sampling_schedule(1000, 4)

    def run(sl, **kw):
        eng = _engine(model[1], "video", (sl.stop - sl.start,) + tuple(z.shape[1:]), npr, matmul="f32", eta=0.5, noise_seed=9,
                      sample_offset=sl.start, **kw)
        eng.set_prompt(zp[sl].contiguous())
        out = eng.run(z[sl].contiguous(), sched)
        return out, eng.apg_momentum

    halves = (slice(0, 2), slice(2, 4))
    whole, mw = run(slice(0, 4), guidance=g4, apg=APG)
    parts = [run(s, guidance=g4[s], apg=APG) for s in halves]
    plain4, _ = run(slice(0, 4))
    plain2 = torch.cat([run(s)[0] for s in halves])
    assert not torch.equal(whole, plain4)
    if torch.equal(plain4, plain2):
        # the model itself is batch-invariant here: then APG must be too (the coefficients depend on the sample alone)
        assert torch.equal(whole, torch.cat([p[0] for p in parts])) and torch.equal(mw, torch.cat([p[1] for p in parts]))
    else:
        assert float((whole - torch.cat([p[0] for p in parts])).norm() / whole.norm()) < 1e-5


@pytest.mark.parametrize("target", ["video", "audio"])
def test_split_streams(dev, model, target):
    z, zp, npr, _ = case(dev, target)
    tn, tp = ts([981, 402], dev), ts([961, 382], dev)
    outs = []
    for split in (True, False):
        eng = _engine(model[1], target, tuple(z.shape), npr, guidance=G2, apg=APG, matmul="f16x2", split_streams=split)
        eng.set_prompt(zp)
        outs.append((eng.step(z, tn, tp), eng.apg_momentum.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_graph_replay_equals_eager_and_follows_set_apg(dev, model, solver):
    from multimodal_diffusion_amd import _lib as L
    z, zp, npr, _ = case(dev, "video")
    sched = R.sampling_schedule(1000, 4)
    eng = _engine(model[1], "video", tuple(z.shape), npr, guidance=G2, apg=APG, solver=solver)
    eng.set_prompt(zp)
    zg, mg = eng.run(z, sched, graph=True), eng.apg_momentum.clone()
    ze, me = eng.run(z, sched, graph=False), eng.apg_momentum.clone()
    assert torch.equal(zg, ze) and torch.equal(mg, me) and bool((mg != 0).any())
    # a captured pair updates the buffer in place, at its address; new parameters start a new generation: the pair is not served stale
    eng.begin(sched)
    a, b = z.clone(), torch.empty_like(z)
    eng.advance(a, b)
    a, b = b, a
    ptr, gen = eng.apg_momentum.data_ptr(), eng._generation
    pair = eng.capture_pair(a, b)
    pair.replay()
    eng.advance(a, b)
    assert torch.equal(b, ze) and eng.apg_momentum.data_ptr() == ptr and torch.equal(eng.apg_momentum, me)
    eng.set_apg(**APG)                                          # the same values: nothing a graph holds has changed
    assert eng._generation == gen
    eng.set_apg(**dict(APG, eta_parallel=0.5))
    assert eng._generation == gen + 1
    with pytest.raises(L.AvdError, match="stale"):
        pair.replay()
    eng.clear_apg()
    assert eng._generation == gen + 2 and eng._apg is None


# ------------------------------------------------------------------------------------------------- non-interference
@pytest.mark.parametrize("target", ["video", "audio"])
def test_apg_off_is_todays_step(dev, model, target):
    """an engine whose APG was set and cleared, and a control without APG, take the launches they took before APG existed: the same
    bits as an engine that never heard of it (the controlled kernels branch on a null APG part at run time)"""
    z, zp, npr, _ = case(dev, target)
    tn, tp = ts([981, 402], dev), ts([961, 382], dev)

    def fresh(**kw):
        eng = _engine(model[1], target, tuple(z.shape), npr, **kw)
        eng.set_prompt(zp)
        return eng

    plain = fresh().step(z, tn, tp)
    eng = fresh(apg=APG)
    assert not torch.equal(eng.step(z, tn, tp), plain)
    eng.clear_apg()
    assert eng._apg is None and eng._ctl is None and torch.equal(eng.step(z, tn, tp), plain)
    assert fresh(apg=None)._apg_stats is None
    ctl = fresh(guidance=G2, guidance_rescale=[0.7, 0.3]).step(z, tn, tp)
    eng = fresh(guidance=G2, apg=APG)
    eng.clear_apg()
    eng.set_cfg(rescale=[0.7, 0.3])
    assert torch.equal(eng.step(z, tn, tp), ctl)
    arr = fresh(guidance=[GS, GS]).step(z, tn, tp)              # the controlled kernel without rescale or APG: the scalar's bits
    assert torch.equal(arr, plain)


def test_cond_only_step_leaves_the_buffer(dev, model):
    z, zp, npr, _ = case(dev, "video")
    sched = torch.tensor([900, 700, 500, 300, 100])
    eng = _engine(model[1], "video", tuple(z.shape), npr, apg=APG, guidance_interval=(400, 800))
    eng.set_prompt(zp)
    tn, tp = ts([900, 900], dev), ts([700, 700], dev)
    eng.step(z, ts([700, 700], dev), ts([500, 500], dev))       # a CFG step: the buffer is written
    m = eng.apg_momentum.clone()
    assert bool((m != 0).any())
    cond = eng.step(z, tn, tp, cond_only=True)
    assert torch.equal(eng.apg_momentum, m)                     # bit-unchanged across a cond-only step
    off = _engine(model[1], "video", tuple(z.shape), npr)
    off.set_prompt(zp)
    assert torch.equal(cond, off.step(z, tn, tp, cond_only=True))
    # run(): 900 is outside the interval (cond-only), 700 and 500 inside, 300 outside; graph and eager agree
    assert torch.equal(eng.run(z, sched, graph=True), eng.run(z, sched, graph=False))


# ------------------------------------------------------------------------------------------------- neutral parameters
@pytest.mark.parametrize("target", ["video", "audio"])
def test_neutral_parameters_against_plain_cfg(dev, model, target):
    """r = 0, eta_p = 1, beta = 0 is plain CFG mathematically, not in bits.  The fused APG step against an fp64 evaluation of the plain
    DDIM step on the same eps, elementwise, within a bound propagated from the fp32 roundings (u = 2^-24 each):
      item 5: d = fl(c - u) and w d and c + w d round once each (k = 0 and d - 0 are exact; w = g - 1 = 2.5 is exact), so
              |e - e*| <= u (3 (g - 1) |d| + |c|)                       with e* = c + (g - 1)(c - u) = u + g (c - u);
      update: o = A x0 + Ce e with x0 = (x - So e) / Dn, so do/de = J = Ce - A So / Dn and e's error reaches o as |J| |e - e*|;
              the update's own six operations round once each on partial results no larger than M = (A / Dn)(|x| + So |e*|) + Ce |e*|,
              and each of the four fp32 coefficients may differ from this test's numpy evaluation by an ulp: 14 u M in all.
    Observed maxima of |o - o*| / bound are recorded in DESIGN.md 4.6."""
    z, zp, npr, _ = case(dev, target)
    B = z.shape[0]
    tn, tp = [981, 402], [961, 382]
    eng = _engine(model[1], target, tuple(z.shape), npr, apg=dict(norm_threshold=0.0, eta_parallel=1.0, momentum=0.0))
    eng.set_prompt(zp)
    out = eng.step(z, ts(tn, dev), ts(tp, dev)).cpu().numpy().astype(np.float64)
    ep = eng.eps_tokens()
    c, u = (_untok(eng, t).cpu().numpy().astype(np.float64) for t in (ep[:B], ep[B:]))
    x = z.cpu().numpy().astype(np.float64)
    ab = ABAR.numpy().astype(np.float32)
    sh = (B,) + (1,) * (z.dim() - 1)
    a_t, a_p = ab[tn], ab[tp]
    So = np.sqrt(np.maximum(np.float32(1) - a_t, 0)).astype(np.float64).reshape(sh)
    Dn = np.maximum(np.sqrt(a_t), np.float32(1e-8)).astype(np.float64).reshape(sh)
    A = np.sqrt(a_p).astype(np.float64).reshape(sh)
    Ce = np.sqrt(np.maximum(np.float32(1) - a_p, 0)).astype(np.float64).reshape(sh)
    e_star = u + GS * (c - u)
    o_star = A * ((x - So * e_star) / Dn) + Ce * e_star
    uro = 2.0 ** -24
    de = uro * (3 * (GS - 1) * np.abs(c - u) + np.abs(c))
    J = np.abs(Ce - A * So / Dn)
    M = (A / Dn) * (np.abs(x) + So * np.abs(e_star)) + Ce * np.abs(e_star)
    bound = J * de + 14 * uro * M
    ratio = np.abs(out - o_star) / bound
    print(f"neutral APG vs fp64 plain CFG step ({target}): max |o - o*| = {np.abs(out - o_star).max():.3e}, max ratio to bound = {ratio.max():.3f}")
    assert ratio.max() <= 1.0
    plain = _engine(model[1], target, tuple(z.shape), npr)
    plain.set_prompt(zp)
    p = plain.step(z, ts(tn, dev), ts(tp, dev)).cpu().numpy().astype(np.float64)
    print(f"  against the plain fused step's bits: max |difference| = {np.abs(out - p).max():.3e}")


# ------------------------------------------------------------------------------------------------- trajectory vs the oracle
def _oracle_step(ws, target, x, zp, tn, tp, g, apg, m):
    if target == "video":
        tok_t, tok_p = R.tube_patch(x, 2, 4, 4), R.audio_tokens(zp, 4, 4)
        at, ap = ws["adapt_v"], ws["adapt_a"]
    else:
        tok_t, tok_p = R.audio_tokens(x, 4, 4), R.tube_patch(zp, 2, 4, 4)
        at, ap = ws["adapt_a"], ws["adapt_v"]
    Xt = R.embed_with_time(tok_t, at["proj.weight"], at["proj.bias"], tn, 256)
    Xp = R.embed_with_time(tok_p, ap["proj.weight"], ap["proj.bias"], torch.zeros_like(tn), 256)
    ec, en = R.eps_pair(Xt, Xp, target == "video", ws["core"], ws["head"], target, 2, 8)
    if target == "video":
        U = lambda t: R.tube_unpatch(t, *x.shape[1:], 2, 4, 4)          # noqa: E731
    else:
        U = lambda t: R.audio_untokens(t, x.shape[1], 4, x.shape[2], 4)  # noqa: E731
    e, d, _ = AR.apg(U(ec).numpy(), U(en).numpy(), g, apg["norm_threshold"], apg["eta_parallel"], apg["momentum"], m)
    return R.ddim_update(x, tn, tp, torch.from_numpy(e), ABAR), d


@pytest.mark.parametrize("target", ["video", "audio"])
def test_trajectory_vs_oracle(dev, model, target):
    ws, _ = model
    n_steps = 8
    sched = R.sampling_schedule(1000, n_steps)
    gen = torch.Generator().manual_seed(2)
    if target == "video":
        z, zp, npr = torch.randn(2, 8, 4, 16, 16, generator=gen), torch.randn(2, 8, 40, generator=gen), 10
    else:
        z, zp, npr = torch.randn(2, 8, 40, generator=gen), torch.randn(2, 8, 4, 8, 8, generator=gen), 8
    apg = APG
    eng = _engine(model[1], target, tuple(z.shape), npr, guidance=G2, apg=apg, matmul="f32")
    eng.set_prompt(zp.to(dev))
    out = eng.run(z.to(dev), sched).cpu().double()
    x, m = z.clone(), np.zeros(tuple(z.shape), np.float32)
    for i in range(n_steps):
        x, m = _oracle_step(ws, target, x, zp, sched[i].repeat(2), sched[i + 1].repeat(2), G2, apg, m)
    ref = x.double()
    assert float((out - ref).norm() / ref.norm()) < 1e-3        # test_gpu_cfg_rescale.py::test_trajectory_vs_oracle's tolerance
    assert float((eng.apg_momentum.cpu().double() - torch.from_numpy(m).double()).norm() / np.linalg.norm(m)) < 1e-3


# ------------------------------------------------------------------------------------------------- the pipelines
def test_sample_one_direction_apg(dev, model):
    import multimodal_diffusion_amd as A
    vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=1.0, sampler_steps=5, sampling={"guidance_scale": {"video": 4.0, "audio": 4.0}})
    vae = Recorder(vae)
    wav = (0.1 * torch.randn(16000, generator=torch.Generator().manual_seed(9))).numpy()
    kw = dict(components(model[1], vae, codec, dev), prompt_modality="audio", prompt_video=None, prompt_audio=wav)
    noise = torch.randn(1, 8, 4, 4, 4, generator=torch.Generator().manual_seed(4))
    a = A.sample_one_direction(cfg=cfg, init_noise=noise, **kw)
    za = vae.last
    b = A.sample_one_direction(cfg=with_sampling(cfg, apg={"audio": {"momentum": -0.5}}), init_noise=noise, **kw)
    assert np.array_equal(a["video"], b["video"]) and torch.equal(vae.last, za)      # the other target's entry: nothing changes
    c = A.sample_one_direction(cfg=with_sampling(cfg, apg={"video": dict(APG, norm_threshold=5.0)}), init_noise=noise, **kw)
    assert c["video"].shape == a["video"].shape
    assert torch.isfinite(vae.last).all() and not torch.equal(vae.last, za)
    with pytest.raises(ValueError, match="guidance_rescale"):
        A.sample_one_direction(cfg=with_sampling(cfg, apg={"video": {}}, guidance_rescale={"video": 0.5}), init_noise=noise, **kw)


def test_stream_generate_apg(dev, model):
    from multimodal_diffusion_amd import stream_infer as S
    with matmul_f32(model[1]):
        vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND)
        kw = dict(components(model[1], vae, codec, dev), shard=False, return_latents=True, **audio_prompt())
        free = S.stream_generate(cfg=cfg, **kw)["latents"]
        on = with_sampling(cfg, apg={"video": dict(APG, norm_threshold=3.0)})
        whole = S.stream_generate(cfg=on, **kw)["latents"]
        assert np.isfinite(whole).all() and whole.shape == free.shape and not np.array_equal(whole, free)
        part = S.stream_generate(cfg=on, max_windows_per_batch=1, **kw)["latents"]
        assert np.array_equal(part, whole)                      # every window is its own sample
        cons = S.stream_generate(cfg=on, consensus="uniform", **kw)["latents"]
        assert np.array_equal(S.stream_generate(cfg=on, consensus="uniform", max_windows_per_batch=2, **kw)["latents"], cons)


# ------------------------------------------------------------------------------------------------- misuse
def test_misuse(dev, model):
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn
    z, zp, npr, _ = case(dev, "video")
    mk = partial(_engine, model[1], "video", tuple(z.shape), npr)
    for bad in (dict(apg={"eta_parallel": 1.5}), dict(apg={"norm_threshold": -1.0}), dict(apg={"momentum": float("nan")}),
                dict(apg={"norm_threshold": float("nan")}), dict(apg={"beta": 0.5}), dict(apg=0.5),
                dict(apg=APG, guidance_rescale=0.5), dict(apg={}, guidance_rescale=[0.0, 0.2])):
        with pytest.raises(ValueError):
            mk(**bad)
    eng = mk(solver="dpmpp_2m", apg=APG)
    eng.set_prompt(zp)
    gen, vals = eng._generation, eng._apg_vals
    for bad in (dict(eta_parallel=-0.1), dict(norm_threshold=float("inf")), dict(momentum=float("nan"))):
        with pytest.raises(ValueError, match="apg"):
            eng.set_apg(**bad)
    with pytest.raises(ValueError, match="guidance_rescale"):
        eng.set_cfg(rescale=0.3)
    resc = mk(guidance_rescale=0.3)
    with pytest.raises(ValueError, match="guidance_rescale"):
        resc.set_apg()
    assert eng._generation == gen and eng._apg_vals == vals and resc._apg is None      # nothing changed
    # slot timesteps and the FIFO queue refuse it, as every CFG control
    S = eng.slots
    tab = torch.full((2, S), 500, dtype=torch.long, device=dev)
    with pytest.raises(ValueError, match="adaptive projected guidance"):
        eng.step_slots(z, tab, tab - 20, t_last=tab + 20)
    with pytest.raises(ValueError, match="adaptive projected guidance"):
        eng._slot_refusals(True)                                # what fifo_open asks before it allocates
    # noise= with APG at eta > 0, seeded or not
    tn, tp = ts([900, 900], dev), ts([800, 800], dev)
    for kw in (dict(eta=0.5), dict(eta=0.5, noise_seed=1)):
        noisy = mk(apg=APG, **kw)
        noisy.set_prompt(zp)
        with pytest.raises(ValueError, match="noise"):
            noisy.step(z, tn, tp, noise=torch.randn_like(z))
    with pytest.raises(ValueError, match="noise_seed"):
        noisy = mk(apg=APG, eta=0.5)
        noisy.set_prompt(zp)
        noisy.step(z, tn, tp)
    # the functional op
    with pytest.raises(ValueError, match="momentum_buf"):
        Fn.apg_guidance(z, z, GS, momentum=-0.5)
    with pytest.raises(ValueError, match="momentum_buf"):
        Fn.apg_guidance(z, z, GS, momentum_buf=torch.zeros_like(z))
    with pytest.raises(ValueError, match="momentum_buf"):
        Fn.apg_guidance(z, z, GS, momentum=-0.5, momentum_buf=torch.zeros_like(z)[:, :4])
    with pytest.raises(ValueError, match="eta_parallel"):
        Fn.apg_guidance(z, z, GS, eta_parallel=1.01)
    with pytest.raises(ValueError):
        Fn.apg_guidance(z[:, :1, :1, :1, :1].contiguous(), z[:, :1, :1, :1, :1].contiguous(), GS)      # one element per sample
    # the C entry: the scratch or the buffer on z_out / x0_hist / the workspace, refused before any launch
    out = torch.full_like(z, 7.0)
    a = eng._apg

    def call(c):
        return L.lib().avd_denoise_step_apg_f32(C.byref(eng.desc), C.byref(c), None, None, None, 0, 0, eng._no_hist.data_ptr(),
                                                eng.x0_hist.data_ptr(), z.data_ptr(), eng.Xp.data_ptr(), tn.data_ptr(), tp.data_ptr(),
                                                out.data_ptr(), eng.workspace.data_ptr(), eng.workspace.numel(), L.stream_ptr(dev))

    A_ = lambda mom=a.momentum_buf, st=a.stats, sb=a.stats_bytes, beta=a.momentum: L.ApgControl(a.norm_threshold, a.eta_parallel, beta, mom, st, sb)  # noqa: E731
    mom0 = eng.apg_momentum.clone()
    for bad in (A_(mom=out.data_ptr()), A_(mom=eng.x0_hist.data_ptr()), A_(mom=z.data_ptr()), A_(mom=eng.workspace.data_ptr()),
                A_(st=out.data_ptr()), A_(st=eng.x0_hist.data_ptr()), A_(sb=a.stats_bytes - 16), A_(st=None, sb=0), A_(mom=None),
                A_(beta=0.0)):
        assert call(bad) == L.EINVAL
    assert call(A_(st=a.stats + 8)) == L.EUNSUPPORTED and call(A_(mom=a.momentum_buf + 4)) == L.EUNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(eng.apg_momentum, mom0)
    assert call(a) == 0                                                   # the engine's own control goes through
