"""Stochastic slot steps and FIFO denoising on the MI355X (include/avdiff_hip.h, "clip-keyed slot noise"): the whole step on an eta > 0
engine with ``clip_first`` against the unseeded step fed ``slot_noise``, against its explicit composition and against the CPU oracle;
``fifo_denoise`` on both solvers in its three drivers against the loop of its parts; and the refusals."""
import pytest
import torch

import _lookahead_ref as LR
import _slot_dpm_ref as SD
import _slot_noise_ref as SN
import _slot_ref as SR
from _kit import ABAR, case, dev, engine, model, ts  # noqa: F401  (dev, model are fixtures)
from _tune import tuned
from conftest import rel_err
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

GS = 3.5
TOL = 1e-4          # the parity tolerance of test_gpu_parity.py
SEED = 0x5EED0F1F0          # the queue's start and entering noise
ESEED = 0x51075EED          # the engines' noise_seed: the step noise
SCHED4 = torch.tensor([999, 749, 499, 249, -1])
SOLVERS = [("ddim", 0.5), ("dpmpp_2m", 1.0)]


def cur(dev, v):
    return torch.tensor([v], dtype=torch.int32, device=dev)


def _uniform(t, B, S, dev):
    return torch.tensor(t, dtype=torch.long, device=dev)[:, None].expand(B, S).contiguous()


# ------------------------------------------------------------------------------------------------- 4. the whole step, uniform tables
@pytest.mark.parametrize("split_streams", [False, True])
@pytest.mark.parametrize("matmul", ["f32", None])          # None: the engine's default mode
@pytest.mark.parametrize("target", ["video", "audio"])
def test_uniform_tables_give_the_unseeded_step_on_slot_noise(dev, model, target, matmul, split_streams):
    from multimodal_diffusion_amd import functional as Fn
    z, zp, npr, _ = case(dev, target, B=2)
    kw = dict(guidance=GS, eta=0.5, split_streams=split_streams, **({} if matmul is None else {"matmul": matmul}))
    eng = engine(model[1], target, tuple(z.shape), npr, noise_seed=ESEED, **kw)
    plain = engine(model[1], target, tuple(z.shape), npr, **kw)
    eng.set_prompt(zp)
    plain.set_prompt(zp)
    tn, tp = [981, 402], [961, 382]
    S, sl = eng.slots, eng.slot_len
    tabs = _uniform(tn, 2, S, dev), _uniform(tp, 2, S, dev)
    cursor = cur(dev, 4)
    out = eng.step_slots(z, *tabs, clip_first=-1, clip_stride=S + 1, clip_cursor=cursor)
    noise = Fn.slot_noise(ESEED, tabs[0], tuple(z.shape), sl, first=3, stride=S + 1)
    ref = plain.step(z, ts(tn, dev), ts(tp, dev), noise=noise)
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref), float((out - ref).abs().max())
    assert not torch.equal(out, plain.step(z, ts(tn, dev), ts(tp, dev), noise=torch.zeros_like(z)))      # the noise term is live
    # the defaults: clip_stride None = S, no cursor
    assert torch.equal(eng.step_slots(z, *tabs, clip_first=3),
                       plain.step(z, ts(tn, dev), ts(tp, dev), noise=Fn.slot_noise(ESEED, tabs[0], tuple(z.shape), sl, first=3)))


# ------------------------------------------------------------------------------------------------- 5. the whole step, mixed tables
def _eps_latent(eng, target, z):
    """the step's own eps tokens -> the CFG combine (two roundings, as the kernel's) -> un-patch / overlap-add, on the device"""
    from multimodal_diffusion_amd import functional as Fn
    tok = eng.eps_tokens()
    B = z.shape[0]
    e_tok = tok[B:] + GS * (tok[:B] - tok[B:])
    if target == "video":
        return Fn.tube_unpatch(e_tok, *z.shape[1:], *eng.tube)
    return Fn.audio_untokens(e_tok, z.shape[1], eng.chunk[0], z.shape[2], eng.chunk[1])


def _oracle_step(ws, target, z, zp, tn, tp, eta, noise, tube=(2, 4, 4), chunk=(4, 4), tdim=256):
    """_slot_ref.step_slots with the DDIM noise term: the oracle's step on slot timesteps, R.ddim_update(eta=, noise=) per position"""
    B, S, L_ = z.shape[0], tn.shape[1], z.shape[2]
    if target == "video":
        _, C_, T, H, W = z.shape
        tok, tokp = R.tube_patch(z, *tube), R.audio_tokens(zp, *chunk)
        at, ap, per_slot, slot_len = ws["adapt_v"], ws["adapt_a"], tok.shape[1] // S, tube[0]
    else:
        _, Ca, F = z.shape
        tok, tokp = R.audio_tokens(z, *chunk), R.tube_patch(zp, *tube)
        at, ap, per_slot, slot_len = ws["adapt_a"], ws["adapt_v"], 1, chunk[0]
    slot = torch.arange(tok.shape[1]) // per_slot
    x = R.linear(tok, at["proj.weight"], at["proj.bias"])
    e = R.timestep_embedding(tn[:, slot].reshape(-1), tdim).view(B, tok.shape[1], tdim)
    Xp = R.embed_with_time(tokp, ap["proj.weight"], ap["proj.bias"], torch.zeros(B, dtype=torch.long), tdim)
    e_c, e_n = R.eps_pair(torch.cat([x, e], -1), Xp, target == "video", ws["core"], ws["head"], target, 2, 8)
    eps_tok = e_n + GS * (e_c - e_n)
    eps = R.tube_unpatch(eps_tok, C_, T, H, W, *tube) if target == "video" else R.audio_untokens(eps_tok, Ca, chunk[0], F, chunk[1])
    sl = SR.slot_of_position(L_, slot_len, S)
    rows = lambda v: v.movedim(2, 1).reshape((B * L_,) + tuple(v.shape[1:2]) + tuple(v.shape[3:]))
    out = R.ddim_update(rows(z), tn[:, sl].reshape(-1), tp[:, sl].reshape(-1), rows(eps), R.alpha_bar_table(R.beta_table(1000)),
                        eta=eta, noise=rows(noise))
    out = out.view((B, L_) + tuple(z.shape[1:2]) + tuple(z.shape[3:])).movedim(1, 2)
    hold = SR.per_position(tn, L_, slot_len, z) == SR.per_position(tp, L_, slot_len, z)
    return torch.where(hold, z, out)


@pytest.mark.parametrize("matmul", ["f32", "bf16x3"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_mixed_tables_ddim_against_the_composition_and_the_oracle(dev, model, target, matmul):
    from multimodal_diffusion_amd import functional as Fn
    ws, mods = model
    z, zp, npr, _ = case(dev, target, B=2)
    eta, first = 0.5, 6
    with tuned(s3_min_rows=0):
        eng = engine(mods, target, tuple(z.shape), npr, guidance=GS, matmul=matmul, eta=eta, noise_seed=ESEED)
        eng.set_prompt(zp)
        tn, tp = SR.tables(2, eng.slots, seed=21)
        out = eng.step_slots(z, tn, tp, clip_first=first)
    sl = eng.slot_len
    noise = Fn.slot_noise(ESEED, tn, tuple(z.shape), sl, first=first)
    comp = Fn.ddim_step_slots(z, tn, tp, _eps_latent(eng, target, z), ABAR, sl, eta=eta, noise=noise)
    assert torch.isfinite(out).all()
    assert torch.equal(out, comp), float((out - comp).abs().max())
    mirror = torch.from_numpy(SN.normals(ESEED, tn.numpy(), tuple(z.shape), sl, first=first)).float()
    ref = _oracle_step(ws, target, z.cpu(), zp.cpu(), tn, tp, eta, mirror)
    err = rel_err(out.cpu(), ref)
    print(f"stochastic slot step vs oracle ({target}, {matmul}): rel err {err:.3e}")
    assert err < TOL
    hold = (SR.per_position(tn, z.shape[2], sl, z) == SR.per_position(tp, z.shape[2], sl, z)).expand_as(z).to(dev)
    assert hold.any() and torch.equal(out[hold], z[hold])                       # held slots: z, bit for bit
    # the noise term is live on the stepping slots: the eta == 0 engine gives another latent there
    det = engine(mods, target, tuple(z.shape), npr, guidance=GS, matmul=matmul)
    det.set_prompt(zp)
    with tuned(s3_min_rows=0):
        assert not torch.equal(det.step_slots(z, tn, tp)[~hold], out[~hold])


@pytest.mark.parametrize("target", ["video", "audio"])
def test_mixed_tables_sde_against_the_composition(dev, model, target):
    from multimodal_diffusion_amd import functional as Fn
    z, zp, npr, h0 = case(dev, target, B=2)
    eta, first = 1.0, -2
    eng = engine(model[1], target, tuple(z.shape), npr, guidance=GS, matmul="f32", solver="dpmpp_2m", eta=eta, noise_seed=ESEED)
    eng.set_prompt(zp)
    tl, tn, tp = SD.tables3(2, eng.slots, seed=21)
    eng.x0_hist.copy_(h0)
    out = eng.step_slots(z, tn, tp, t_last=tl, clip_first=first)
    sl = eng.slot_len
    hm = h0.clone()
    comp = Fn.dpmpp_2m_sde_step_slots(z, _eps_latent(eng, target, z), hm, tl, tn, tp, ABAR, sl, eta,
                                      Fn.slot_noise(ESEED, tn, tuple(z.shape), sl, first=first))
    assert torch.isfinite(out).all() and torch.isfinite(eng.x0_hist).all()
    assert torch.equal(out, comp), float((out - comp).abs().max())
    assert torch.equal(eng.x0_hist, hm)
    hold = (SR.per_position(tn, z.shape[2], sl, z) == SR.per_position(tp, z.shape[2], sl, z)).expand_as(z).to(dev)
    assert hold.any() and torch.equal(out[hold], z[hold]) and torch.equal(eng.x0_hist[hold], h0[hold])


# ------------------------------------------------------------------------------------------------- 6. fifo_denoise
def _setup(dev, mods, target, solver, eta, B=2, seed=ESEED):
    """the queue of test_gpu_fifo.py: S = 2, B samples, either target, on an engine of the given solver, eta and noise_seed"""
    g = torch.Generator().manual_seed(17)
    kw = dict(guidance=GS, solver=solver, eta=eta, **({} if seed is None else {"noise_seed": seed}))
    if target == "video":
        return engine(mods, "video", (B, 8, 4, 16, 16), 10, **kw), torch.randn(8, 150, generator=g).to(dev), 20
    return engine(mods, "audio", (B, 8, 8), 8, **kw), torch.randn(8, 14, 8, 8, generator=g).to(dev), 2


def _loop(eng, canvas_p, hop, sched, K, seed):
    """fifo_denoise restated from its parts: the plan's tables, step_slots keyed by the clip slot the queue's head holds, the torch
    shift of z (and of engine.x0_hist), set_prompt"""
    from multimodal_diffusion_amd import functional as Fn, schedule_utils as su
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_len, fifo_prompt_windows
    B, S, sl = eng.embed.B, eng.slots, eng.slot_len
    rn, rp, sn, sp = su.fifo_plan(sched, S)
    dpm = eng.solver == "dpmpp_2m"
    rl, last = su.fifo_plan_last(sched, S) if dpm else (None, None)
    n = B * S
    Lp = fifo_prompt_len(eng, canvas_p)
    z = Fn.canvas_noise(seed, torch.full((B,), int(sched[0])), eng.latent_shape, eng.latent_shape[2])
    eng.set_prompt(fifo_prompt_windows(canvas_p, 0, B, S, hop, Lp))
    for r in range(n - 1):
        z = eng.step_slots(z, rn[r], rp[r], t_last=rl[r] if dpm else None, clip_first=0)
    done = []
    for m in range(K):
        eng.set_prompt(fifo_prompt_windows(canvas_p, m, B, S, hop, Lp))
        z = eng.step_slots(z, sn, sp, t_last=last, clip_first=m)
        one_slot = (1, z.shape[1], sl) + tuple(z.shape[3:])
        tail = Fn.canvas_noise(seed, torch.tensor([int(sched[0])]), one_slot, sl, window_offset=n + m)[0]
        z, popped = SR.shift(z, tail, sl)
        if dpm:
            eng.x0_hist.copy_(SR.shift(eng.x0_hist, torch.zeros_like(tail), sl)[0])
        done.append(popped)
    return torch.cat(done, 1)


@pytest.mark.parametrize("solver,eta", SOLVERS)
@pytest.mark.parametrize("target", ["video", "audio"])
def test_stochastic_fifo_denoise_equals_the_loop_of_its_parts(dev, model, target, solver, eta):
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop = _setup(dev, model[1], target, solver, eta)
    out3 = A.fifo_denoise(eng, canvas_p, hop, SCHED4, 3, SEED)
    ref3 = _loop(eng, canvas_p, hop, SCHED4, 3, SEED)
    sl = eng.slot_len
    assert out3.shape == (8, 3 * sl) + tuple(eng.latent_shape[3:]) and torch.isfinite(out3).all() and float(out3.std()) > 0
    assert torch.equal(out3, ref3), float((out3 - ref3).abs().max())
    # the same seeds reproduce the clip, and a longer clip leaves the slots already out unchanged
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, SCHED4, 3, SEED), out3)
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, SCHED4, 5, SEED)[:, :3 * sl], out3)
    # another engine seed gives other step noise; the eta == 0 engine another clip again; equal seeds for start and steps are safe
    other, _, _ = _setup(dev, model[1], target, solver, eta, seed=ESEED + 1)
    assert not torch.equal(A.fifo_denoise(other, canvas_p, hop, SCHED4, 3, SEED), out3)
    det, _, _ = _setup(dev, model[1], target, solver, 0.0, seed=None)
    assert not torch.equal(A.fifo_denoise(det, canvas_p, hop, SCHED4, 3, SEED), out3)
    same = A.fifo_denoise(eng, canvas_p, hop, SCHED4, 3, ESEED)
    assert torch.isfinite(same).all() and torch.equal(same, _loop(eng, canvas_p, hop, SCHED4, 3, ESEED))


@pytest.mark.parametrize("n_slots", [4, 5])
@pytest.mark.parametrize("solver,eta", SOLVERS)
@pytest.mark.parametrize("target", ["video", "audio"])
def test_stochastic_fifo_denoise_graph_equals_eager(dev, model, target, solver, eta, n_slots):
    """n = 4: the ramp is one eager step and one replayed pair; n_slots 4: eager + pair + leftover, 5: eager + two pairs.  The captured
    steps hold the seed, first and stride by value and follow the clip slot off the cursor m."""
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop = _setup(dev, model[1], target, solver, eta)
    eager = A.fifo_denoise(eng, canvas_p, hop, SCHED4, n_slots, SEED, graph=False)
    h_e = None if eng.x0_hist is None else eng.x0_hist.clone()
    replayed = A.fifo_denoise(eng, canvas_p, hop, SCHED4, n_slots, SEED, graph=True)
    assert not torch.cuda.is_current_stream_capturing()
    assert replayed.shape == eager.shape and torch.isfinite(replayed).all() and float(replayed.std()) > 0
    assert torch.equal(replayed, eager), float((replayed - eager).abs().max())
    if solver == "dpmpp_2m":
        assert torch.equal(eng.x0_hist, h_e)


def _lookahead_loop(eng, canvas_p, hop, sched, K, ctx, seed):
    """fifo_denoise(lookahead=ctx) restated from its parts (the loop of _lookahead_ref.py), every step keyed by the clip slot window 0
    starts at, m - ctx, the windows h = S - ctx clip slots apart"""
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_len
    B, S, sl, shape = eng.embed.B, eng.slots, eng.slot_len, eng.latent_shape
    h = S - ctx
    n = B * h
    s = sched.tolist()
    Lp = fifo_prompt_len(eng, canvas_p)
    rn, rp, rl, sn, sp, slast = LR.plan(s, S, ctx, "noise")
    dpm = eng.solver == "dpmpp_2m"

    def noise(p0, n_pos):      # the seeded normals at s_0 of canvas positions p0 .. p0 + n_pos - 1: one window at hop 1
        return Fn.canvas_noise(seed, torch.tensor([s[0]]), (1, shape[1], n_pos) + tuple(shape[3:]), 1, window_offset=p0)[0]

    head, act = noise(2 ** 32 - ctx * sl, ctx * sl), noise(0, n * sl)
    old = [head[:, q * sl:(q + 1) * sl] for q in range(ctx)] + [act[:, a * sl:(a + 1) * sl] for a in range(n)]
    z = LR.windows(old, B, S, ctx)
    eng.set_prompt(LR.prompt_windows(canvas_p, -ctx, B, h, hop, Lp))
    for r in range(n - 1):
        z = eng.step_slots(z, rn[r], rp[r], t_last=rl[r] if dpm else None, clip_first=-ctx, clip_stride=h)
        if dpm:
            eng.x0_hist.copy_(LR.lookahead_hist(eng.x0_hist, ctx, 0, sl))
        z, _ = LR.lookahead(z, ctx, 0, sl)
    done = []
    for m in range(K):
        eng.set_prompt(LR.prompt_windows(canvas_p, m - ctx, B, h, hop, Lp))
        row = min(m, ctx)
        z = eng.step_slots(z, sn[row], sp[row], t_last=slast[row] if dpm else None, clip_first=m - ctx, clip_stride=h)
        if dpm:
            eng.x0_hist.copy_(LR.lookahead_hist(eng.x0_hist, ctx, 1, sl))
        z, popped = LR.lookahead(z, ctx, 1, sl, noise((n + m) * sl, sl))
        done.append(popped)
    return torch.cat(done, 1)


@pytest.mark.parametrize("solver,eta", SOLVERS)
@pytest.mark.parametrize("target", ["video", "audio"])
def test_stochastic_lookahead_denoise_equals_its_loop(dev, model, target, solver, eta):
    """S = 2, ctx = 1: four windows one slot apart carry the four steps of the schedule"""
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop = _setup(dev, model[1], target, solver, eta, B=4)
    out = A.fifo_denoise(eng, canvas_p, hop, SCHED4, 3, SEED, lookahead=1)
    ref = _lookahead_loop(eng, canvas_p, hop, SCHED4, 3, 1, SEED)
    assert out.shape == (8, 3 * eng.slot_len) + tuple(eng.latent_shape[3:]) and torch.isfinite(out).all() and float(out.std()) > 0
    assert torch.equal(out, ref), float((out - ref).abs().max())
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, SCHED4, 3, SEED, lookahead=1), out)
    other, _, _ = _setup(dev, model[1], target, solver, eta, B=4, seed=ESEED + 1)
    assert not torch.equal(A.fifo_denoise(other, canvas_p, hop, SCHED4, 3, SEED, lookahead=1), out)
    det, _, _ = _setup(dev, model[1], target, solver, 0.0, B=4, seed=None)
    assert not torch.equal(A.fifo_denoise(det, canvas_p, hop, SCHED4, 3, SEED, lookahead=1), out)


# ------------------------------------------------------------------------------------------------- 7. refusals
def test_stochastic_step_slots_refusals_leave_out_untouched(dev, model):
    mods = model[1]
    z, zp, npr, known = case(dev, "video", B=2)
    tn, tp = (t.to(dev) for t in SR.tables(2, 2, seed=2))
    out = torch.full_like(z, 7.0)
    base = dict(guidance=GS, eta=0.5, noise_seed=ESEED)

    def refused(eng, match, exc=ValueError, **kw):
        eng.set_prompt(zp)
        with pytest.raises(exc, match=match):
            eng.step_slots(z, tn, tp, out=out, **dict(dict(clip_first=0), **kw))
        torch.cuda.synchronize()
        assert (out == 7.0).all()

    seeded = engine(mods, "video", tuple(z.shape), npr, **base)
    refused(seeded, "eta == 0", clip_first=None)                                       # no clip_first: the pinned refusal
    refused(engine(mods, "video", tuple(z.shape), npr, guidance=GS, eta=0.5), "noise_seed")          # clip_first on an unseeded engine
    refused(engine(mods, "video", tuple(z.shape), npr, guidance=GS, eta=0.5), "eta == 0", clip_first=None)
    for bad in (0, -1, 2.0, True, 2 ** 31):
        refused(seeded, "clip_stride", clip_stride=bad)
    for bad in (1.5, True, 2 ** 32, -2 ** 32):
        refused(seeded, "clip_first", clip_first=bad)
    for bad in (torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int64, device=dev),
                torch.zeros(2, dtype=torch.int32, device=dev), 3):
        refused(seeded, "cursor", clip_cursor=bad)
    refused(seeded, "ddim", t_last=tn)                                                 # t_last on a ddim engine
    refused(engine(mods, "video", tuple(z.shape), npr, solver="dpmpp_2m", **dict(base, eta=1.0)), "t_last")
    eng = engine(mods, "video", tuple(z.shape), npr, **base)
    eng.set_known(known)
    refused(eng, "latent guide")
    refused(engine(mods, "video", tuple(z.shape), npr, **dict(base, guidance=[2.0, 3.0])), "CFG control")
    refused(engine(mods, "video", tuple(z.shape), npr, guidance_rescale=0.5, **base), "CFG control")
    eng = engine(mods, "video", tuple(z.shape), npr, **base)
    eng.set_apg(norm_threshold=1.0)
    refused(eng, "projected guidance")
    eng = engine(mods, "video", tuple(z.shape), npr, noise_keying="canvas", canvas_hop=2, **base)
    eng.set_window_consensus(2)
    refused(eng, "window consensus")
    # and the seeded engine steps once nothing is in the way
    assert torch.isfinite(seeded.step_slots(z, tn, tp, clip_first=0, clip_stride=2, clip_cursor=cur(dev, 0))).all()


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_clip_first_at_eta_0_changes_nothing(dev, model, solver):
    from multimodal_diffusion_amd import _lib as L
    z, zp, npr, h0 = case(dev, "video", B=2)
    eng = engine(model[1], "video", tuple(z.shape), npr, guidance=GS, solver=solver, noise_seed=ESEED)
    eng.set_prompt(zp)
    tl, tn, tp = SD.tables3(2, 2, seed=2)
    tl = tl if solver == "dpmpp_2m" else None

    def run(**kw):
        if eng.x0_hist is not None:
            eng.x0_hist.copy_(h0)
        L.prof_enable(True)
        try:
            out = eng.step_slots(z, tn, tp, t_last=tl, **kw)
            torch.cuda.synchronize()
        finally:
            L.prof_enable(False)
        launches = {k: v[0] for k, v in L.prof_report().items() if v[0]}
        return out, None if eng.x0_hist is None else eng.x0_hist.clone(), launches

    ref, href, n_ref = run()
    out, hist, n_out = run(clip_first=5, clip_stride=3, clip_cursor=cur(dev, 2))
    assert torch.equal(out, ref) and n_out == n_ref                 # the same bits from the same launches
    assert href is None or torch.equal(hist, href)


def test_fifo_denoise_refuses_an_unseeded_eta_engine_in_every_driver(dev, model):
    import multimodal_diffusion_amd as A
    seen = []
    for B, kw in ((2, dict(graph=False)), (2, dict(graph=True)), (4, dict(lookahead=1))):
        eng, canvas_p, hop = _setup(dev, model[1], "video", "ddim", 0.5, B=B, seed=None)
        with pytest.raises(ValueError, match="eta == 0") as e:
            A.fifo_denoise(eng, canvas_p, hop, SCHED4, 2, SEED, **kw)
        assert not torch.cuda.is_current_stream_capturing()
        seen.append(str(e.value))
    assert seen[0] == seen[1] == seen[2]
