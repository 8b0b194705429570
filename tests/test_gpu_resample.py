"""RePaint resampling on the MI355X (include/avdiff_hip.h, "renoise"): avd_renoise_f32 / avd_renoise_canvas_f32 against the float64
reference (per-sample timesteps, the identity case, the tail lanes), in place, under a guide (held region on its forward path bit
for bit), the keys (sample / window offsets, visit, the stream's own tag), the canvas keying (windows agree, values of the per-sample
stream at [p, e']); DenoiseEngine.run on a schedule with up-jumps against the hand-driven chain, graph against eager, the schedule
cursor's t_last after a jump, the held region of a resampled run; stream_generate / sample_one_direction with ``resample``; and the
refusals."""
import ctypes as C
from functools import partial

import numpy as np
import pytest
import torch

import _canvas_noise_ref as CN
import _consensus_ref as W
import _guide_ref as G
import _noise_ref as NR
import _renoise_ref as RR
from _kit import (ABAR, STREAM_HALF_SECOND, Recorder, audio_case, audio_prompt, components, dev, engine, matmul_f32, model,  # noqa: F401  (dev / model are fixtures)
                  pipeline, soft_mask, ts, video_case)
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu
SEED, GSEED = 0xDEADBEEF12345678, 0x1234567ABCDEF01          # both key words non-zero
TOL = 2e-5                                                   # the bound test_gpu_latent_guide.py holds q to
_engine = partial(engine, guidance=3.0)


def _err(got, ref):
    return float(np.abs(got.cpu().double().numpy() - ref).max())


def _hard_mask(shape, seed=5):
    return (torch.rand(shape, generator=torch.Generator().manual_seed(seed)) < 0.5).float()


def _latents(dev, kind):
    """(z, known) of the kit's smallest cases, and a [2, 3, 37] latent whose per_sample = 111 ends in a tail lane of three"""
    if kind == "video":
        z, _, _, known = video_case(dev, B=2, W=32, known=True)
    elif kind == "audio":
        z, _, _, known = audio_case(dev, B=2, L=40, known=True)
    else:
        g = torch.Generator().manual_seed(2)
        z, known = torch.randn(2, 3, 37, generator=g).to(dev), torch.randn(2, 3, 37, generator=g).to(dev)
    return z, known


def _unaligned(x, copy=False):
    """a contiguous view of x's shape that starts one float into a larger buffer"""
    v = torch.empty(x.numel() + 1, device=x.device)[1:].view(x.shape)
    assert v.data_ptr() % 16 != 0
    return v.copy_(x) if copy else v


# per-sample timesteps that differ across the batch: a jump from the clean end (t_from = -1), an identity sample (t_to <= t_from)
T_PAIRS = [([-1, 500], [300, 200]), ([100, 700], [600, 999]), ([250, 250], [250, 750])]


# ------------------------------------------------------------------------------------------------- the per-sample entry
@pytest.mark.parametrize("kind", ["video", "audio", "tail"])
def test_kernel_vs_reference(dev, kind):
    from multimodal_diffusion_amd import functional as Fn
    z, known = _latents(dev, kind)
    shape = tuple(z.shape)
    md = soft_mask(shape, seed=6).to(dev)                     # the descriptor holds raw pointers: known and md stay alive
    guide_soft = Fn.latent_guide_desc(known, md, GSEED, 4)
    for visit, (tf, tt) in enumerate(T_PAIRS):
        out = Fn.renoise(z, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit + 7, sample_offset=4)
        assert out.shape == z.shape and out.dtype == torch.float32
        ref = RR.renoise_f64(z.cpu().numpy(), tf, tt, ABAR.numpy(), SEED, visit + 7, sample_offset=4)
        err = _err(out, ref)
        print(f"renoise {kind} {tf}->{tt}: max err {err:.3e} (bound {TOL:.0e})")
        assert err <= TOL
        same = RR.coef(ABAR.numpy(), tf, tt)[0]
        assert same.any() or visit == 1
        for b in np.nonzero(same)[0]:
            assert torch.equal(out[b], z[b])                  # the identity case: z itself, bit for bit
        for b in np.nonzero(~same)[0]:
            assert not torch.equal(out[b], z[b])
        # in place = out of place, and an explicit out
        zi = z.clone()
        assert Fn.renoise(zi, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit + 7, sample_offset=4, out=zi) is zi and torch.equal(zi, out)
        # an out one float into a larger buffer takes the guarded lanes: the same bits
        ou = _unaligned(z)
        assert torch.equal(Fn.renoise(z, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit + 7, sample_offset=4, out=ou), out)
        # a soft mask: the blend of the contract
        got = Fn.renoise(z, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit + 7, sample_offset=4, guide=guide_soft)
        m = md.cpu().numpy()
        ref_g = RR.renoise_f64(z.cpu().numpy(), tf, tt, ABAR.numpy(), SEED, visit + 7, sample_offset=4, known=known.cpu().numpy(),
                               mask=m, guide_seed=GSEED)
        err = _err(got, ref_g)
        print(f"renoise {kind} {tf}->{tt} under a soft mask: max err {err:.3e} (bound {TOL:.0e})")
        assert err <= TOL
        q = Fn.latent_guide(known, ts(tt, dev), ABAR, seed=GSEED, sample_offset=4)
        assert torch.equal(got[md == 1], q[md == 1]) and torch.equal(got[md == 0], out[md == 0])
        gi = z.clone()
        Fn.renoise(gi, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit + 7, sample_offset=4, guide=guide_soft, out=gi)
        assert torch.equal(gi, got)


@pytest.mark.parametrize("kind", ["video", "audio", "tail"])
def test_guide_holds_the_forward_path(dev, kind):
    """mask 1: avd_latent_guide_f32's pure forward noising at t_to, bit for bit; mask 0: the unguided renoise, bit for bit"""
    from multimodal_diffusion_amd import functional as Fn
    z, known = _latents(dev, kind)
    shape = tuple(z.shape)
    for mask in (_hard_mask(shape), _hard_mask(shape[1:])):                      # per sample, and one shared by the batch
        md = mask.to(dev)
        g = Fn.latent_guide_desc(known, md, GSEED, 0)
        for tf, tt in T_PAIRS:
            got = Fn.renoise(z, ts(tf, dev), ts(tt, dev), ABAR, SEED, 3, guide=g)
            q = Fn.latent_guide(known, ts(tt, dev), ABAR, seed=GSEED)
            free = Fn.renoise(z, ts(tf, dev), ts(tt, dev), ABAR, SEED, 3)
            keep = md.expand(shape) == 1
            assert keep.any() and (~keep).any()
            assert torch.equal(got[keep], q[keep]) and torch.equal(got[~keep], free[~keep])
    # no mask reads as 1 everywhere
    g1 = Fn.latent_guide_desc(known, None, GSEED, 0)
    assert torch.equal(Fn.renoise(z, ts([100, 100], dev), ts([600, 600], dev), ABAR, SEED, 3, guide=g1),
                       Fn.latent_guide(known, ts([600, 600], dev), ABAR, seed=GSEED))


def test_keys(dev):
    from multimodal_diffusion_amd import functional as Fn
    z4, _, _, k4 = video_case(dev, B=4, W=32, known=True)
    tf, tt = ts([-1, 100, 300, 500], dev), ts([400, 600, 200, 900], dev)
    m4 = _hard_mask(z4.shape[1:]).to(dev)                     # shared by the batch; alive while a descriptor points at it
    for guided in (False, True):
        def call(sl, off, visit=9):
            g = Fn.latent_guide_desc(k4[sl], m4, GSEED, off) if guided else None       # k4[sl]: a view of k4
            return Fn.renoise(z4[sl].contiguous(), tf[sl], tt[sl], ABAR, SEED, visit, sample_offset=off, guide=g)
        whole = call(slice(0, 4), 0)
        assert torch.equal(whole, torch.cat([call(slice(0, 2), 0), call(slice(2, 4), 2)]))       # B = 4 is two B = 2 calls
        assert torch.equal(call(slice(0, 4), 0), whole)                                         # the same visit: the same bits
        other = call(slice(0, 4), 0, visit=10)
        assert not torch.equal(other, whole) and torch.equal(other[2], whole[2])                 # fresh normals; the identity sample
        assert not torch.equal(call(slice(0, 4), 1), whole)
    # the stream's own tag: with z = 0 the output is S n_r, which is neither S times DDIM's normals at t = visit nor the known noise
    z0 = torch.zeros_like(z4)
    visit = 9
    out = Fn.renoise(z0, ts([-1] * 4, dev), ts([999] * 4, dev), ABAR, SEED, visit)
    rho = ABAR[999].item()
    assert 0 < rho < 1e-3                                                                        # a small rho: S is close to 1
    S = torch.sqrt(torch.clamp(1.0 - ABAR[999], min=0.0)).to(dev)
    ddim = S * Fn.gaussian_noise(SEED, 0, ts([visit] * 4, dev), tuple(z4.shape))
    assert not torch.equal(out, ddim) and float((out - ddim).abs().max()) > 0.5
    kn = Fn.latent_guide(z0, ts([999] * 4, dev), ABAR, seed=SEED)                                # S n_k of the same seed
    assert not torch.equal(out, kn) and float((out - kn).abs().max()) > 0.5
    ref = RR.renoise_f64(z0.cpu().numpy(), [-1] * 4, [999] * 4, ABAR.numpy(), SEED, visit)       # and it is the contract's stream
    assert _err(out, ref) <= TOL
    assert abs(float(out.std()) - 1.0) < 0.02 and abs(float(out.mean())) < 0.02


# ------------------------------------------------------------------------------------------------- the canvas entry
CANVAS_CASES = [
    ("video inner 16", (3, 8, 4, 4, 4), 2, 0),                # the vector lanes
    ("video inner 16, offset", (3, 8, 4, 4, 4), 2, 5),
    ("video inner 6", (3, 3, 4, 2, 3), 2, 1),                 # inner % 4 != 0: one generator call per element
    ("audio inner 1", (3, 8, 40), 4, 2),                      # the scalar lanes
    ("audio L 4", (3, 8, 4), 2, 0),
]


@pytest.mark.parametrize("name,shape,hop,off", CANVAS_CASES, ids=[c[0] for c in CANVAS_CASES])
def test_canvas_entry(dev, name, shape, hop, off):
    from multimodal_diffusion_amd import functional as Fn
    N = shape[0]
    outer, L_, inner = W.dims(shape)
    P = (N - 1) * hop + L_
    g = torch.Generator().manual_seed(5)
    canvas = torch.randn((outer, P) + shape[3:], generator=g).numpy()
    known_c = torch.randn((outer, P) + shape[3:], generator=g).numpy()
    mask_c = _hard_mask((outer, P) + shape[3:], seed=8).numpy()
    z = torch.from_numpy(W.windows_from_canvas(canvas, L_, hop)).to(dev)
    known = torch.from_numpy(W.windows_from_canvas(known_c, L_, hop)).to(dev)
    mask = torch.from_numpy(W.windows_from_canvas(mask_c, L_, hop)).to(dev)
    tf, tt, visit = [249] * N, [749] * N, 4
    guide = Fn.latent_guide_desc(known, mask, GSEED, off)
    kw = dict(sample_offset=off, canvas_hop=hop)
    free = Fn.renoise(z, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit, **kw)
    held = Fn.renoise(z, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit, guide=guide, **kw)
    # the float64 reference
    for label, got, kwr in (("free", free, {}), ("guided", held, dict(known=known.cpu().numpy(), mask=mask.cpu().numpy(),
                                                                         guide_seed=GSEED))):
        ref = RR.renoise_canvas_f64(z.cpu().numpy(), tf, tt, ABAR.numpy(), SEED, visit, hop, off, **kwr)
        err = _err(got, ref)
        print(f"canvas renoise {name} ({label}): max err {err:.3e} (bound {TOL:.0e})")
        assert err <= TOL
        assert W.overlaps_agree(got.cpu().numpy(), hop)       # windows that agreed before the jump agree after it, bit for bit
    # bit for bit: the per-sample entry over the canvas positions as samples of outer*inner elements, at [p, e']
    def rows(c):
        return torch.from_numpy(np.ascontiguousarray(np.moveaxis(c.reshape(outer, P, inner), 1, 0).reshape(P, outer * inner))).to(dev)
    known_r, mask_r = rows(known_c), rows(mask_c)            # alive while g_rows points at them
    g_rows = Fn.latent_guide_desc(known_r, mask_r, GSEED, off * hop)
    for got, gr in ((free, None), (held, g_rows)):
        per = Fn.renoise(rows(canvas), ts([249] * P, dev), ts([749] * P, dev), ABAR, SEED, visit, sample_offset=off * hop, guide=gr)
        assert np.array_equal(got.cpu().numpy(), CN.gather_windows(per.cpu().numpy(), shape, hop))
    # the guide: q(t_to) of the canvas-keyed guide where the mask is 1, the free renoise where it is 0
    q = Fn.latent_guide(known, ts(tt, dev), ABAR, seed=GSEED, canvas_hop=hop, window_offset=off)
    assert torch.equal(held[mask == 1], q[mask == 1]) and torch.equal(held[mask == 0], free[mask == 0])
    # in place, an unaligned z (one generator call per element), window offsets, the visit, per-window timesteps with an identity one
    zi = z.clone()
    Fn.renoise(zi, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit, guide=guide, out=zi, **kw)
    assert torch.equal(zi, held)
    buf = torch.empty(z.numel() + 1, device=dev)
    zu = buf[1:].view(shape)
    zu.copy_(z)
    assert zu.data_ptr() % 16 != 0
    assert torch.equal(Fn.renoise(zu, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit, guide=guide, **kw), held)
    assert torch.equal(Fn.renoise(z, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit, guide=guide, out=_unaligned(z), **kw), held)
    parts = []
    for lo, hi in ((0, 2), (2, 3)):
        gp = Fn.latent_guide_desc(known[lo:hi], mask[lo:hi], GSEED, off + lo)                     # views of known / mask
        parts.append(Fn.renoise(z[lo:hi].contiguous(), ts(tf[lo:hi], dev), ts(tt[lo:hi], dev), ABAR, SEED, visit, sample_offset=off + lo,
                                canvas_hop=hop, guide=gp))
    assert torch.equal(torch.cat(parts), held)
    assert not torch.equal(Fn.renoise(z, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit + 1, **kw), free)
    mixed_f, mixed_t = [-1, 500, 100], [300, 200, 600]
    mixed = Fn.renoise(z, ts(mixed_f, dev), ts(mixed_t, dev), ABAR, SEED, visit, **kw)
    assert torch.equal(mixed[1], z[1]) and not torch.equal(mixed[0], z[0])
    for zm in (z.clone(), _unaligned(z, copy=True)):          # the identity window in place, on this shape's lanes and the unaligned ones
        Fn.renoise(zm, ts(mixed_f, dev), ts(mixed_t, dev), ABAR, SEED, visit, out=zm, **kw)
        assert torch.equal(zm, mixed)
    assert _err(mixed, RR.renoise_canvas_f64(z.cpu().numpy(), mixed_f, mixed_t, ABAR.numpy(), SEED, visit, hop, off)) <= TOL
    # keyed per sample the windows part
    per_sample = Fn.renoise(z, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit, sample_offset=off)
    assert not W.overlaps_agree(per_sample.cpu().numpy(), hop)
    with pytest.raises(ValueError, match="same sample_offset"):
        Fn.renoise(z, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit, guide=Fn.latent_guide_desc(known, mask, GSEED, off + 1), **kw)


# ------------------------------------------------------------------------------------------------- one map for the keyings
@pytest.mark.parametrize("per", [1, 3, 5, 8])                 # a lone partial lane (1, 3), a full lane and a tail of one, no tail
def test_per_sample_entries_are_the_canvas_entries_at_hop_1(dev, per):
    """the batch [B, 1, 1, per] at hop 1 puts window b on canvas position off + b, element e' = i: the per-sample stream's counters"""
    from multimodal_diffusion_amd import functional as Fn
    B, off, shape = 2, 11, (2, 1, 1, 1, per)
    g = torch.Generator().manual_seed(per)
    z, known = torch.randn(shape, generator=g).to(dev), torch.randn(shape, generator=g).to(dev)
    md = torch.tensor([0.0, 1.0, 0.4, 0.75] * 4)[:B * per].view(shape).to(dev)      # both selects, and fractions from per = 3 on
    zn, kn, mn = (x.cpu().numpy().reshape(B, per) for x in (z, known, md))
    # the draw
    tn = [731, 17]
    draw = Fn.gaussian_noise(SEED, off, ts(tn, dev), shape)
    assert torch.equal(draw, Fn.canvas_noise(SEED, ts(tn, dev), shape, 1, window_offset=off))
    assert np.abs(draw.cpu().double().numpy().reshape(B, per) - NR.normals(SEED, off, tn, per)).max() < 1e-5
    # the guide: the blend, and z = None; an unaligned z takes the guarded lanes
    tau = [700, 300]
    q_ref = G.q_f64(kn, tau, ABAR.numpy(), GSEED, off)
    for zz, ref in ((z, G.blend_f64(mn, q_ref, zn)), (None, q_ref)):
        m = md if zz is not None else None
        per_sample = Fn.latent_guide(known, ts(tau, dev), ABAR, z=zz, mask=m, seed=GSEED, sample_offset=off)
        assert torch.equal(per_sample, Fn.latent_guide(known, ts(tau, dev), ABAR, z=zz, mask=m, seed=GSEED, canvas_hop=1, window_offset=off))
        assert _err(per_sample.reshape(B, per), ref) <= TOL
        if zz is not None:
            assert torch.equal(Fn.latent_guide(known, ts(tau, dev), ABAR, z=_unaligned(z, copy=True), mask=m, seed=GSEED, sample_offset=off),
                               per_sample)
    # the renoise, free and guided; sample 1 is the identity
    tf, tt, visit = [249, 500], [749, 200], 4
    guide = Fn.latent_guide_desc(known, md, GSEED, off)
    for gd, kwr in ((None, {}), (guide, dict(known=kn, mask=mn, guide_seed=GSEED))):
        per_sample = Fn.renoise(z, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit, sample_offset=off, guide=gd)
        assert torch.equal(per_sample, Fn.renoise(z, ts(tf, dev), ts(tt, dev), ABAR, SEED, visit, sample_offset=off, guide=gd, canvas_hop=1))
        assert _err(per_sample.reshape(B, per), RR.renoise_f64(zn, tf, tt, ABAR.numpy(), SEED, visit, sample_offset=off, **kwr)) <= TOL
        if gd is None:
            assert torch.equal(per_sample[1], z[1]) and not torch.equal(per_sample[0], z[0])


# ------------------------------------------------------------------------------------------------- the engine
def _chain(eng, z, sched):
    """the hand-driven form of run(): a step per down pair, a renoise (visit = the pair's index) per up pair; DPM-Solver++(2M) takes
    the first step, and every step after a jump, with t_last=None"""
    B, dev_ = z.shape[0], z.device
    s = sched.tolist()
    last = None
    for i, (a, b) in enumerate(zip(s[:-1], s[1:])):
        if b > a:
            z = eng.renoise(z, ts([a] * B, dev_), ts([b] * B, dev_), i)
            last = None
            continue
        tl = None if (eng.solver != "dpmpp_2m" or last is None) else ts([last] * B, dev_)
        z = eng.step(z, ts([a] * B, dev_), ts([b] * B, dev_), t_last=tl)
        last = a
    return z


@pytest.mark.parametrize("solver,eta", [("ddim", 0.0), ("ddim", 0.5), ("dpmpp_2m", 0.0)])
def test_run_equals_the_hand_driven_chain(dev, model, solver, eta):
    from multimodal_diffusion_amd import schedule_utils as su
    z, zp, npr, known = video_case(dev, B=2, known=True)
    sched = su.resample_schedule(R.sampling_schedule(1000, 6), 2, 2)
    assert sched.numel() == 6 + 4 + 2 + 1 and su.has_jumps(sched)
    eng = _engine(model[1], "video", tuple(z.shape), npr, eta=eta, solver=solver, noise_seed=SEED, sample_offset=3)
    eng.set_prompt(zp)
    for guided in (False, True):
        if guided:
            eng.set_known(known, soft_mask(tuple(z.shape[1:]), seed=7), guide_seed=GSEED)
        ref = _chain(eng, z, sched)
        eager = eng.run(z, sched, graph=False)
        graph = eng.run(z, sched, graph=True)
        assert torch.isfinite(ref).all() and torch.equal(eager, ref) and torch.equal(graph, eager)
        plain = eng.run(z, R.sampling_schedule(1000, 6), graph=False)
        assert not torch.equal(plain, ref)                    # the jumps are live


def test_a_climb_to_a_new_timestep_is_still_a_ddim_step(dev, model):
    """the DDIM engine has always taken any schedule: an up-pair to a timestep not passed before is no time travel and stays a step,
    on an unseeded engine too"""
    z, zp, npr = video_case(dev, B=2)
    sched = torch.tensor([990, 900, 360, 700, 650, -1])
    eng = _engine(model[1], "video", tuple(z.shape), npr)
    eng.set_prompt(zp)
    ref = z
    for a, b in zip(sched[:-1].tolist(), sched[1:].tolist()):
        ref = eng.step(ref, ts([a] * 2, dev), ts([b] * 2, dev))
    assert torch.equal(eng.run(z, sched, graph=False), ref) and torch.equal(eng.run(z, sched, graph=True), ref)


def test_sched_advance_ms_after_a_jump(dev):
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import schedule_utils as su
    dec = R.sampling_schedule(1000, 6)
    for sched in (dec, su.resample_schedule(dec, 2, 2), su.resample_schedule(dec, 1, 3)):
        s = sched.tolist()
        sd = sched.to(dev, torch.long).contiguous()
        cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        tl, tn, tp = (torch.empty(3, dtype=torch.long, device=dev) for _ in range(3))
        for i in range(len(s) - 1):
            L.check(L.lib().avd_sched_advance_ms(sd.data_ptr(), sd.numel(), cursor.data_ptr(), tl.data_ptr(), tn.data_ptr(), tp.data_ptr(),
                                                 3, L.stream_ptr(dev)))
            want = s[i - 1] if i > 0 and s[i - 1] > s[i] else -1      # on a decreasing schedule: the entry before, as always
            assert tl.tolist() == [want] * 3 and tn.tolist() == [s[i]] * 3 and tp.tolist() == [s[i + 1]] * 3
            if sched is dec:
                assert want == (s[i - 1] if i > 0 else -1)
        assert int(cursor) == len(s) - 1


@pytest.mark.parametrize("target", ["video", "audio"])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_held_region_of_a_resampled_run(dev, model, solver, target):
    from multimodal_diffusion_amd import schedule_utils as su
    z, zp, npr, known = (video_case if target == "video" else audio_case)(dev, B=2, known=True)
    shape = tuple(z.shape)
    mask = _hard_mask(shape[1:], seed=9)
    eng = _engine(model[1], target, shape, npr, solver=solver, noise_seed=SEED)
    eng.set_prompt(zp)
    eng.set_known(known, mask, guide_seed=GSEED)
    start, sk = eng.start_latent(z, R.sampling_schedule(1000, 6), 1.0)
    out = eng.run(start, su.resample_schedule(sk, 2, 2))
    keep = mask.to(dev).expand(shape) == 1
    assert torch.isfinite(out).all() and torch.equal(out[keep], known[keep]) and not torch.equal(out[~keep], known[~keep])
    assert not torch.equal(out, eng.run(start, sk))


# ------------------------------------------------------------------------------------------------- the pipelines
INIT_VIDEO = np.random.default_rng(5).integers(0, 256, size=(20, 32, 32, 3), dtype=np.uint8)          # 20 frames: 4 windows of 0.5 s


def test_stream_generate_resamples_under_consensus(dev, model):
    from multimodal_diffusion_amd import stream_infer as S
    from multimodal_diffusion_amd.sampler import canvas_frame_mask
    with matmul_f32(model[1]):                                # one kernel family whatever the batch, so that batch sizes can be compared
        vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND)
        hop, L_ = S.latent_hop(cfg, "video")
        assert (hop, L_) == (1, 2)
        kws = dict(components(model[1], vae, codec, dev), cfg=cfg, shard=False, consensus="uniform", return_latents=True,
                   init_video=INIT_VIDEO, mask=canvas_frame_mask((8, 5, 4, 4), 0, 2), noise_seed=3, **audio_prompt())
        whole = S.stream_generate(resample=(2, 2), **kws)
        lat = whole["latents"]
        assert lat.shape == (4, 8, 2, 4, 4) and np.isfinite(lat).all() and W.overlaps_agree(lat, hop)
        part = S.stream_generate(resample=(2, 2), max_windows_per_batch=2, **kws)               # lock-step engines
        assert np.array_equal(part["latents"], lat)
        plain = S.stream_generate(**kws)
        assert not np.array_equal(plain["latents"], lat)
        # the held canvas positions come out the same either way: the known canvas
        canvas, canvas_p = (S.canvas_from_windows(torch.from_numpy(x), hop).numpy() for x in (lat, plain["latents"]))
        assert np.array_equal(canvas[:, :2], canvas_p[:, :2]) and not np.array_equal(canvas[:, 2:], canvas_p[:, 2:])
        # the config's form is the argument's
        by_cfg = S.stream_generate(**dict(kws, cfg=dict(cfg, sampling=dict(cfg["sampling"], resample={"jump": 2, "resamples": 2}))))
        assert np.array_equal(by_cfg["latents"], lat)


def test_sample_one_direction_resamples(dev, model):
    import multimodal_diffusion_amd as A
    vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=1.0, sampler_steps=5)
    wav = (0.1 * torch.randn(16000, generator=torch.Generator().manual_seed(9))).numpy()
    clip = np.random.default_rng(3).integers(0, 256, size=(16, 32, 32, 3), dtype=np.uint8)
    rec = Recorder(vae)
    noise = torch.randn(1, 8, 4, 4, 4, generator=torch.Generator().manual_seed(4))
    m = A.frame_mask((8, 4, 4, 4), 0, 2)
    kw = dict(components(model[1], rec, codec, dev), cfg=cfg, prompt_modality="audio", prompt_video=None, prompt_audio=wav,
              init_noise=noise, init_video=clip, mask=m, noise_seed=3)
    base = A.sample_one_direction(**kw)
    z_base = rec.last
    once = A.sample_one_direction(resample=(2, 1), **kw)      # resamples == 1: today's run, bit for bit
    assert torch.equal(rec.last, z_base) and np.array_equal(once["video"], base["video"])
    twice = A.sample_one_direction(resample=(2, 2), **kw)
    z_twice = rec.last
    keep = m.to(dev).bool().unsqueeze(0)
    assert not torch.equal(z_twice, z_base) and torch.equal(z_twice[keep], z_base[keep])
    assert twice["video"].shape == clip.shape


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals(dev, model):
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd import schedule_utils as su
    z, zp, npr, known = video_case(dev, B=3, W=16, known=True)
    shape = tuple(z.shape)
    sched = su.resample_schedule(R.sampling_schedule(1000, 4), 2, 2)
    tn, tp = ts([249] * 3, dev), ts([749] * 3, dev)
    # no noise_seed: the renoise has no key, also at eta == 0
    for solver in ("ddim", "dpmpp_2m"):
        unseeded = _engine(model[1], "video", shape, npr, solver=solver)
        unseeded.set_prompt(zp)
        with pytest.raises(ValueError, match="noise_seed"):
            unseeded.run(z, sched)
        with pytest.raises(ValueError, match="noise_seed"):
            unseeded.renoise(z, tn, tp, 0)
    # consensus with per-sample keying
    per = _engine(model[1], "video", shape, npr, noise_seed=SEED)
    per.set_prompt(zp)
    per.set_window_consensus(2)
    with pytest.raises(ValueError, match="consensus.*noise_keying='canvas'"):
        per.run(z, sched)
    with pytest.raises(ValueError, match="consensus"):
        per.renoise(z, tn, tp, 0)
    per.set_known(known, None, guide_seed=GSEED)              # a per-sample guide does not change that
    with pytest.raises(ValueError, match="consensus"):
        per.run(z, sched)
    per.set_known(known, None, guide_seed=GSEED, keying="canvas", hop=2)      # a canvas-keyed guide at the consensus hop does
    assert torch.isfinite(per.run(z, sched)).all()
    canvas = _engine(model[1], "video", shape, npr, noise_seed=SEED, noise_keying="canvas", canvas_hop=2)
    canvas.set_prompt(zp)
    canvas.set_window_consensus(2)
    zc = torch.from_numpy(W.windows_from_canvas(torch.randn(8, 8, 16, 16, generator=torch.Generator().manual_seed(3)).numpy(), 4, 2)).to(dev)
    assert W.overlaps_agree(canvas.run(zc, sched).cpu().numpy(), 2)
    canvas.set_known(known, None, guide_seed=GSEED)           # a per-sample guide under a canvas-keyed renoise
    with pytest.raises(ValueError, match="keyed per sample"):
        canvas.run(zc, sched)
    # the multistep solver: strictly decreasing runs, joined by jumps back to a timestep already passed
    dpm = _engine(model[1], "video", shape, npr, solver="dpmpp_2m", noise_seed=SEED)
    dpm.set_prompt(zp)
    for bad in ([999, 500, 500, -1], [999, 200, 500, -1], [999, 500, 999, 999, -1]):
        with pytest.raises(ValueError, match="decreasing"):
            dpm.run(z, torch.tensor(bad))
    ddim = _engine(model[1], "video", shape, npr, noise_seed=SEED)
    ddim.set_prompt(zp)
    with pytest.raises(ValueError, match="both 999"):
        ddim.run(z, torch.tensor([999, 500, 999, 999, -1]))
    # functional.renoise
    for bad in (-1, 2 ** 32, 1.5):
        with pytest.raises(ValueError, match="visit"):
            Fn.renoise(z, tn, tp, ABAR, SEED, bad)
    with pytest.raises(ValueError, match="entries"):
        Fn.renoise(z, tn[:2], tp, ABAR, SEED, 0)
    with pytest.raises(ValueError, match="out must"):
        Fn.renoise(z, tn, tp, ABAR, SEED, 0, out=torch.empty(3, 8, 4, 16, 8, device=dev))
    with pytest.raises(ValueError, match="2\\*\\*32"):
        Fn.renoise(z, tn, tp, ABAR, SEED, 0, sample_offset=2 ** 32 - 2)
    with pytest.raises(ValueError, match="2\\*\\*32"):
        Fn.renoise(z, tn, tp, ABAR, SEED, 0, sample_offset=2 ** 32 - 2, canvas_hop=2)
    buf = torch.empty(z.numel() + 4, device=dev)
    with pytest.raises(ValueError, match="overlap"):          # out neither z nor apart from it: the C entry refuses
        key = Fn.noise_key(SEED, 0)
        L.check(L.lib().avd_renoise_f32(C.byref(key), 0, None, tn.data_ptr(), tp.data_ptr(), ABAR.to(dev).data_ptr(), 1000,
                                        buf.data_ptr(), buf.data_ptr() + 16, 3, z.numel() // 3, L.stream_ptr(dev)))
    # the pipelines: resample without a mask, and without noise_seed
    vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=1.0, sampler_steps=5)
    wav = (0.1 * torch.randn(16000, generator=torch.Generator().manual_seed(9))).numpy()
    clip = np.zeros((16, 32, 32, 3), dtype=np.uint8)
    kw = dict(components(model[1], vae, codec, dev), cfg=cfg, prompt_modality="audio", prompt_video=None, prompt_audio=wav)
    with pytest.raises(ValueError, match="mask"):
        A.sample_one_direction(resample=(2, 2), noise_seed=3, init_video=clip, **kw)
    with pytest.raises(ValueError, match="noise_seed"):
        A.sample_one_direction(resample=(2, 2), init_video=clip, mask=A.frame_mask((8, 4, 4, 4), 0, 2), **kw)
