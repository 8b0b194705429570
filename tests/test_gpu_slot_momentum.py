"""Slot APG momentum on the MI355X (include/avdiff_hip.h, "slot APG momentum"): the fused slot updates with a momentum buffer over
chained calls against the numpy mirror; S = 1 against the per-sample APG step with the same momentum; held slots, the uncovered audio
tail and a slot's bits wherever it sits; beta = 0 and the zero buffer against today's slot APG; ``avd_fifo_carry_f32`` against the
torch statement; ``fifo_denoise(apg_momentum=)`` eager, replayed, lookahead and restated by hand; the C entries' refusals.  Reduced
model, the smallest shapes that reach every path; the helpers and the bounds are those of test_gpu_slot_cfg.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import _apg_ref as AR
import _cfg_ref as CR
import _lookahead_ref as LR
import _slot_ref as SR
import test_gpu_slot_cfg as TG
from _kit import ABAR, dev, engine, model  # noqa: F401  (dev, model are fixtures)
from _tune import tuned
from test_slot_momentum_cpu import CARRY_CASES

pytestmark = pytest.mark.gpu

GS, T, APG, GTAB = TG.GS, TG.T, TG.APG, TG.GTAB
BETA = -0.5
# video: four whole chunks on the 4-token rows form (and, with cfg_rows = 0, the gather form); a ragged second chunk, gather form; S = 1
# with a single ragged chunk.  audio: two slots of 24 elements and two uncovered frames; S = 1 (F == len)
V_ROWS, V_RAGGED, V_ONE = ((2, 8, 4, 16, 16), (2, 4, 4)), ((2, 12, 4, 8, 8), (2, 4, 4)), ((1, 5, 2, 8, 8), (2, 4, 4))
A_TAIL, A_ONE = ((2, 6, 10), (4, 4)), ((2, 6, 4), (4, 4))
GEOMS = [V_ROWS, V_RAGGED, V_ONE, A_TAIL, A_ONE]
UPDATES = [(0.0, False), (0.5, False), (0.0, True)]          # DDIM, seeded DDIM, DPM-Solver++(2M)
SENTINEL = 1234.5


def _ctl(dev, ge, B=None, beta=BETA, M=None):
    """TG.Ctl in its APG mode with the control rebuilt as an avd_slot_cfg_momentum: the same seven fields, apg = AVD_SLOT_APG_MOMENTUM,
    then beta and the buffer"""
    L, _ = TG._lib()
    c = TG.Ctl(dev, "apg", ge.B if B is None else B, ge.S, ge.per_slot)
    c.c = L.SlotCfgMomentum(L.ptr(c.g), None, L.SLOT_APG_MOMENTUM, APG[0], APG[1], L.ptr(c.stats), c.nb, beta, None if M is None else M.data_ptr())
    return c


def _tables(ge, B, seed):
    if B * ge.S >= 2:
        return SR.tables(B, ge.S, seed=ge.S * 8 + B + seed)
    return torch.tensor([[499]]), torch.tensor([[449]])      # one slot: it steps


def _inputs(ge, dev, seed=0, B=None):
    """(z, eps2 [2B, Nt, D], t_last, t_now, t_prev, M0): random cond, a null correlated with it (S_dc does not cancel), mixed pairs with
    holds where the batch has two slots or more, a random non-zero momentum with the sentinel on an uncovered audio tail"""
    B = ge.B if B is None else B
    shape = (B,) + ge.shape[1:]
    g = torch.Generator().manual_seed(sum(ge.shape) + seed)
    z = torch.randn(shape, generator=g)
    c = torch.randn(B, ge.Nt, ge.D, generator=g)
    u = 0.2 * c + 0.5 * torch.randn(B, ge.Nt, ge.D, generator=g)
    M0 = torch.randn(shape, generator=g)
    if not ge.video:
        M0[:, :, ge.S * ge.slot_len:] = SENTINEL
    tn, tp = _tables(ge, B, seed)
    sc = SR.SCHED
    tl = torch.tensor([[sc[sc.index(int(a)) - 1] if sc.index(int(a)) > 0 else -1 for a in row] for row in tn])
    return z.to(dev), torch.cat([c, u]).to(dev), tl.to(dev), tn.to(dev), tp.to(dev), M0.to(dev)


def _rows(ge, lat):
    """a latent-layout tensor [B, C, L, ...] -> one slot per row [B * S, per_slot] in the slot's own latent order"""
    B, sl = lat.shape[0], ge.slot_len
    v = lat[:, :, :ge.S * sl].reshape(B, lat.shape[1], ge.S, -1)
    return v.permute(0, 2, 1, 3).reshape(B * ge.S, -1)


def _lat(ge, rows, like):
    """the inverse of _rows, into a copy of ``like`` (what rows do not cover, an uncovered audio tail, stays)"""
    B, sl = like.shape[0], ge.slot_len
    out = like.clone()
    v = rows.reshape(B, ge.S, like.shape[1], -1).permute(0, 2, 1, 3)
    out[:, :, :ge.S * sl] = v.reshape((B, like.shape[1], ge.S * sl) + tuple(like.shape[3:]))
    return out


def _mirror(ge, eps2, tn, M, coef_dev=None):
    """per slot, from the numpy mirror of "adaptive projected guidance" applied to one slot at a time with m_prev = the slot's elements of
    M: (coef_ref [B*S, 4] = (s, k, w, g), d rows, e rows); with ``coef_dev`` e is built from the device's coefficients"""
    B = eps2.shape[0] // 2
    c = _rows(ge, ge.untok(eps2[:B])).cpu().numpy()
    u = _rows(ge, ge.untok(eps2[B:])).cpu().numpy()
    m = _rows(ge, M).cpu().numpy()
    g = GTAB.numpy()[np.clip(tn.cpu().numpy().reshape(-1), 0, T - 1)]
    e, d, (s, k, w) = AR.apg(c, u, g, APG[0], APG[1], BETA, m)
    if coef_dev is not None:
        e = AR.combine_f32(c, d, coef_dev[:, 2], coef_dev[:, 1])
    return np.stack([s, k, w, g], 1), d, e, (c, u)


def _composed(ge, z, e_lat, tl, tn, tp, eta, dpm, hist, first):
    from multimodal_diffusion_amd import functional as Fn
    noise = Fn.slot_noise(TG.SEED, tn, tuple(z.shape), ge.slot_len, first=first) if eta > 0 else None
    if dpm:
        h = hist.clone()
        return Fn.dpmpp_2m_step_slots(z, e_lat, h, tl, tn, tp, ABAR, ge.slot_len), h
    return Fn.ddim_step_slots(z, tn, tp, e_lat, ABAR, ge.slot_len, eta, noise), None


# ------------------------------------------------------------------------------------------------- 1. the fused updates, chained
@pytest.mark.parametrize("shape,patch", GEOMS)
def test_three_chained_fused_updates_equal_the_mirror(dev, shape, patch):
    """Per call: the coefficients within 2 ulp of the mirror; given those coefficients the output (and x0_hist) within 1e-6 relative of
    the functional slot update on the mirrored eps — the two bounds of test_gpu_slot_cfg.py's APG-against-fp64 check; the stored d is
    elementwise fp32 with one rounding per operation and is compared bit for bit, as are held slots and the uncovered tail."""
    from multimodal_diffusion_amd import functional as Fn
    ge = TG.Geom(shape, patch)
    B, S = ge.B, ge.S
    key = Fn.slot_key(TG.SEED, 3, S)
    for eta, dpm in UPDATES:
        z, _, tl, tn, tp, M = _inputs(ge, dev)
        hist = torch.randn(ge.shape, generator=torch.Generator().manual_seed(7)).to(dev) if dpm else None
        stepping = (tn != tp).reshape(-1).cpu().numpy()
        held = (SR.per_position(tn, ge.shape[2], ge.slot_len, z) == SR.per_position(tp, ge.shape[2], ge.slot_len, z)).expand_as(z)
        for call in range(3):
            eps2 = _inputs(ge, dev, seed=10 + call)[1]
            ctl = _ctl(dev, ge, M=M)
            M_before, h_before = M.clone(), None if hist is None else hist.clone()
            out = ge.run(dev, ge.shape, ge.patch, z, eps2, tn, tp, ctl.c, eta=eta, key=key if eta > 0 else None, tl=tl if dpm else None,
                         hist=hist)
            coef = ctl.coef().reshape(B * S, 4)
            coef_ref, d, e, (c, u) = _mirror(ge, eps2, tn, M_before, coef)
            assert AR.cancellation_free(c[stepping], d[stepping])
            assert np.isfinite(coef).all() and np.array_equal(coef[~stepping], np.tile(TG.SC.NEUTRAL, (int((~stepping).sum()), 1)))
            ul = CR.ulps(coef[stepping], coef_ref[stepping])
            print(f"{shape} eta {eta} dpm {dpm} call {call}: coefficient ulps max {ul.max(axis=0)}")
            assert ul.max() <= 2, (coef[stepping], coef_ref[stepping])
            # the buffer: d on the stepping slots, untouched under held slots and on the uncovered tail
            d_rows = torch.from_numpy(np.where(stepping[:, None], d, _rows(ge, M_before).cpu().numpy())).to(dev)
            assert torch.equal(M, _lat(ge, d_rows, M_before))
            assert torch.equal(M[held], M_before[held])
            if not ge.video and ge.shape[2] > S * ge.slot_len:
                assert bool((M[:, :, S * ge.slot_len:] == SENTINEL).all())
            e_lat = _lat(ge, torch.from_numpy(e).to(dev), torch.zeros_like(z))
            ref, href = _composed(ge, z, e_lat, tl, tn, tp, eta, dpm, h_before, 3)
            err = TG.rel(out, ref)
            print(f"{shape} eta {eta} dpm {dpm} call {call}: rel err {err:.3e}")
            assert torch.isfinite(out).all() and err <= 1e-6
            assert torch.equal(out[held], z[held])
            if dpm:
                assert TG.rel(hist, href) <= 1e-6 and torch.equal(hist[held], h_before[held])
            if call == 0:      # the momentum did something: today's slot APG differs
                free = TG.Ctl(dev, "apg", B, S, ge.per_slot)
                h2 = None if hist is None else h_before.clone()
                plain = ge.run(dev, ge.shape, ge.patch, z, eps2, tn, tp, free.c, eta=eta, key=key if eta > 0 else None,
                               tl=tl if dpm else None, hist=h2)
                assert not torch.equal(plain, out)
            z = out


def test_rows_and_gather_forms_agree_under_momentum(dev):
    from multimodal_diffusion_amd import functional as Fn
    for shape, patch in (V_ROWS, TG.GEOMS[0]):                      # the 4-token and the 8-token rows form
        ge = TG.Geom(shape, patch)
        z, eps2, tl, tn, tp, M0 = _inputs(ge, dev, seed=2)
        h0 = torch.randn(ge.shape, generator=torch.Generator().manual_seed(7)).to(dev)
        key = Fn.slot_key(TG.SEED, 0, ge.S)
        for eta, dpm in UPDATES + [(1.0, True)]:
            got = []
            for rows in (1, 0):
                with tuned(cfg_rows=rows):
                    M, h = M0.clone(), h0.clone() if dpm else None
                    ctl = _ctl(dev, ge, M=M)
                    out = TG._video(dev, ge.shape, ge.patch, z, eps2, tn, tp, ctl.c, eta=eta, key=key if eta > 0 else None,
                                    tl=tl if dpm else None, hist=h)
                    got.append((out, M, h, ctl.coef()))
            assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]) and np.array_equal(got[0][3], got[1][3])
            assert not torch.equal(got[0][1], M0)
            if dpm:
                assert torch.equal(got[0][2], got[1][2])


# ------------------------------------------------------------------------------------------------- 2. S = 1: the per-sample APG step
@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_one_slot_per_sample_is_the_per_sample_apg_step_with_momentum(dev, model, target, solver):
    """three chained steps: ``step_slots`` under ``set_slot_cfg(apg=, apg_momentum=)`` is ``step`` under ``set_apg(momentum=)`` with
    g_b = g(t_b), bit for bit: output, momentum buffer, coefficients and x0_hist"""
    z, zp, npr = TG._s1_case(dev, target)
    dpm = solver == "dpmpp_2m"
    a = engine(model[1], target, tuple(z.shape), npr, guidance=GS, solver=solver)      # slots
    b = engine(model[1], target, tuple(z.shape), npr, guidance=GS, solver=solver)      # per sample
    assert a.slots == 1
    for e in (a, b):
        e.set_prompt(zp)
    a.set_slot_cfg(guidance=GTAB, apg={"norm_threshold": APG[0], "eta_parallel": APG[1]}, apg_momentum=BETA)
    b.set_apg(APG[0], APG[1], BETA)
    b._zero_apg_momentum()
    assert a.slot_momentum is not None and not a.slot_momentum.any()
    steps = [([981, 402], [961, 382], [-1, -1]), ([961, 382], [941, 362], [981, 402]), ([941, 362], [921, 342], [961, 382])]
    za = zb = z
    for i, (now, prev, last) in enumerate(steps):
        tn, tp, tl = (torch.tensor(v).view(2, 1) for v in (now, prev, last))
        b.set_cfg(guidance=GTAB[tn[:, 0]].tolist())
        za = a.step_slots(za, tn, tp, t_last=tl if dpm else None)
        zb = b.step(zb, tn[:, 0].to(dev), tp[:, 0].to(dev), t_last=tl[:, 0].to(dev) if dpm else None)
        assert torch.isfinite(za).all() and torch.equal(za, zb), i
        assert torch.equal(a.slot_momentum, b.apg_momentum) and a.slot_momentum.any(), i
        assert torch.equal(a.slot_cfg_coef()[:, 0], b._apg_stats[b._apg_stats.numel() - 32:].view(torch.float32).view(2, 4)), i
        if dpm:
            assert torch.equal(a.x0_hist, b.x0_hist), i
    a.clear_slot_cfg()
    assert a.slot_momentum is None and a._smom is None


# ------------------------------------------------------------------------------------------------- 3. held slots, the tail, placement
@pytest.mark.parametrize("shape,patch", [V_ROWS, V_RAGGED, A_TAIL])
def test_a_slot_gives_the_same_bits_wherever_it_sits(dev, shape, patch):
    """copy one slot's eps tokens, z, pair and momentum elements into another (b, s) of a batch of 3 with other neighbours: its
    coefficients, its output and its new momentum are bit-equal"""
    ge = TG.Geom(shape, patch)
    assert ge.B == 2
    z, eps2, _, tn, tp, M = _inputs(ge, dev, seed=3)
    step = [(b, s) for b in range(2) for s in range(ge.S) if tn[b, s] != tp[b, s]]
    bs, ss = step[0]
    z3, eps3, _, tn3, tp3, M3 = _inputs(ge, dev, seed=4, B=3)
    bd, sd = 2, (ss + 1) % ge.S
    per, sl = ge.Nt // ge.S, ge.slot_len
    for half_src, half_dst in ((0, 0), (2, 3)):
        eps3[half_dst + bd, sd * per:(sd + 1) * per] = eps2[half_src + bs, ss * per:(ss + 1) * per]
    z3[bd, :, sd * sl:(sd + 1) * sl] = z[bs, :, ss * sl:(ss + 1) * sl]
    M3[bd, :, sd * sl:(sd + 1) * sl] = M[bs, :, ss * sl:(ss + 1) * sl]
    tn3[bd, sd], tp3[bd, sd] = tn[bs, ss], tp[bs, ss]
    c2, c3 = _ctl(dev, ge, M=M), _ctl(dev, ge, B=3, M=M3)
    M_before = M.clone()
    out2 = ge.run(dev, ge.shape, ge.patch, z, eps2, tn, tp, c2.c)
    out3 = ge.run(dev, (3,) + ge.shape[1:], ge.patch, z3, eps3, tn3, tp3, c3.c)
    assert np.array_equal(c2.coef()[bs, ss], c3.coef()[bd, sd]) and np.isfinite(c2.coef()[bs, ss]).all()
    assert torch.equal(out2[bs, :, ss * sl:(ss + 1) * sl], out3[bd, :, sd * sl:(sd + 1) * sl])
    assert torch.equal(M[bs, :, ss * sl:(ss + 1) * sl], M3[bd, :, sd * sl:(sd + 1) * sl])
    assert not torch.equal(M[bs, :, ss * sl:(ss + 1) * sl], M_before[bs, :, ss * sl:(ss + 1) * sl])


def test_a_wholly_held_batch_touches_nothing(dev):
    for shape, patch in (V_ROWS, A_TAIL):
        ge = TG.Geom(shape, patch)
        z, eps2, tl, tn, _, M = _inputs(ge, dev, seed=6)
        h0 = torch.randn(ge.shape, generator=torch.Generator().manual_seed(7)).to(dev)
        M0, h = M.clone(), h0.clone()
        ctl = _ctl(dev, ge, M=M)
        out = ge.run(dev, ge.shape, ge.patch, z, eps2, tn, tn.clone(), ctl.c, tl=tl, hist=h)
        assert torch.equal(out, z) and torch.equal(M, M0) and torch.equal(h, h0)


# ------------------------------------------------------------------------------------------------- 4. beta = 0 and the zero buffer
@pytest.mark.parametrize("shape,patch", [V_ROWS, V_RAGGED, V_ONE, A_TAIL])
def test_a_zero_buffer_gives_the_first_step_the_bits_of_todays_slot_apg(dev, shape, patch):
    ge = TG.Geom(shape, patch)
    z, eps2, tl, tn, tp, _ = _inputs(ge, dev, seed=8)
    today = TG.Ctl(dev, "apg", ge.B, ge.S, ge.per_slot)               # the 48-byte control, apg = 1: today's call
    assert C.sizeof(today.c) == 48 and today.c.apg == 1
    none = _ctl(dev, ge, beta=0.0, M=None)                            # the momentum struct at beta = 0: the same launches
    assert torch.equal(ge.run(dev, ge.shape, ge.patch, z, eps2, tn, tp, none.c), ge.run(dev, ge.shape, ge.patch, z, eps2, tn, tp, today.c))
    ref = ge.run(dev, ge.shape, ge.patch, z, eps2, tn, tp, today.c)
    M = torch.zeros(ge.shape, device=dev)
    ctl = _ctl(dev, ge, M=M)
    out = ge.run(dev, ge.shape, ge.patch, z, eps2, tn, tp, ctl.c)
    assert torch.equal(out, ref) and np.array_equal(ctl.coef(), today.coef())
    d0 = ge.untok(eps2[:ge.B]) - ge.untok(eps2[ge.B:])                # the buffer now holds d = d0 under the stepping slots
    stepping = (SR.per_position(tn, ge.shape[2], ge.slot_len, z) != SR.per_position(tp, ge.shape[2], ge.slot_len, z)).expand_as(z)
    if not ge.video:
        stepping = stepping.clone()
        stepping[:, :, ge.S * ge.slot_len:] = False
    assert torch.equal(M[stepping], d0[stepping]) and not M[~stepping].any()


def test_engine_without_a_momentum_is_todays_slot_apg(dev, model):
    z, zp, npr, _ = TG.case(dev, "video")
    eng = engine(model[1], "video", tuple(z.shape), npr, guidance=GS)
    eng.set_prompt(zp)
    tn, tp = SR.tables(2, eng.slots, seed=5)
    apg = {"norm_threshold": APG[0], "eta_parallel": APG[1]}
    eng.set_slot_cfg(guidance=GTAB, apg=apg)
    ref = eng.step_slots(z, tn, tp)
    for mom in (None, 0, 0.0):
        eng.set_slot_cfg(guidance=GTAB, apg=apg, apg_momentum=mom)
        assert eng.slot_momentum is None and C.sizeof(eng._scfg) == 48 and eng._scfg.apg == 1
        assert torch.equal(eng.step_slots(z, tn, tp), ref)
    eng.set_slot_cfg(guidance=GTAB, apg=apg, apg_momentum=BETA)      # a zeroed buffer: the first step's bits, then not
    assert torch.equal(eng.step_slots(z, tn, tp), ref)
    # (the same eps again would give d = d0 / 2, which under the norm cap is the same e: step on from another latent)
    second = eng.step_slots(ref, tn, tp)
    eng.set_slot_cfg(guidance=GTAB, apg=apg)
    assert not torch.equal(eng.step_slots(ref, tn, tp), second)


# ------------------------------------------------------------------------------------------------- 5. the carry
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("B,S,ctx", CARRY_CASES)
def test_fifo_carry_equals_the_torch_statement(dev, B, S, ctx, shift):
    """16-byte lanes (inner % 4 == 0, aligned), scalar lanes (inner 15 and the audio layout's inner 1), and a base that is 4 bytes off
    a 16-byte boundary, which forces the scalar path on a vector-shaped buffer: the same bits as the CPU reference"""
    from multimodal_diffusion_amd import functional as Fn
    sl = 2
    g = torch.Generator().manual_seed(B * 16 + S * 4 + ctx)
    for tail in ((2, 4), (3, 5), ()):
        buf = torch.randn((B, 3, S * sl) + tail, generator=g)
        ref = Fn.fifo_carry(buf, S, sl, ctx=ctx, shift=shift)
        got = Fn.fifo_carry(buf.to(dev), S, sl, ctx=ctx, shift=shift)
        assert got.is_cuda and torch.equal(got.cpu(), ref), tail
    buf = torch.randn(B, 3, S * sl, 2, 4, generator=g)
    flat_in, flat_out = torch.zeros(buf.numel() + 4, device=dev), torch.full((buf.numel() + 4,), 7.0, device=dev)
    src, dst = flat_in[1:1 + buf.numel()].view(buf.shape), flat_out[1:1 + buf.numel()].view(buf.shape)
    assert src.data_ptr() % 16 == 4 and src.is_contiguous()
    src.copy_(buf)
    assert Fn.fifo_carry(src, S, sl, ctx=ctx, shift=shift, out=dst) is dst
    assert torch.equal(dst.cpu(), Fn.fifo_carry(buf, S, sl, ctx=ctx, shift=shift))
    assert float(flat_out[0]) == 7.0 and bool((flat_out[1 + buf.numel():] == 7.0).all())      # nothing outside the view


def test_fifo_carry_refuses_an_overlap_before_any_launch(dev):
    L, lib = TG._lib()
    flat = torch.full((2 * 96 + 8,), 7.0, device=dev)
    n = 2 * 3 * 4 * 4
    for off in (0, 4, n - 4):
        rc = lib.avd_fifo_carry_f32(flat.data_ptr(), flat.data_ptr() + 4 * off, 2, 3, 2, 0, 1, 2, 4, L.stream_ptr(dev))
        assert rc == L.EINVAL and b"must not overlap" in lib.avd_last_error()
    for args, word in (((2, 3, 2, 2, 1, 2, 4), b"ctx"), ((2, 3, 2, 0, 2, 2, 4), b"shift"), ((0, 3, 2, 0, 1, 2, 4), b"bad dims")):
        rc = lib.avd_fifo_carry_f32(flat.data_ptr(), flat.data_ptr() + 4 * n, *args, L.stream_ptr(dev))
        assert rc == L.EINVAL and word in lib.avd_last_error()
    assert lib.avd_fifo_carry_f32(None, flat.data_ptr(), 2, 3, 2, 0, 1, 2, 4, L.stream_ptr(dev)) == L.EINVAL
    torch.cuda.synchronize()
    assert bool((flat == 7.0).all())


# ------------------------------------------------------------------------------------------------- 6. the queue
K = 6
AKW = dict(apg={"norm_threshold": 20.0, "eta_parallel": 0.5}, apg_momentum=BETA)


def _torch_carry(eng, before, ctx, shift):
    """replace what the engine's own carry launch left by the torch statement on the buffer's state before the move"""
    from multimodal_diffusion_amd import functional as Fn
    eng.slot_momentum.copy_(Fn.fifo_carry(before, eng.slots, eng.slot_len, ctx=ctx, shift=shift))


def _plain_loop(eng, canvas_p, hop, sched, n_slots, seed):
    """fifo_denoise restated from step_slots, fifo_shift and functional.fifo_carry on the host"""
    from multimodal_diffusion_amd import functional as Fn, schedule_utils as su
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_len, fifo_prompt_windows
    B, S = eng.embed.B, eng.slots
    rn, rp, sn, sp = su.fifo_plan(sched, S)
    dpm = eng.solver == "dpmpp_2m"
    rl, last = su.fifo_plan_last(sched, S) if dpm else (None, None)
    n, s0 = B * S, int(sched[0])
    Lp = fifo_prompt_len(eng, canvas_p)
    z = Fn.canvas_noise(seed, torch.full((B,), s0), eng.latent_shape, eng.latent_shape[2])
    eng.set_prompt(fifo_prompt_windows(canvas_p, 0, B, S, hop, Lp))
    eng.slot_momentum.zero_()
    for r in range(n - 1):
        z = eng.step_slots(z, rn[r], rp[r], t_last=rl[r] if dpm else None)
    done = []
    for m in range(n_slots):
        eng.set_prompt(fifo_prompt_windows(canvas_p, m, B, S, hop, Lp))
        z = eng.step_slots(z, sn, sp, t_last=last)
        before = eng.slot_momentum.cpu()
        z, popped = eng.fifo_shift(z, n + m, s0, seed=seed)
        _torch_carry(eng, before, 0, 1)
        done.append(popped)
    return torch.cat(done, 1)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_fifo_denoise_with_momentum_eager_graph_and_loop(dev, model, solver):
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop = TG._queue(dev, model[1], solver=solver)
    free = A.fifo_denoise(eng, canvas_p, hop, TG.SCHED4, K, TG.QSEED, apg=AKW["apg"])
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, TG.SCHED4, K, TG.QSEED, apg=AKW["apg"], apg_momentum=None), free)
    eager = A.fifo_denoise(eng, canvas_p, hop, TG.SCHED4, K, TG.QSEED, **AKW)
    assert eng._scfg is None and eng.slot_momentum is None            # set for the call only
    assert torch.isfinite(eager).all() and not torch.equal(eager, free)
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, TG.SCHED4, K, TG.QSEED, **AKW), eager)       # every call starts from zero
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, TG.SCHED4, K, TG.QSEED, graph=True, **AKW), eager)
    assert eng._scfg is None and eng.slot_momentum is None
    eng.set_slot_cfg(**AKW)
    ref = _plain_loop(eng, canvas_p, hop, TG.SCHED4, K, TG.QSEED)
    assert eng.slot_momentum.any()
    eng.clear_slot_cfg()
    assert torch.equal(eager, ref), float((eager - ref).abs().max())


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_fifo_lookahead_with_momentum_equals_its_loop(dev, model, solver):
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_len
    eng, canvas_p, hop = TG._queue(dev, model[1], solver=solver)
    sched, ctx = [999, 499, -1], 1                                    # lookahead = 1 of S = 2: h = 1, n = B * h = 2 steps
    out = A.fifo_denoise(eng, canvas_p, hop, torch.tensor(sched), K, TG.QSEED, lookahead=ctx, **AKW)
    assert eng._scfg is None and torch.isfinite(out).all()
    assert not torch.equal(out, A.fifo_denoise(eng, canvas_p, hop, torch.tensor(sched), K, TG.QSEED, lookahead=ctx, apg=AKW["apg"]))
    shape = eng.latent_shape

    def noise(p0, n_pos):
        return Fn.canvas_noise(TG.QSEED, torch.tensor([999]), (1, shape[1], n_pos) + tuple(shape[3:]), 1, window_offset=p0)[0]

    # LR.loop with the carry behind every move
    eng.set_slot_cfg(**AKW)
    B, S, sl = eng.embed.B, eng.slots, eng.slot_len
    h = S - ctx
    n = B * h
    Lp = fifo_prompt_len(eng, canvas_p)
    rn, rp, rl, sn, sp, slast = LR.plan(sched, S, ctx, "noise")
    dpm = solver == "dpmpp_2m"
    head, act = noise(2 ** 32 - ctx * sl, ctx * sl), noise(0, n * sl)
    old = [head[:, q * sl:(q + 1) * sl] for q in range(ctx)] + [act[:, a * sl:(a + 1) * sl] for a in range(n)]
    z = LR.windows(old, B, S, ctx)
    eng.set_prompt(LR.prompt_windows(canvas_p, -ctx, B, h, hop, Lp))
    done = []
    for it in range(n - 1 + K):
        ramp, m = it < n - 1, it - (n - 1)
        if not ramp:
            eng.set_prompt(LR.prompt_windows(canvas_p, m - ctx, B, h, hop, Lp))
        row = it if ramp else min(m, ctx)
        tabs = (rn, rp, rl) if ramp else (sn, sp, slast)
        z = eng.step_slots(z, tabs[0][row], tabs[1][row], t_last=tabs[2][row] if dpm else None)
        shift = 0 if ramp else 1
        if dpm:
            eng.x0_hist.copy_(LR.lookahead_hist(eng.x0_hist, ctx, shift, sl))
        _torch_carry(eng, eng.slot_momentum.cpu(), ctx, shift)
        if ramp:
            z, _ = LR.lookahead(z, ctx, 0, sl)
        else:
            z, popped = LR.lookahead(z, ctx, 1, sl, noise((n + m) * sl, sl))
            done.append(popped)
    eng.clear_slot_cfg()
    ref = torch.cat(done, 1)
    assert torch.equal(out, ref), float((out - ref).abs().max())


def test_fifo_denoise_momentum_with_init_canvas(dev, model):
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop = TG._queue(dev, model[1], eta=0.5, noise_seed=11)
    sl = eng.slot_len
    known = torch.randn((8, 3 * sl, 16, 16), generator=torch.Generator().manual_seed(3)).to(dev)
    from multimodal_diffusion_amd.sampler import canvas_frame_mask
    mask = canvas_frame_mask(tuple(known.shape), sl, 2 * sl)
    kw = dict(init_canvas=known, mask=mask, guide_seed=TG.GSEED)
    part = A.fifo_denoise(eng, canvas_p, hop, TG.SCHED4, 3, TG.QSEED, **kw, **AKW)
    base = A.fifo_denoise(eng, canvas_p, hop, TG.SCHED4, 3, TG.QSEED, apg=AKW["apg"], **kw)
    assert torch.equal(part[:, sl:2 * sl], known[:, sl:2 * sl]) and torch.isfinite(part).all()       # the held region, bit for bit
    assert not torch.equal(part[:, 2 * sl:], base[:, 2 * sl:])
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, TG.SCHED4, 3, TG.QSEED, guided_shift=True, **kw, **AKW), part)
    assert eng._scfg is None and eng._clip is None and eng.slot_momentum is None


# ------------------------------------------------------------------------------------------------- 7. the C entries' refusals
def test_c_abi_refusals_launch_nothing(dev):
    L, lib = TG._lib()
    ge = TG.Geom(*V_ROWS)
    z, eps2, _, tn, tp, M = _inputs(ge, dev, seed=5)
    M0 = M.clone()
    out = torch.full(ge.shape, 7.0, device=dev)
    ab = ABAR.to(dev)

    def call(cfg):
        return lib.avd_cfg_unpatch_ddim_slots_cfg_f32(eps2.data_ptr(), z.data_ptr(), None, tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), T, GS,
                                                      0.0, None, None, ge.S, None, out.data_ptr(), *ge.shape, *ge.patch, C.byref(cfg),
                                                      L.stream_ptr(dev))

    c = _ctl(dev, ge, beta=0.0, M=M)                                  # a buffer without beta
    assert call(c.c) == L.EINVAL and b"exactly when momentum != 0" in lib.avd_last_error()
    c = _ctl(dev, ge, beta=BETA, M=None)                              # beta without a buffer
    assert call(c.c) == L.EINVAL and b"exactly when momentum != 0" in lib.avd_last_error()
    c = _ctl(dev, ge, beta=float("nan"), M=M)
    assert call(c.c) == L.EINVAL and b"finite" in lib.avd_last_error()
    c = _ctl(dev, ge, M=M)
    c.c.momentum_buf += 4
    assert call(c.c) == L.EUNSUPPORTED and b"momentum_buf must be 16-byte aligned" in lib.avd_last_error()
    c = _ctl(dev, ge, M=M)
    for t in (out, z, eps2, c.stats):
        c.c.momentum_buf = t.data_ptr() + 64
        assert call(c.c) == L.EINVAL and b"momentum_buf must not overlap" in lib.avd_last_error()
    # momentum without apg: the C control cannot state it (apg itself says that the two fields follow); with a rescale table beside it
    # the momentum struct is refused as APG beside a rescale is, and the engine refuses apg_momentum without apg (the CPU tests)
    c = _ctl(dev, ge, M=M)
    c.p = TG.PTAB.to(dev, torch.float32).contiguous()
    c.c.rescale_t = c.p.data_ptr()
    assert call(c.c) == L.EINVAL and b"together with APG" in lib.avd_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and torch.equal(M, M0)


def test_the_whole_step_checks_the_buffer_against_its_workspace(dev, model):
    """the composite entry makes the control's checks before the model runs, with the workspace as the eps source"""
    zz, zp, npr, _ = TG.case(dev, "video")
    eng = engine(model[1], "video", tuple(zz.shape), npr, guidance=GS)
    eng.set_prompt(zp)
    eng.set_slot_cfg(apg={"norm_threshold": 1.0}, apg_momentum=BETA)
    tn = torch.full((2, eng.slots), 500)
    o = torch.full_like(zz, 7.0)
    eng._scfg.momentum_buf = eng.workspace.data_ptr() + 64
    with pytest.raises(ValueError, match="momentum_buf must not overlap"):
        eng.step_slots(zz, tn, tn - 50, out=o)
    eng._scfg.momentum_buf = zz.data_ptr()
    with pytest.raises(ValueError, match="momentum_buf must not overlap"):
        eng.step_slots(zz, tn, tn - 50, out=o)
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and not eng.slot_momentum.any()
    with pytest.raises(ValueError, match="no momentum"):
        eng.set_slot_cfg(apg={"norm_threshold": 1.0, "momentum": -0.5}, apg_momentum=BETA)


# ------------------------------------------------------------------------------------------------- the pipeline
import test_gpu_stream_fifo as TS  # noqa: E402
from test_gpu_stream_fifo import one_second  # noqa: E402,F401  (a fixture)


def test_stream_generate_takes_apg_momentum(one_second):  # noqa: F811
    """fifo={"apg_momentum":} and streaming.fifo.apg_momentum reach fifo_denoise: the canvas of the call by hand, bit for bit"""
    case = one_second
    apg = {"norm_threshold": 2.0, "eta_parallel": 0.5}
    cfg = TS.with_sampling(case.cfg, apg={"video": apg})
    free = TS._fifo(case, cfg=cfg)["latent_canvas"]
    got = TS._fifo(case, cfg=cfg, fifo={"apg_momentum": BETA})["latent_canvas"]
    assert np.array_equal(got, case.by_hand(apg=apg, apg_momentum=BETA).cpu().numpy()) and not np.array_equal(got, free)
    by_cfg = TS._fifo(case, cfg=dict(cfg, streaming=dict(cfg["streaming"], fifo={"apg_momentum": BETA})))["latent_canvas"]
    assert np.array_equal(by_cfg, got)
    assert np.array_equal(TS._fifo(case, cfg=cfg, fifo={"apg_momentum": 0.0})["latent_canvas"], free)
    with pytest.raises(ValueError, match="needs sampling.apg"):
        TS._fifo(case, fifo={"apg_momentum": BETA})
