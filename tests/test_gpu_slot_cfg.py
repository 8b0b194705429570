"""The slot CFG control on the MI355X (include/avdiff_hip.h, "slot CFG control"): the fused slot updates under a guidance table, a
per-slot rescale and per-slot APG against the numpy mirror; the bit identities (a constant table against the existing slot entries, rows
against gather, a slot's numbers wherever it sits); S = 1 against the per-sample controlled step; the whole step against the composed
path; ``fifo_denoise`` in its three drivers; misuse.  Reduced model, the kit's small shapes."""
import ctypes as C

import numpy as np
import pytest
import torch

import _apg_ref as AR
import _cfg_ref as CR
import _lookahead_ref as LR
import _slot_cfg_ref as SC
import _slot_ref as SR
from _kit import ABAR, case, dev, engine, model  # noqa: F401  (dev, model are fixtures)
from _tune import tuned

pytestmark = pytest.mark.gpu

GS = 3.5
T = 1000
SEED = 0x5107_5EED_0001         # the slot key: the step noise
GSEED = 0x4B4E0BADCAFE          # the clip guide's known noise
QSEED = 0x5EED0F1F0             # a queue's start and entering noise
GTAB = torch.linspace(1.0, 6.0, T)                         # guidance rises with the noise level
PTAB = 0.25 + 0.5 * torch.linspace(0.0, 1.0, T)            # phi in [0.25, 0.75]
APG = (2.0, 0.25)                                          # (r, eta_p): r caps the norm of the small slots' d, not of the large ones'
MODES = ["table", "rescale", "apg"]
# (eta, dpm): DDIM, seeded DDIM, DPM-Solver++(2M), its SDE form
UPDATES = [(0.0, False), (0.5, False), (0.0, True), (1.0, True)]


def _lib():
    from multimodal_diffusion_amd import _lib as L
    return L, L.lib()


def rel(a, b):
    """the bound of test_fused_equals_composed: the relative error in norm"""
    return float((a - b).norm() / b.norm())


class Ctl:
    """an avd_slot_cfg over device tables and a scratch of its own; ``coef()`` reads the scratch's tail"""

    def __init__(self, dev, mode, B, S, per_slot, gtab=GTAB, ptab=PTAB, apg=APG, pad=0):
        L, lib = _lib()
        self.mode, self.B, self.S = mode, B, S
        self.g = None if gtab is None else gtab.to(dev, torch.float32).contiguous()
        self.p = ptab.to(dev, torch.float32).contiguous() if mode == "rescale" else None
        self.nb = lib.avd_slot_cfg_stats_bytes(B, S, per_slot) if mode != "table" else 0
        assert self.nb >= 0
        self.stats = torch.full((self.nb + pad,), 0xFF, dtype=torch.uint8, device=dev) if self.nb else None       # NaN bytes: nothing stale reads as a number
        r, eta_p = apg if mode == "apg" else (0.0, 0.0)
        self.c = L.SlotCfg(L.ptr(self.g), L.ptr(self.p), 1 if mode == "apg" else 0, r, eta_p, L.ptr(self.stats), self.nb)

    def coef(self):
        return self.stats[self.nb - 16 * self.B * self.S:self.nb].view(torch.float32).view(self.B, self.S, 4).cpu().numpy()


# ------------------------------------------------------------------------------------------------- the fused updates through the C entries
def _video(dev, shape, tube, z, eps2, tn, tp, cfg=None, eta=0.0, key=None, guide=None, tl=None, hist=None):
    """z_out of avd_cfg_unpatch_ddim_slots_cfg_f32 (cfg set) or of the existing entry the arguments select"""
    L, lib = _lib()
    B, Cc, T_, H, W = shape
    out, ab = torch.full(shape, float("nan"), device=dev), ABAR.to(dev)
    tail = (T_ // tube[0], L.ptr(hist), out.data_ptr(), B, Cc, T_, H, W, *tube)
    head = (eps2.data_ptr(), z.data_ptr(), L.ptr(tl), tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), T, GS, eta)
    kp, gp = (None if key is None else C.byref(key)), (None if guide is None else C.byref(guide))
    if cfg is not None:
        L.check(lib.avd_cfg_unpatch_ddim_slots_cfg_f32(*head, kp, gp, *tail, C.byref(cfg), L.stream_ptr(dev)))
    elif guide is not None:
        L.check(lib.avd_cfg_unpatch_ddim_slots_guided_f32(*head, kp, gp, *tail, L.stream_ptr(dev)))
    elif key is not None or tl is not None:      # at eta == 0 the key is required and not read
        L.check(lib.avd_cfg_unpatch_ddim_slots_seeded_f32(*head, C.byref(key or L.SlotKey(0, 0, 1, None)), *tail, L.stream_ptr(dev)))
    else:
        L.check(lib.avd_cfg_unpatch_ddim_slots_f32(eps2.data_ptr(), z.data_ptr(), tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), T, GS,
                                                   T_ // tube[0], out.data_ptr(), B, Cc, T_, H, W, *tube, L.stream_ptr(dev)))
    return out


def _audio(dev, shape, chunk, z, eps2, tn, tp, cfg=None, eta=0.0, key=None, guide=None, tl=None, hist=None):
    L, lib = _lib()
    B, Ca, F = shape
    Na = (F - chunk[0]) // chunk[1] + 1
    out, ab = torch.full(shape, float("nan"), device=dev), ABAR.to(dev)
    tail = (Na, L.ptr(hist), out.data_ptr(), B, Ca, F, *chunk)
    head = (eps2.data_ptr(), z.data_ptr(), L.ptr(tl), tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), T, GS, eta)
    kp, gp = (None if key is None else C.byref(key)), (None if guide is None else C.byref(guide))
    if cfg is not None:
        L.check(lib.avd_cfg_untoken_ddim_audio_slots_cfg_f32(*head, kp, gp, *tail, C.byref(cfg), L.stream_ptr(dev)))
    elif guide is not None:
        L.check(lib.avd_cfg_untoken_ddim_audio_slots_guided_f32(*head, kp, gp, *tail, L.stream_ptr(dev)))
    elif key is not None or tl is not None:
        L.check(lib.avd_cfg_untoken_ddim_audio_slots_seeded_f32(*head, C.byref(key or L.SlotKey(0, 0, 1, None)), *tail, L.stream_ptr(dev)))
    else:
        L.check(lib.avd_cfg_untoken_ddim_audio_slots_f32(eps2.data_ptr(), z.data_ptr(), tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), T, GS, Na,
                                                         out.data_ptr(), B, Ca, F, *chunk, L.stream_ptr(dev)))
    return out


class Geom:
    """one case of the fused update alone: the latent, the token layout and its slots"""

    def __init__(self, shape, patch):
        self.shape, self.patch, self.video = tuple(shape), tuple(patch), len(shape) == 5
        self.B = shape[0]
        if self.video:
            _, Cc, T_, H, W = shape
            t, h, w = patch
            self.S, self.slot_len, self.Nt, self.D = T_ // t, t, (T_ // t) * (H // h) * (W // w), Cc * t * h * w
            self.per_slot = Cc * t * H * W
        else:
            _, Ca, F = shape
            self.S = self.Nt = (F - patch[0]) // patch[1] + 1
            self.slot_len, self.D, self.per_slot = patch[0], Ca * patch[0], Ca * patch[0]
        self.run = _video if self.video else _audio

    def untok(self, tok):
        from multimodal_diffusion_amd import functional as Fn
        if self.video:
            return Fn.tube_unpatch(tok.contiguous(), *self.shape[1:], *self.patch)
        return Fn.audio_untokens(tok.contiguous(), self.shape[1], self.patch[0], self.shape[2], self.patch[1])

    def inputs(self, dev, seed=0, B=None):
        """(z, eps2 [2B, Nt, D], t_last, t_now, t_prev, the constant slot): cond random, null correlated with it (so that S_dc does not
        cancel), mixed pairs with holds from _slot_ref.tables, and one stepping slot whose cond and null tokens are one constant
        (None where the tables leave a single stepping slot: B * S = 2 holds one hold and one step)"""
        B = self.B if B is None else B
        shape = (B,) + self.shape[1:]
        g = torch.Generator().manual_seed(sum(self.shape) + self.patch[0] + seed)
        z = torch.randn(shape, generator=g)
        c = torch.randn(B, self.Nt, self.D, generator=g)
        u = 0.2 * c + 0.5 * torch.randn(B, self.Nt, self.D, generator=g)      # corr(c - u, c) ~ 0.85: clear of 0 at 32 elements too
        tn, tp = SR.tables(B, self.S, seed=self.S * 8 + B + seed)
        step = [(b, s) for b in range(B) for s in range(self.S) if tn[b, s] != tp[b, s]]
        const = step[len(step) // 2] if len(step) >= 2 else None
        per = self.Nt // self.S
        if const is not None:
            b0, s0 = const
            c[b0, s0 * per:(s0 + 1) * per] = 0.375
            u[b0, s0 * per:(s0 + 1) * per] = 0.375
        sc = SR.SCHED
        tl = torch.tensor([[sc[sc.index(int(a)) - 1] if sc.index(int(a)) > 0 else -1 for a in row] for row in tn])
        tl[step[0]] = -1                                         # a first-order slot beside the second-order ones
        eps2 = torch.cat([c, u]).to(dev)
        return z.to(dev), eps2, tl.to(dev), tn.to(dev), tp.to(dev), const


# the 8-token rows form, the gather form, S = 4 (tube t = 1), a ragged last chunk on the 4-token rows form (per_slot = 2304); audio
# S = 10 with per_slot = 32, the second with an uncovered tail
GEOMS = [((2, 8, 4, 16, 32), (2, 4, 4)), ((2, 8, 4, 16, 8), (2, 4, 4)), ((2, 8, 4, 16, 32), (1, 4, 4)), ((1, 6, 4, 12, 16), (2, 4, 4)),
         ((2, 8, 40), (4, 4)), ((2, 8, 42), (4, 4))]


def _composed(ge, z, eps_tok, tl, tn, tp, eta, dpm, h0, key_first=None):
    """the functional slot update on the mirrored eps: (z_out, x0_hist or None)"""
    from multimodal_diffusion_amd import functional as Fn
    e = ge.untok(eps_tok)
    noise = Fn.slot_noise(SEED, tn, tuple(z.shape), ge.slot_len, first=key_first) if eta > 0 else None
    if dpm:
        h = h0.clone()
        if eta > 0:
            return Fn.dpmpp_2m_sde_step_slots(z, e, h, tl, tn, tp, ABAR, ge.slot_len, eta, noise), h
        return Fn.dpmpp_2m_step_slots(z, e, h, tl, tn, tp, ABAR, ge.slot_len), h
    return Fn.ddim_step_slots(z, tn, tp, e, ABAR, ge.slot_len, eta, noise), None


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,patch", GEOMS)
def test_fused_update_equals_the_mirror(dev, shape, patch, mode):
    """Coefficients read from the scratch within 2 ulp of the mirror (the bound of test_functional_matches_mirror for the same fp64
    construction); given those coefficients the output within 1e-6 relative of the functional slot update on the mirrored eps (the bound
    of test_fused_equals_composed); held slots z bit for bit; finite; not the plain slot entry."""
    from multimodal_diffusion_amd import functional as Fn
    ge = Geom(shape, patch)
    B, S = ge.B, ge.S
    z, eps2, tl, tn, tp, const = ge.inputs(dev)
    ec, en = eps2[:B].cpu().numpy(), eps2[B:].cpu().numpy()
    tn_c, tp_c = tn.cpu().numpy(), tp.cpu().numpy()
    _, coef_ref = SC.control(ec, en, tn_c, tp_c, GS, T, GTAB.numpy(), PTAB.numpy() if mode == "rescale" else None,
                             APG if mode == "apg" else None)
    stepping = tn_c != tp_c
    assert stepping.any() and (~stepping).any() and (const is not None or B * S == 2)
    free = stepping.copy()
    if const is not None:
        free[const] = False
    assert free.any()
    if mode == "apg":      # the 2 ulp of k need S_dc free of cancellation (test_gpu_apg.py's input condition), per stepping random slot
        cs, us = SC.slot_tokens(ec, S), SC.slot_tokens(en, S)
        assert AR.cancellation_free(cs[free], cs[free] - us[free])
        assert const is None or (coef_ref[const][0] == 1.0 and coef_ref[const][1] == 0.0)       # d == 0: S_dd == 0 and S_dc == 0
        assert (coef_ref[free][:, 0] < 1.0).any()                               # and r caps some slot
    if mode == "rescale":
        assert const is None or coef_ref[const][0] == 1.0                       # y == c == a constant: sigma_y == 0
    h0 = torch.randn(ge.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    key = Fn.slot_key(SEED, 3, S)
    held = (SR.per_position(tn, ge.shape[2], ge.slot_len, z) == SR.per_position(tp, ge.shape[2], ge.slot_len, z)).expand_as(z)
    for eta, dpm in UPDATES:
        ctl = Ctl(dev, mode, B, S, ge.per_slot)
        hist = h0.clone() if dpm else None
        kw = dict(eta=eta, key=key if eta > 0 else None, tl=tl if dpm else None, hist=hist)
        out = ge.run(dev, ge.shape, ge.patch, z, eps2, tn, tp, ctl.c, **kw)
        if mode == "table":
            coef = coef_ref
        else:
            coef = ctl.coef()
            assert np.isfinite(coef).all()
            assert np.array_equal(coef[~stepping], np.tile(SC.NEUTRAL, (int((~stepping).sum()), 1)))
            ul = CR.ulps(coef[stepping], coef_ref[stepping])
            print(f"{mode} {shape} eta {eta} dpm {dpm}: coefficient ulps max {ul.max(axis=0)}")
            assert ul.max() <= 2, (coef[stepping], coef_ref[stepping])
        eps_tok = torch.from_numpy(SC.apply(ec, en, coef, mode == "apg")).to(dev)
        ref, href = _composed(ge, z, eps_tok, tl, tn, tp, eta, dpm, h0, key_first=3)
        err = rel(out, ref)
        print(f"{mode} {shape} eta {eta} dpm {dpm}: rel err {err:.3e}")
        assert torch.isfinite(out).all() and err <= 1e-6
        assert torch.equal(out[held], z[held])
        if dpm:
            assert rel(hist, href) <= 1e-6 and torch.equal(hist[held], h0[held])
        hp = h0.clone() if dpm else None
        plain = ge.run(dev, ge.shape, ge.patch, z, eps2, tn, tp, None, **dict(kw, hist=hp))
        assert not torch.equal(plain, out)
        if not ge.video and ge.shape[2] % ge.patch[0]:      # the uncovered tail: eps = 0 there, so the plain entry's bits
            cov = ge.S * ge.patch[0]
            assert torch.equal(out[:, :, cov:], plain[:, :, cov:])


# ------------------------------------------------------------------------------------------------- bit identities
@pytest.mark.parametrize("shape,patch", [GEOMS[0], GEOMS[1], GEOMS[3], GEOMS[5]])
def test_a_constant_table_is_the_existing_slot_entry(dev, shape, patch):
    from multimodal_diffusion_amd import functional as Fn
    ge = Geom(shape, patch)
    B, S = ge.B, ge.S
    z, eps2, tl, tn, tp, _ = ge.inputs(dev, seed=1)
    h0 = torch.randn(ge.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    known = torch.randn((shape[1], 3 * ge.shape[2]) + tuple(shape[3:]), generator=torch.Generator().manual_seed(9)).to(dev)
    mask = torch.rand(known.shape, generator=torch.Generator().manual_seed(10)).to(dev)
    key = Fn.slot_key(SEED, 1, S)
    guide = Fn.clip_guide(known, mask, GSEED, 1, S, None, ge.shape)
    for gtab in (torch.full((T,), GS), None):                   # a table of the scalar, and no table at all
        for eta, dpm in UPDATES:
            for gd in (None, guide):
                ctl = Ctl(dev, "table", B, S, ge.per_slot, gtab=gtab)
                ha, hb = (h0.clone(), h0.clone()) if dpm else (None, None)
                kw = dict(eta=eta, key=key if eta > 0 else None, guide=gd, tl=tl if dpm else None)
                out = ge.run(dev, ge.shape, ge.patch, z, eps2, tn, tp, ctl.c, hist=ha, **kw)
                ref = ge.run(dev, ge.shape, ge.patch, z, eps2, tn, tp, None, hist=hb, **kw)
                assert torch.equal(out, ref), (eta, dpm, gd is not None)
                if dpm:
                    assert torch.equal(ha, hb)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape,patch", [GEOMS[0], GEOMS[2], GEOMS[3]])
def test_rows_and_gather_forms_agree(dev, shape, patch, mode):
    from multimodal_diffusion_amd import functional as Fn
    ge = Geom(shape, patch)
    z, eps2, tl, tn, tp, _ = ge.inputs(dev, seed=2)
    h0 = torch.randn(ge.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    key = Fn.slot_key(SEED, 0, ge.S)
    for eta, dpm in UPDATES:
        got = []
        for rows in (1, 0):
            with tuned(cfg_rows=rows):
                ctl = Ctl(dev, mode, ge.B, ge.S, ge.per_slot)
                h = h0.clone() if dpm else None
                out = _video(dev, ge.shape, ge.patch, z, eps2, tn, tp, ctl.c, eta=eta, key=key if eta > 0 else None, tl=tl if dpm else None,
                             hist=h)
                got.append((out, h, None if mode == "table" else ctl.coef()))
        assert torch.equal(got[0][0], got[1][0])
        if dpm:
            assert torch.equal(got[0][1], got[1][1])
        if mode != "table":
            assert np.array_equal(got[0][2], got[1][2])


@pytest.mark.parametrize("mode", ["rescale", "apg"])
@pytest.mark.parametrize("shape,patch", [GEOMS[0], GEOMS[1], GEOMS[4]])
def test_a_slot_gives_the_same_bits_wherever_it_sits(dev, shape, patch, mode):
    """copy one slot's eps tokens, z and pair into another (b, s) of a batch of 3: its coefficients and its output are bit-equal"""
    ge = Geom(shape, patch)
    assert ge.B == 2
    z, eps2, _, tn, tp, const = ge.inputs(dev, seed=3)
    step = [(b, s) for b in range(2) for s in range(ge.S) if tn[b, s] != tp[b, s] and (b, s) != const]
    bs, ss = step[0]
    z3, eps3, _, tn3, tp3, _ = ge.inputs(dev, seed=4, B=3)
    bd, sd = 2, (ss + 1) % ge.S                                                   # another sample, another slot index
    per, sl = ge.Nt // ge.S, ge.slot_len
    for half_src, half_dst in ((0, 0), (2, 3)):                                   # cond and null rows of the stacked eps
        eps3[half_dst + bd, sd * per:(sd + 1) * per] = eps2[half_src + bs, ss * per:(ss + 1) * per]
    z3[bd, :, sd * sl:(sd + 1) * sl] = z[bs, :, ss * sl:(ss + 1) * sl]
    tn3[bd, sd], tp3[bd, sd] = tn[bs, ss], tp[bs, ss]
    shape3 = (3,) + ge.shape[1:]
    c2, c3 = Ctl(dev, mode, 2, ge.S, ge.per_slot), Ctl(dev, mode, 3, ge.S, ge.per_slot)
    out2 = ge.run(dev, ge.shape, ge.patch, z, eps2, tn, tp, c2.c)
    out3 = ge.run(dev, shape3, ge.patch, z3, eps3, tn3, tp3, c3.c)
    assert np.array_equal(c2.coef()[bs, ss], c3.coef()[bd, sd]) and np.isfinite(c2.coef()[bs, ss]).all()
    assert torch.equal(out2[bs, :, ss * sl:(ss + 1) * sl], out3[bd, :, sd * sl:(sd + 1) * sl])


# ------------------------------------------------------------------------------------------------- S = 1: the per-sample controlled step
def _s1_case(dev, target):
    g = torch.Generator().manual_seed(31)
    if target == "video":
        return torch.randn(2, 8, 2, 16, 32, generator=g).to(dev), torch.randn(2, 8, 40, generator=g).to(dev), 10
    return torch.randn(2, 8, 4, generator=g).to(dev), torch.randn(2, 8, 4, 8, 8, generator=g).to(dev), 8


@pytest.mark.parametrize("mode", ["rescale", "apg"])
@pytest.mark.parametrize("kw", [{}, dict(solver="dpmpp_2m"), dict(eta=0.7, noise_seed=5)], ids=["ddim", "dpmpp_2m", "seeded"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_one_slot_per_sample_is_the_per_sample_controlled_step(dev, model, target, kw, mode):
    """At S = 1 the slot is the sample: ``step_slots`` under ``set_slot_cfg`` is ``step`` with g_b = g(t_b), phi_b = phi(t_b) (or
    ``set_apg``), bit for bit, x0_hist included.  At eta > 0 the two draw their step noise from differently keyed streams by contract
    ("clip-keyed slot noise" has a domain word of its own), so no output of ``step`` can equal the slot step's; there the per-sample
    step's coefficients are compared bit for bit, and the output against the elementwise per-sample path fed those coefficients and the
    slot step's normals (``slot_noise``), bit for bit as well."""
    from multimodal_diffusion_amd import functional as Fn
    z, zp, npr = _s1_case(dev, target)
    B = 2
    tn, tp = torch.tensor([[981], [402]]), torch.tensor([[961], [382]])
    tl = torch.tensor([[999], [-1]])
    dpm, seeded = kw.get("solver") == "dpmpp_2m", "eta" in kw
    g_b, phi_b = GTAB[tn[:, 0]].tolist(), PTAB[tn[:, 0]].tolist()
    h0 = torch.randn(z.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    a = engine(model[1], target, tuple(z.shape), npr, guidance=GS, **kw)          # slots
    b = engine(model[1], target, tuple(z.shape), npr, guidance=GS, **kw)          # per sample
    assert a.slots == 1
    for e in (a, b):
        e.set_prompt(zp)
        if dpm:
            e.x0_hist.copy_(h0)
    if mode == "rescale":
        a.set_slot_cfg(guidance=GTAB, rescale=PTAB)
        b.set_cfg(guidance=g_b, rescale=phi_b)
    else:
        a.set_slot_cfg(guidance=GTAB, apg={"norm_threshold": APG[0], "eta_parallel": APG[1]})
        b.set_cfg(guidance=g_b)
        b.set_apg(*APG)
    out = a.step_slots(z, tn, tp, t_last=tl if dpm else None, clip_first=4 if seeded else None)
    ref = b.step(z, tn[:, 0].to(dev), tp[:, 0].to(dev), t_last=tl[:, 0].to(dev) if dpm else None)
    coef = a.slot_cfg_coef()[:, 0]
    if mode == "rescale":
        s_b = b._cfg_stats[b._cfg_stats.numel() - 16:].view(torch.float32)[:B]
        assert torch.equal(coef[:, 0], s_b)
        assert torch.equal(coef[:, 1:3].cpu(), torch.tensor([g_b, phi_b]).T.contiguous())
    else:
        assert torch.equal(coef, b._apg_stats[b._apg_stats.numel() - 16 * B:].view(torch.float32).view(B, 4))
    assert torch.isfinite(out).all()
    if not seeded:
        assert torch.equal(out, ref)
        if dpm:
            assert torch.equal(a.x0_hist, b.x0_hist)
        return
    ep = a.eps_tokens()
    assert torch.equal(ep, b.eps_tokens())                      # one model evaluation: the uniform table embeds as the per-sample step
    c, u = ep[:B], ep[B:]
    if mode == "rescale":                                       # separate torch kernels: one rounding per operation, as the contract's r(y)
        gt, ph, s = (v.view(B, 1, 1) for v in (coef[:, 1], coef[:, 2], coef[:, 0]))
        y = u + gt * (c - u)
        e = ph * (y * s) + (1.0 - ph) * y
    else:
        e = c + coef[:, 2].view(B, 1, 1) * ((c - u) - coef[:, 1].view(B, 1, 1) * c)
    ge = Geom(tuple(z.shape), a.tube if target == "video" else a.chunk)
    noise = Fn.slot_noise(5, tn, tuple(z.shape), a.slot_len, first=4)
    comp = Fn.ddim_step(z, tn[:, 0].to(dev), tp[:, 0].to(dev), ge.untok(e), ABAR, eta=0.7, noise=noise)
    assert torch.equal(out, comp), float((out - comp).abs().max())
    assert not torch.equal(out, ref)


# ------------------------------------------------------------------------------------------------- the whole step, S > 1
SOLVERS = [{}, dict(eta=0.7, noise_seed=5), dict(solver="dpmpp_2m")]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kw", SOLVERS, ids=["ddim", "seeded", "dpmpp_2m"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_whole_step_equals_the_composed_path(dev, model, target, kw, mode):
    """fused against eps_tokens -> the mirror -> the functional slot update -> functional.clip_guide_slots, within 1e-6, with and
    without the clip guide"""
    from multimodal_diffusion_amd import functional as Fn
    z, zp, npr, _ = case(dev, target)
    eng = engine(model[1], target, tuple(z.shape), npr, guidance=GS, **kw)
    eng.set_prompt(zp)
    B, S, sl = z.shape[0], eng.slots, eng.slot_len
    ge = Geom(tuple(z.shape), eng.tube if target == "video" else eng.chunk)
    assert S > 1 and ge.S == S
    dpm, eta = kw.get("solver") == "dpmpp_2m", kw.get("eta", 0.0)
    tn, tp = SR.tables(B, S, seed=S + B)
    sc = SR.SCHED
    tl = torch.tensor([[sc[sc.index(int(a)) - 1] if sc.index(int(a)) > 0 else -1 for a in row] for row in tn])
    h0 = torch.randn(z.shape, generator=torch.Generator().manual_seed(7)).to(dev)
    known = torch.randn((z.shape[1], 2 * z.shape[2]) + tuple(z.shape[3:]), generator=torch.Generator().manual_seed(9)).to(dev)
    mask = torch.rand(known.shape, generator=torch.Generator().manual_seed(10))
    apg = {"norm_threshold": APG[0], "eta_parallel": APG[1]}
    eng.set_slot_cfg(guidance=GTAB, rescale=PTAB if mode == "rescale" else None, apg=apg if mode == "apg" else None)
    first = 1
    held = (SR.per_position(tn, z.shape[2], sl, z) == SR.per_position(tp, z.shape[2], sl, z)).expand_as(z).to(dev)
    for guided in (False, True):
        if guided:
            eng.set_clip_guide(known, mask, guide_seed=GSEED)
        if dpm:
            eng.x0_hist.copy_(h0)
        need_first = guided or eta > 0
        out = eng.step_slots(z, tn, tp, t_last=tl if dpm else None, clip_first=first if need_first else None).clone()
        hist = eng.x0_hist.clone() if dpm else None
        ep = eng.eps_tokens().cpu().numpy()
        e_tok, _ = SC.control(ep[:B], ep[B:], tn.numpy(), tp.numpy(), GS, T, GTAB.numpy(), PTAB.numpy() if mode == "rescale" else None,
                              APG if mode == "apg" else None)
        e = ge.untok(torch.from_numpy(e_tok).to(dev))
        noise = Fn.slot_noise(5, tn, tuple(z.shape), sl, first=first) if eta > 0 else None
        if dpm:
            h = h0.clone()
            ref = Fn.dpmpp_2m_step_slots(z, e, h, tl, tn, tp, ABAR, sl)
            assert rel(hist, h) <= 1e-6 and torch.equal(hist[held], h0[held])
        else:
            ref = Fn.ddim_step_slots(z, tn, tp, e, ABAR, sl, eta, noise)
        if guided:
            tau = torch.where(tn == tp, torch.full_like(tp, Fn.SLOT_LEAVE), tp)
            ref = Fn.clip_guide_slots(known, tau, ABAR, ref, mask.to(dev), slot_len=sl, seed=GSEED, first=first)
        err = rel(out, ref)
        print(f"{target} {kw} {mode} guided {guided}: rel err {err:.3e}")
        assert torch.isfinite(out).all() and err <= 1e-6
        assert torch.equal(out[held], z[held])
    # the control did something: the plain guided slot step differs
    eng.clear_slot_cfg()
    if dpm:
        eng.x0_hist.copy_(h0)
    assert not torch.equal(eng.step_slots(z, tn, tp, t_last=tl if dpm else None, clip_first=first), out)


# ------------------------------------------------------------------------------------------------- fifo_denoise
SCHED4 = torch.tensor([999, 749, 499, 249, -1])
K = 3


def _queue(dev, mods, **kw):
    """the kit queue: video B = 2, S = 2, under an audio prompt of 20 frames per target slot"""
    g = torch.Generator().manual_seed(17)
    return engine(mods, "video", (2, 8, 4, 16, 16), 10, guidance=GS, **kw), torch.randn(8, 150, generator=g).to(dev), 20


def _plain_loop(eng, canvas_p, hop, sched, n_slots, seed):
    """fifo_denoise restated from step_slots and fifo_shift (the engine's slot control, when set, acts through step_slots)"""
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
    for r in range(n - 1):
        z = eng.step_slots(z, rn[r], rp[r], t_last=rl[r] if dpm else None)
    done = []
    for m in range(n_slots):
        eng.set_prompt(fifo_prompt_windows(canvas_p, m, B, S, hop, Lp))
        z = eng.step_slots(z, sn, sp, t_last=last)
        z, popped = eng.fifo_shift(z, n + m, s0, seed=seed)
        done.append(popped)
    return torch.cat(done, 1)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_fifo_denoise_under_the_control_eager_graph_and_loop(dev, model, solver):
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import schedule_utils as su
    eng, canvas_p, hop = _queue(dev, model[1], solver=solver)
    gtab = su.guidance_interval_table(5.0, (200, 800), T)
    assert float(gtab[999]) == 1.0 and float(gtab[749]) == float(gtab[249]) == 5.0          # the schedule crosses the interval's ends
    kw = dict(guidance_by_level=gtab, rescale_by_level=0.7)
    plain = A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, QSEED)
    eager = A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, QSEED, **kw)
    assert eng._scfg is None                                    # set for the call only
    assert torch.isfinite(eager).all() and not torch.equal(eager, plain)
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, QSEED, graph=True, **kw), eager)
    assert eng._scfg is None
    eng.set_slot_cfg(guidance=gtab, rescale=0.7)
    ref = _plain_loop(eng, canvas_p, hop, SCHED4, K, QSEED)
    eng.clear_slot_cfg()
    assert torch.equal(eager, ref), float((eager - ref).abs().max())
    # APG rides through the same drivers
    akw = dict(guidance_by_level=gtab, apg={"norm_threshold": 20.0, "eta_parallel": 0.5})
    a_eager = A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, QSEED, **akw)
    assert torch.isfinite(a_eager).all() and not torch.equal(a_eager, plain) and not torch.equal(a_eager, eager)
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, QSEED, graph=True, **akw), a_eager)
    # a constant table, phi = 0 and no APG: the bits of the call without the new arguments (and no statistics pass: no scratch)
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, QSEED, guidance_by_level=GS, rescale_by_level=0.0), plain)
    assert torch.equal(A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, QSEED, graph=True, guidance_by_level=lambda t: GS), plain)
    assert eng._scfg is None and eng._scfg_stats is not None


def test_fifo_lookahead_under_the_control_equals_its_loop(dev, model):
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import functional as Fn, schedule_utils as su
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_len
    eng, canvas_p, hop = _queue(dev, model[1])
    sched = torch.tensor([999, 499, -1])                         # lookahead = 1 of S = 2: h = 1, n = B * h = 2 steps
    gtab = su.guidance_interval_table(5.0, (200, 800), T)
    kw = dict(guidance_by_level=gtab, rescale_by_level=0.7)
    out = A.fifo_denoise(eng, canvas_p, hop, sched, K, QSEED, lookahead=1, **kw)
    assert eng._scfg is None and torch.isfinite(out).all()
    assert not torch.equal(out, A.fifo_denoise(eng, canvas_p, hop, sched, K, QSEED, lookahead=1))
    shape = eng.latent_shape

    def noise(p0, n_pos):
        return Fn.canvas_noise(QSEED, torch.tensor([999]), (1, shape[1], n_pos) + tuple(shape[3:]), 1, window_offset=p0)[0]

    eng.set_slot_cfg(guidance=gtab, rescale=0.7)
    ref = LR.loop(eng, canvas_p, hop, fifo_prompt_len(eng, canvas_p), sched.tolist(), K, 1, noise)
    eng.clear_slot_cfg()
    assert torch.equal(out, ref), float((out - ref).abs().max())


def test_fifo_denoise_control_with_init_canvas_and_cleanup(dev, model):
    import multimodal_diffusion_amd as A
    eng, canvas_p, hop = _queue(dev, model[1], eta=0.5, noise_seed=11)
    sl = eng.slot_len
    known = torch.randn((8, K * sl, 16, 16), generator=torch.Generator().manual_seed(3)).to(dev)
    kw = dict(guidance_by_level=lambda t: 1.0 + 4.0 * t / T, rescale_by_level=0.7)
    out = A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, QSEED, init_canvas=known, guide_seed=GSEED, **kw)      # a full mask
    assert torch.equal(out, known)                              # the held region leaves equal to the canvas, bit for bit
    assert eng._scfg is None and eng._clip is None
    from multimodal_diffusion_amd.sampler import canvas_frame_mask
    mask = canvas_frame_mask(tuple(known.shape), sl, 2 * sl)
    part = A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, QSEED, init_canvas=known, mask=mask, guide_seed=GSEED, **kw)
    base = A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, QSEED, init_canvas=known, mask=mask, guide_seed=GSEED)
    assert torch.equal(part[:, sl:2 * sl], known[:, sl:2 * sl]) and torch.isfinite(part).all()
    assert not torch.equal(part[:, 2 * sl:], base[:, 2 * sl:])
    # cleared when the call raises as well: a schedule that does not fit the queue is found after the control's own checks
    with pytest.raises(ValueError, match="queue"):
        A.fifo_denoise(eng, canvas_p, hop, torch.tensor([999, 499, -1]), K, QSEED, **kw)
    assert eng._scfg is None
    eng.set_cfg(rescale=0.5)                                    # step_slots refuses it: raised inside the drivers, with the control set
    for extra in (dict(), dict(graph=True), dict(init_canvas=known, guide_seed=GSEED)):
        with pytest.raises(ValueError, match="step_slots takes the scalar guidance"):
            A.fifo_denoise(eng, canvas_p, hop, SCHED4, K, QSEED, **kw, **extra)
        assert eng._scfg is None and eng._clip is None
    eng.set_cfg(rescale=0.0)


# ------------------------------------------------------------------------------------------------- misuse
def test_misuse_is_refused_with_out_untouched(dev, model):
    L, lib = _lib()
    ge = Geom(*GEOMS[0])
    z, eps2, _, tn, tp, _ = ge.inputs(dev, seed=5)
    out = torch.full(ge.shape, 7.0, device=dev)
    ab = ABAR.to(dev)

    def call(cfg, out_t=out):
        return lib.avd_cfg_unpatch_ddim_slots_cfg_f32(eps2.data_ptr(), z.data_ptr(), None, tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), T, GS,
                                                      0.0, None, None, ge.S, None, out_t.data_ptr(), *ge.shape, *ge.patch, C.byref(cfg),
                                                      L.stream_ptr(dev))

    both = Ctl(dev, "rescale", ge.B, ge.S, ge.per_slot)
    both.c.apg = 1
    assert call(both.c) == L.EINVAL and b"together with APG" in lib.avd_last_error()
    short = Ctl(dev, "apg", ge.B, ge.S, ge.per_slot)
    short.c.stats_bytes -= 16
    assert call(short.c) == L.EINVAL and b"needed" in lib.avd_last_error()
    off = Ctl(dev, "rescale", ge.B, ge.S, ge.per_slot, pad=16)
    off.c.stats += 4
    assert call(off.c) == L.EUNSUPPORTED and b"16-byte aligned" in lib.avd_last_error()
    over = Ctl(dev, "apg", ge.B, ge.S, ge.per_slot)
    for t in (out, z, eps2):
        over.c.stats = t.data_ptr() + 64
        assert call(over.c) == L.EINVAL and b"must not overlap" in lib.avd_last_error()
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    # the engine: APG with momentum, APG with rescale, step / run with a slot control set
    zz, zp, npr, _ = case(dev, "video")
    eng = engine(model[1], "video", tuple(zz.shape), npr, guidance=GS)
    eng.set_prompt(zp)
    with pytest.raises(ValueError, match="no momentum"):
        eng.set_slot_cfg(apg={"norm_threshold": 1.0, "momentum": -0.5})
    with pytest.raises(ValueError, match="cannot be combined with guidance_rescale"):
        eng.set_slot_cfg(rescale=0.5, apg={"norm_threshold": 1.0})
    assert eng._scfg is None
    eng.set_slot_cfg(rescale=0.5)
    o2 = torch.full_like(zz, 7.0)
    t1 = torch.tensor([500, 500], device=dev)
    with pytest.raises(ValueError, match="step takes no slot CFG control"):
        eng.step(zz, t1, t1 - 50, out=o2)
    with pytest.raises(ValueError, match="run takes no slot CFG control"):
        eng.run(zz, SCHED4)
    torch.cuda.synchronize()
    assert bool((o2 == 7.0).all())
    # and the per-sample controls stay refused by step_slots, in the words they had
    eng.clear_slot_cfg()
    eng.set_cfg(rescale=0.5)
    with pytest.raises(ValueError, match="step_slots takes the scalar guidance"):
        eng.step_slots(zz, torch.full((2, eng.slots), 500), torch.full((2, eng.slots), 450))
