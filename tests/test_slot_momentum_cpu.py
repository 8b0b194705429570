"""Slot APG momentum on the host (include/avdiff_hip.h, "slot APG momentum"): ``functional.fifo_carry`` against an index-by-index
loop, the torch slot APG reference with momentum against the contract written out by hand and against the numpy mirror, and the host
refusals of ``set_slot_cfg`` / ``fifo_denoise`` / ``stream_generate(sampler="fifo")``."""
import ctypes as C
import inspect
import math
import pathlib

import numpy as np
import pytest
import torch

import _apg_ref as AR
from _kit import pipeline_cfg
from test_slot_cfg_cpu import _bare_engine

ROOT = pathlib.Path(__file__).resolve().parents[1]
STREAM_ONE_SECOND = {"window_seconds": 1.0, "hop_seconds": 0.5, "crossfade_seconds": 0.25}
CARRY_CASES = [(1, 1, 0), (2, 3, 0), (3, 4, 2), (2, 2, 1)]          # (B, S, ctx)


def carry_loop(buf, S, sl, ctx, shift):
    """the contract, one element at a time: window b position s >= ctx takes the owner copy of logical slot b*h + s + shift"""
    B, outer = buf.shape[:2]
    v = buf.reshape(B, outer, S * sl, -1)
    out = torch.full_like(v, float("nan"))
    h = S - ctx
    Q = ctx + B * h
    for b in range(B):
        for s in range(S):
            q = b * h + s + shift
            for j in range(sl):
                if s < ctx or q >= Q:
                    out[b, :, s * sl + j] = 0.0
                else:
                    bs, ss = (q - ctx) // h, ctx + (q - ctx) % h
                    out[b, :, s * sl + j] = v[bs, :, ss * sl + j]
    return out.reshape(buf.shape)


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("B,S,ctx", CARRY_CASES)
@pytest.mark.parametrize("tail", [(3, 4), ()], ids=["video", "audio"])
def test_fifo_carry_is_the_index_loop(B, S, ctx, shift, tail):
    from multimodal_diffusion_amd import functional as Fn
    sl = 2
    buf = torch.randn((B, 3, S * sl) + tail, generator=torch.Generator().manual_seed(B * 16 + S * 4 + ctx))
    keep = buf.clone()
    out = Fn.fifo_carry(buf, S, sl, ctx=ctx, shift=shift)
    assert torch.equal(out, carry_loop(buf, S, sl, ctx, shift)) and torch.equal(buf, keep)
    v = out.reshape(B, 3, S, -1)
    assert not v[:, :, :ctx].any()                                  # every context position
    if shift:
        assert not v[B - 1, :, S - 1].any()                          # the entering tail slot
        if B * (S - ctx) > 1:
            assert out.any()
    else:                                                            # nothing moves: the stepping positions as they were
        assert torch.equal(v[:, :, ctx:], buf.reshape(B, 3, S, -1)[:, :, ctx:])
    into = torch.full_like(buf, 7.0)
    assert Fn.fifo_carry(buf, S, sl, ctx=ctx, shift=shift, out=into) is into and torch.equal(into, out)


def test_fifo_carry_at_ctx_0_shift_1_is_the_shift_of_the_history():
    """queue slot q of the result is queue slot q + 1 of the input across sample boundaries, zeros in the tail"""
    from multimodal_diffusion_amd import functional as Fn
    B, S, sl = 3, 2, 2
    buf = torch.randn(B, 4, S * sl, 5, 2, generator=torch.Generator().manual_seed(1))
    out = Fn.fifo_carry(buf, S, sl)
    slots = lambda t: t.reshape(B, 4, S, sl, 10).permute(0, 2, 1, 3, 4).reshape(B * S, 4, sl, 10)      # noqa: E731
    assert torch.equal(slots(out)[:-1], slots(buf)[1:]) and not slots(out)[-1].any()


@pytest.mark.parametrize("kw,match", [(dict(slots=3), "sliding length"), (dict(ctx=2), "ctx"), (dict(ctx=-1), "ctx"), (dict(shift=2), "shift"),
                                      (dict(shift=True), "shift"), (dict(slot_len=0), "slot_len")])
def test_fifo_carry_argument_errors(kw, match):
    from multimodal_diffusion_amd import functional as Fn
    args = dict(dict(slots=2, slot_len=2, ctx=0, shift=1), **kw)
    with pytest.raises(ValueError, match=match):
        Fn.fifo_carry(torch.zeros(2, 3, 4), **args)
    with pytest.raises(ValueError, match="float32"):
        Fn.fifo_carry(torch.zeros(2, 3, 4, dtype=torch.float64), 2, 2)


# ------------------------------------------------------------------------------------------------- the reference
def _slots(n=3, per=96, seed=0):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn(n, per, generator=g)
    return c, 0.2 * c + 0.5 * torch.randn(n, per, generator=g)


def _by_hand(c, u, g, r, eta_p, beta, m):
    """the contract's items 2, 4 and 5 for one slot, in numpy: d in fp32, moments in fp64, coefficients rounded once, e in fp32"""
    F = np.float32
    c, u = c.numpy(), u.numpy()
    d = (c - u) + F(beta) * m.numpy() if beta != 0.0 else c - u
    sdd, sdc, scc = (np.sum(np.float64(a) * np.float64(b)) for a, b in ((d, d), (d, c), (c, c)))
    s = F(min(1.0, float(F(r)) / math.sqrt(sdd))) if r != 0.0 and sdd != 0.0 else F(1.0)
    k = F((1.0 - float(F(eta_p))) * sdc / scc)
    w = F((F(g) - F(1.0)) * s)
    return (c + w * (d - k * c)).astype(F), d.astype(F)


def test_two_chained_steps_equal_the_formula_by_hand():
    from multimodal_diffusion_amd import functional as Fn
    n, beta, r, eta_p = 3, -0.5, 4.0, 0.25
    g = [2.0, 3.5, 6.0]
    c1, u1 = _slots(n, seed=1)
    c2, u2 = _slots(n, seed=2)
    m0 = torch.randn(n, 96, generator=torch.Generator().manual_seed(3))
    e1, d1 = Fn.slot_apg_reference(c1, u1, g, r, eta_p, momentum=beta, m_prev=m0)
    e2, d2 = Fn.slot_apg_reference(c2, u2, g, r, eta_p, momentum=beta, m_prev=d1)
    assert e1.dtype == d1.dtype == torch.float32
    capped = 0
    for i in range(n):
        h1, hd1 = _by_hand(c1[i], u1[i], g[i], r, eta_p, beta, m0[i])
        h2, hd2 = _by_hand(c2[i], u2[i], g[i], r, eta_p, beta, torch.from_numpy(hd1))
        assert np.array_equal(d1[i].numpy(), hd1) and np.array_equal(d2[i].numpy(), hd2)
        assert np.array_equal(e1[i].numpy(), h1) and np.array_equal(e2[i].numpy(), h2)
        capped += float(np.linalg.norm(hd2)) > r
    assert capped                                                    # r caps some slot: the norm of the accumulated d is what it sees
    assert not torch.equal(d2, c2 - u2)


def test_beta_0_is_the_existing_mirror_and_a_zero_buffer_is_the_first_step():
    from multimodal_diffusion_amd import functional as Fn
    c, u = _slots(4, seed=5)
    g = np.array([1.0, 2.5, 4.0, 7.0], np.float32)
    e0, d0 = Fn.slot_apg_reference(c, u, g, 3.0, 0.5)
    e_ref, d_ref, _ = AR.apg(c.numpy(), u.numpy(), g, 3.0, 0.5)
    assert np.array_equal(e0.numpy(), e_ref) and np.array_equal(d0.numpy(), d_ref)
    e_m, d_m, _ = AR.apg(c.numpy(), u.numpy(), g, 3.0, 0.5, -0.75, d0.numpy())
    e1, d1 = Fn.slot_apg_reference(c, u, g, 3.0, 0.5, momentum=-0.75, m_prev=d0)
    assert np.array_equal(e1.numpy(), e_m) and np.array_equal(d1.numpy(), d_m)
    with pytest.raises(ValueError, match="m_prev goes with momentum"):
        Fn.slot_apg_reference(c, u, g, 3.0, 0.5, momentum=-0.5)
    with pytest.raises(ValueError, match="m_prev goes with momentum"):
        Fn.slot_apg_reference(c, u, g, 3.0, 0.5, m_prev=d0)


def test_a_slots_first_step_after_a_carry_is_the_momentum_free_value():
    """a queue of B * S = 4 slots of 2 positions: after the carry the entering slot's momentum is zero, so its step is the step without
    momentum, and the slot that moved up steps on the momentum it brought along"""
    from multimodal_diffusion_amd import functional as Fn
    B, S, sl, Ca = 2, 2, 2, 3
    M = torch.randn(B, Ca, S * sl, generator=torch.Generator().manual_seed(11))
    M2 = Fn.fifo_carry(M, S, sl)
    rows = lambda t: t.reshape(B, Ca, S, sl).permute(0, 2, 1, 3).reshape(B * S, Ca * sl)      # noqa: E731  (one slot per row, (ch, j) order)
    c, u = _slots(B * S, Ca * sl, seed=12)
    e, d = Fn.slot_apg_reference(c, u, 3.5, 2.0, 0.25, momentum=-0.5, m_prev=rows(M2))
    e_free, d_free = Fn.slot_apg_reference(c, u, 3.5, 2.0, 0.25)
    assert torch.equal(e[-1], e_free[-1]) and torch.equal(d[-1], d_free[-1])
    assert torch.equal(rows(M2)[:-1], rows(M)[1:])
    e_moved, _ = Fn.slot_apg_reference(c[:1], u[:1], 3.5, 2.0, 0.25, momentum=-0.5, m_prev=rows(M)[1:2])
    assert torch.equal(e[0], e_moved[0]) and not torch.equal(e[0], e_free[0])


# ------------------------------------------------------------------------------------------------- bindings and refusals
def test_header_and_bindings():
    from multimodal_diffusion_amd import _lib as L
    import multimodal_diffusion_amd as A
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    assert "slot APG momentum" in header and "avd_fifo_carry_f32" in header and hasattr(L.lib(), "avd_fifo_carry_f32")
    assert "which is not built" not in header and "no slot momentum" not in header
    assert "avd_slot_cfg_momentum" in header and "#define AVD_SLOT_APG_MOMENTUM 2" in header and L.SLOT_APG_MOMENTUM == 2
    # avd_slot_cfg keeps its 48 bytes; the momentum struct is that control followed by the two trailing fields (float + pad, pointer)
    assert C.sizeof(L.SlotCfg) == 48 and not hasattr(L.SlotCfg, "momentum") and issubclass(L.SlotCfgMomentum, L.SlotCfg)
    names = ("guidance_t", "rescale_t", "apg", "norm_threshold", "eta_parallel", "stats", "stats_bytes")
    assert [getattr(L.SlotCfgMomentum, f).offset for f in names] == [getattr(L.SlotCfg, f).offset for f in names]
    assert [getattr(L.SlotCfgMomentum, f).offset for f in ("momentum", "momentum_buf")] == [48, 56] and C.sizeof(L.SlotCfgMomentum) == 64
    cfg = L.SlotCfgMomentum(None, None, 2, 2.0, 0.5, None, 0)        # the trailing fields default to zero and NULL
    assert cfg.momentum == 0.0 and not cfg.momentum_buf
    assert "apg_momentum" in inspect.signature(A.DenoiseEngine.set_slot_cfg).parameters
    assert "apg_momentum" in inspect.signature(A.fifo_denoise).parameters
    assert isinstance(A.DenoiseEngine.slot_momentum, property)
    assert L.lib().avd_abi_version() == L.ABI_VERSION == 7           # an addition


APG = {"norm_threshold": 2.0, "eta_parallel": 0.25}
BAD = [(dict(apg_momentum=-0.5), "needs apg"),
       (dict(apg_momentum=-0.5, guidance=3.0), "needs apg"),
       (dict(apg=APG, apg_momentum=float("nan")), "finite"),
       (dict(apg=APG, apg_momentum=float("inf")), "finite"),
       (dict(apg=APG, apg_momentum=True), "number"),
       (dict(apg=dict(APG, momentum=-0.5)), "no momentum.*apg_momentum"),
       (dict(apg=dict(APG, momentum=-0.5), apg_momentum=-0.5), "no momentum.*apg_momentum")]


@pytest.mark.parametrize("kw,match", BAD)
def test_set_slot_cfg_refusals(kw, match):
    eng = _bare_engine()
    with pytest.raises(ValueError, match=match):
        eng.set_slot_cfg(**kw)
    assert eng._scfg is None and eng.slot_momentum is None and eng._smom is None


def test_a_bare_engine_has_no_slot_momentum_and_zero_means_none():
    from multimodal_diffusion_amd import _lib as L
    eng = _bare_engine()
    assert eng.slot_momentum is None and eng._smom_beta == 0.0
    eng.set_slot_cfg(guidance=3.0)                                   # today's call keeps working on the shell
    assert type(eng._scfg) is L.SlotCfg and eng._scfg.apg == 0
    eng.clear_slot_cfg()
    g, phi, apg, nb, beta = eng._check_slot_cfg(None, None, APG, 0.0)
    assert beta == 0.0 and apg == (2.0, 0.25)
    assert eng._check_slot_cfg(None, None, APG, None)[4] == 0.0 and eng._check_slot_cfg(None, None, APG, -0.5)[4] == -0.5


def test_fifo_denoise_checks_apg_momentum_first():
    import multimodal_diffusion_amd as A
    eng = _bare_engine()
    args = (eng, torch.zeros(8, 40), 20, torch.tensor([999, 749, 499, 249, -1]), 0, 1)
    for kw, match in BAD:
        kw = {{"guidance": "guidance_by_level"}.get(k, k): v for k, v in kw.items()}
        for extra in (dict(), dict(graph=True), dict(lookahead=1)):
            with pytest.raises(ValueError, match=match):
                A.fifo_denoise(*args, **kw, **extra)
    assert eng._scfg is None and eng.slot_momentum is None
    with pytest.raises(ValueError, match="n_slots"):                 # valid: the next check is reached, nothing is set
        A.fifo_denoise(*args, apg=APG, apg_momentum=-0.5)
    assert eng._scfg is None and eng._smom is None


def test_fifo_options_take_apg_momentum_and_refuse_the_rest():
    from multimodal_diffusion_amd import stream_infer as S
    cfg = pipeline_cfg(clip_seconds=1.0, sampler_steps=4, streaming=STREAM_ONE_SECOND)
    kw = dict(shard=False, consensus=None, noise_keying=None, resample=None, init_noise=None)
    assert S._fifo_options(cfg, fifo=None, **kw)["apg_momentum"] is None
    assert S._fifo_options(cfg, fifo={"apg_momentum": -0.5}, **kw)["apg_momentum"] == -0.5
    st = dict(cfg, streaming=dict(STREAM_ONE_SECOND, fifo={"apg_momentum": -0.25, "steps": 4}))
    assert S._fifo_options(st, fifo=None, **kw)["apg_momentum"] == -0.25
    assert S._fifo_options(st, fifo={"apg_momentum": 0.5}, **kw)["apg_momentum"] == 0.5          # the argument wins
    for bad, match in (({"apg_momentum": float("nan")}, "finite"), ({"apg_momentum": float("-inf")}, "finite"),
                       ({"apg_momentum": "x"}, "number"), ({"apg_momenta": -0.5}, "steps, lookahead and graph"),
                       ({"momentum": -0.5}, "steps, lookahead and graph")):
        with pytest.raises(ValueError, match=match):
            S._fifo_options(cfg, fifo=bad, **kw)
