"""Slot timesteps on the GPU ("slot timesteps" in include/avdiff_hip.h): the fused update alone, the front end alone and the whole
step, each against the per-sample entry it generalises — bit for bit — and the whole step on mixed tables against the CPU oracle."""
import ctypes as C

import pytest
import torch

import _slot_ref as SR
from _kit import ABAR, audio_case, case, dev, engine, model, ts, video_case  # noqa: F401  (dev, model are fixtures)
from _tune import tuned
from conftest import rel_err

pytestmark = pytest.mark.gpu

GS = 3.5
TOL = 1e-4          # the parity tolerance of test_gpu_parity.py


def _lib():
    from multimodal_diffusion_amd import _lib as L
    return L, L.lib()


# ------------------------------------------------------------------------------------------------- 1. the fused update alone
def _video_update(dev, shape, tube, tn, tp, slots):
    """z_out of the slot form (slots != 0: tn / tp are [B, S]) or of the per-sample entry, on fixed random eps2 / z"""
    L, lib = _lib()
    B, Cc, T, H, W = shape
    g = torch.Generator().manual_seed(sum(shape) + tube[0])
    z = torch.randn(shape, generator=g).to(dev)
    eps2 = torch.randn(2 * B, z[0].numel(), generator=g).to(dev)           # [2B, Nt * D]
    out = torch.full(shape, float("nan"), device=dev)
    ab = ABAR.to(dev)
    head = (eps2.data_ptr(), z.data_ptr(), tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), 1000, GS)
    dims = (B, Cc, T, H, W, *tube, L.stream_ptr(dev))
    if slots:
        L.check(lib.avd_cfg_unpatch_ddim_slots_f32(*head, slots, out.data_ptr(), *dims))
    else:
        L.check(lib.avd_cfg_unpatch_ddim_f32(*head, 0.0, None, out.data_ptr(), *dims))
    return z, out


# W = 32 / 16 / 8: the 8-token and the 4-token whole-line forms and the gather form; tube t = 1: S = T; B = 1 and 3
VIDEO_CASES = [((2, 8, 4, 16, 32), (2, 4, 4)), ((2, 8, 4, 16, 16), (2, 4, 4)), ((2, 8, 4, 16, 8), (2, 4, 4)),
               ((2, 8, 4, 16, 32), (1, 4, 4)), ((1, 8, 4, 16, 32), (2, 4, 4)), ((3, 8, 4, 16, 16), (2, 4, 4))]


@pytest.mark.parametrize("shape,tube", VIDEO_CASES)
def test_video_update_equals_per_sample_entry_per_pair(dev, shape, tube):
    B, S = shape[0], shape[2] // tube[0]
    tn, tp = (t.to(dev) for t in SR.tables(B, S, seed=S * 8 + B))
    z, out = _video_update(dev, shape, tube, tn, tp, S)
    ref = SR.by_pairs(lambda a, p: _video_update(dev, shape, tube, a, p, 0)[1], z, tn, tp, tube[0])
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref), float((out - ref).abs().max())
    hold = SR.per_position(tn, shape[2], tube[0], z) == SR.per_position(tp, shape[2], tube[0], z)
    assert hold.any() and torch.equal(out[hold.expand_as(z)], z[hold.expand_as(z)])
    assert not torch.equal(out, z)


@pytest.mark.parametrize("shape,tube", VIDEO_CASES[:2])
def test_video_update_gather_and_row_forms_agree(dev, shape, tube):
    B, S = shape[0], shape[2] // tube[0]
    tn, tp = (t.to(dev) for t in SR.tables(B, S, seed=5))
    with tuned(cfg_rows=1):
        _, rows = _video_update(dev, shape, tube, tn, tp, S)
    with tuned(cfg_rows=0):
        _, gather = _video_update(dev, shape, tube, tn, tp, S)
    assert torch.isfinite(rows).all() and torch.equal(rows, gather)


def _audio_update(dev, shape, chunk, tn, tp, slots):
    L, lib = _lib()
    B, Ca, F = shape
    na = (F - chunk[0]) // chunk[1] + 1
    g = torch.Generator().manual_seed(F)
    z = torch.randn(shape, generator=g).to(dev)
    eps2 = torch.randn(2 * B, na, Ca * chunk[0], generator=g).to(dev)
    out = torch.full(shape, float("nan"), device=dev)
    ab = ABAR.to(dev)
    head = (eps2.data_ptr(), z.data_ptr(), tn.data_ptr(), tp.data_ptr(), ab.data_ptr(), 1000, GS)
    dims = (B, Ca, F, *chunk, L.stream_ptr(dev))
    if slots:
        L.check(lib.avd_cfg_untoken_ddim_audio_slots_f32(*head, slots, out.data_ptr(), *dims))
    else:
        L.check(lib.avd_cfg_untoken_ddim_audio_f32(*head, 0.0, None, out.data_ptr(), *dims))
    return z, out


@pytest.mark.parametrize("F", [40, 42])          # 42: two uncovered frames, which follow the last slot with eps = 0
def test_audio_update_equals_per_sample_entry_per_pair(dev, F):
    shape, chunk, S = (2, 8, F), (4, 4), 10
    tn, tp = (t.to(dev) for t in SR.tables(2, S, seed=F))
    z, out = _audio_update(dev, shape, chunk, tn, tp, S)
    ref = SR.by_pairs(lambda a, p: _audio_update(dev, shape, chunk, a, p, 0)[1], z, tn, tp, 4)
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref), float((out - ref).abs().max())
    hold = (SR.per_position(tn, F, 4, z) == SR.per_position(tp, F, 4, z)).expand_as(z)
    assert hold.any() and torch.equal(out[hold], z[hold])


def test_audio_update_refuses_overlapping_chunks(dev):
    L, _ = _lib()
    tn, tp = (t.to(dev) for t in SR.tables(2, 19, seed=1))
    with pytest.raises(L.AvdError, match="non-overlapping"):
        _audio_update(dev, (2, 8, 40), (4, 2), tn, tp, 19)


def test_functional_mirror_equals_fused_update(dev):
    """functional.ddim_step_slots on the un-patched CFG eps is the fused slot update, bit for bit"""
    from multimodal_diffusion_amd import functional as Fn
    shape, tube = (2, 8, 4, 16, 32), (2, 4, 4)
    tn, tp = (t.to(dev) for t in SR.tables(2, 2, seed=3))
    z, out = _video_update(dev, shape, tube, tn, tp, 2)
    g = torch.Generator().manual_seed(sum(shape) + tube[0])
    torch.randn(shape, generator=g)
    eps2 = torch.randn(4, 64, 256, generator=g).to(dev)
    # the combine of the kernel, without contraction: two roundings, as torch's separate ops
    eps_tok = eps2[2:] + GS * (eps2[:2] - eps2[2:])
    eps_lat = Fn.tube_unpatch(eps_tok, 8, 4, 16, 32, *tube)
    assert torch.equal(Fn.ddim_step_slots(z, tn, tp, eps_lat, ABAR, 2), out)


# ------------------------------------------------------------------------------------------------- 2. the front end
@pytest.mark.parametrize("target", ["video", "audio"])
def test_front_end_rows_equal_uniform_timestep_rows(dev, model, target):
    L, lib = _lib()
    z, zp, npr, _ = case(dev, target, B=2)
    eng = engine(model[1], target, tuple(z.shape), npr, guidance=GS)
    Xp = eng.set_prompt(zp)
    e, B, N, d, S = eng.embed, 2, eng.N, eng.d, eng.slots
    tn, _ = (t.to(dev) for t in SR.tables(B, S, seed=11))
    tok = torch.empty(lib.avd_embed_workspace_floats(C.byref(e)), device=dev)
    args = (C.byref(e), z.data_ptr(), eng._aw.data_ptr(), eng._ab.data_ptr())

    def pair(t_uniform):
        X2 = torch.full((2 * B, N, d), float("nan"), device=dev)
        t = torch.full((B,), t_uniform, dtype=torch.long, device=dev)
        L.check(lib.avd_embed_cfg_pair_f32(*args, t.data_ptr(), Xp.data_ptr(), tok.data_ptr(), X2.data_ptr(), L.stream_ptr(dev)))
        return X2

    X2 = torch.full((2 * B, N, d), float("nan"), device=dev)
    L.check(lib.avd_embed_cfg_pair_slots_f32(*args, tn.data_ptr(), S, Xp.data_ptr(), tok.data_ptr(), X2.data_ptr(), L.stream_ptr(dev)))
    assert torch.isfinite(X2).all()
    t0 = 0 if e.target_first else e.Np
    per_slot = e.Nt // S
    refs = {t: pair(t) for t in sorted(set(tn.reshape(-1).tolist()))}
    for b in range(B):
        for s in range(S):
            rows = slice(t0 + s * per_slot, t0 + (s + 1) * per_slot)
            ref = refs[int(tn[b, s])]
            assert torch.equal(X2[b, rows], ref[b, rows]), (b, s)                       # cond half
            assert torch.equal(X2[B + b, rows], ref[B + b, rows]), (b, s)               # null half
    prompt = slice(e.Nt, N) if e.target_first else slice(0, e.Np)
    any_ref = next(iter(refs.values()))
    assert torch.equal(X2[:, prompt], any_ref[:, prompt])
    assert len(refs) > 1 and not torch.equal(X2, any_ref)


# ------------------------------------------------------------------------------------------------- 3. the whole step
def _uniform(t, B, S, dev):
    return torch.tensor(t, dtype=torch.long, device=dev)[:, None].expand(B, S).contiguous()


@pytest.mark.parametrize("split_streams", [False, True])
@pytest.mark.parametrize("matmul", ["f32", "bf16x3"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_uniform_tables_give_the_plain_step(dev, model, target, matmul, split_streams):
    z, zp, npr, _ = case(dev, target, B=2)
    with tuned(s3_min_rows=0):          # these few hundred rows on the split-operand path where bf16x3 is asked for
        eng = engine(model[1], target, tuple(z.shape), npr, guidance=GS, matmul=matmul, split_streams=split_streams)
        eng.set_prompt(zp)
        tn, tp = [981, 402], [961, -1]
        ref = eng.step(z, ts(tn, dev), ts(tp, dev))
        out = eng.step_slots(z, _uniform(tn, 2, eng.slots, dev), _uniform(tp, 2, eng.slots, dev))
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref), float((out - ref).abs().max())


def test_uniform_tables_on_the_default_route_with_the_short_null_layout(dev, model):
    """audio -> video with the engine's defaults: one stream, the null half without its duplicate prompt rows"""
    from multimodal_diffusion_amd import _lib as L
    z, zp, npr = video_case(dev, B=2)
    with tuned(s3_min_rows=0):
        eng = engine(model[1], "video", tuple(z.shape), npr, guidance=GS)
        eng.set_prompt(zp)
        tn, tp = ts([981, 402], dev), ts([961, 382], dev)
        ref = eng.step(z, tn, tp)
        L.prof_enable(True)
        try:
            out = eng.step_slots(z, tn[:, None].expand(2, 2), tp[:, None].expand(2, 2))
            torch.cuda.synchronize()
        finally:
            L.prof_enable(False)
    assert L.prof_report().get("qkv3_replicate_kernel", (0,))[0] == 2          # one per block: the short layout ran
    assert torch.equal(out, ref)


@pytest.mark.parametrize("matmul", ["f32", "bf16x3"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_mixed_tables_against_the_oracle(dev, model, target, matmul):
    ws, mods = model
    z, zp, npr, _ = case(dev, target, B=2)
    with tuned(s3_min_rows=0):
        eng = engine(mods, target, tuple(z.shape), npr, guidance=GS, matmul=matmul)
        eng.set_prompt(zp)
        tn, tp = SR.tables(2, eng.slots, seed=21)
        out = eng.step_slots(z, tn, tp)
    ref = SR.step_slots(ws, target, z.cpu(), zp.cpu(), tn, tp, GS)
    err = rel_err(out.cpu(), ref)
    print(f"slot step vs oracle ({target}, {matmul}): rel err {err:.3e}")
    assert err < TOL
    hold = (SR.per_position(tn, z.shape[2], eng.slot_len, z) == SR.per_position(tp, z.shape[2], eng.slot_len, z)).expand_as(z).to(dev)
    assert hold.any() and torch.equal(out[hold], z[hold])                       # held slots: z, bit for bit
    assert not torch.equal(out[~hold], z[~hold])


def test_slots_and_slot_len(dev, model):
    z, zp, npr = video_case(dev, B=2)
    eng = engine(model[1], "video", tuple(z.shape), npr, guidance=GS)
    assert (eng.slots, eng.slot_len) == (2, 2)
    za, zv, npa = audio_case(dev, B=2, L=42)
    eng = engine(model[1], "audio", tuple(za.shape), npa, guidance=GS)
    assert (eng.slots, eng.slot_len) == (10, 4)


def test_step_slots_refusals_leave_out_untouched(dev, model):
    import multimodal_diffusion_amd as A
    mods = model[1]
    z, zp, npr, known = case(dev, "video", B=2)
    tn, tp = (t.to(dev) for t in SR.tables(2, 2, seed=2))
    out = torch.full_like(z, 7.0)

    def refused(eng, match, exc=ValueError, tn=tn, tp=tp):
        eng.set_prompt(zp)
        with pytest.raises(exc, match=match):
            eng.step_slots(z, tn, tp, out=out)
        torch.cuda.synchronize()
        assert (out == 7.0).all()

    refused(engine(mods, "video", tuple(z.shape), npr, guidance=GS, eta=0.5, noise_seed=1), "eta == 0")
    refused(engine(mods, "video", tuple(z.shape), npr, guidance=GS, solver="dpmpp_2m"), "solver")
    eng = engine(mods, "video", tuple(z.shape), npr, guidance=GS)
    eng.set_known(known)
    refused(eng, "latent guide")
    refused(engine(mods, "video", tuple(z.shape), npr, guidance=[2.0, 3.0]), "CFG control")
    refused(engine(mods, "video", tuple(z.shape), npr, guidance=GS, guidance_rescale=0.5), "CFG control")
    eng = engine(mods, "video", tuple(z.shape), npr, guidance=GS)
    eng.set_window_consensus(2)
    refused(eng, "window consensus")
    core, head = mods[0], mods[1]
    torch.manual_seed(1)
    add = A.DenoiseEngine(core=core, head=head, tstep_dim=256, target="video", latent_shape=tuple(z.shape), prompt_tokens=npr,
                          alpha_bar=ABAR, guidance=GS, temb_mode="add", adapt_v=A.LinearAdapter(256, 512).to(dev),
                          adapt_a=A.LinearAdapter(32, 512).to(dev))
    refused(add, "concat")
    # overlapping audio chunks
    za, zv, npa = audio_case(dev, B=2)
    oa = torch.full_like(za, 7.0)
    eng = engine(mods, "audio", tuple(za.shape), npa, guidance=GS, chunk=(4, 2))
    eng.set_prompt(zv)
    t19 = [t.to(dev) for t in SR.tables(2, 19, seed=4)]
    with pytest.raises(ValueError, match="non-overlapping"):
        eng.step_slots(za, *t19, out=oa)
    assert (oa == 7.0).all()
    # the tables: shape, dtype
    eng = engine(mods, "video", tuple(z.shape), npr, guidance=GS)
    refused(eng, r"\[B, S\]", tn=tn[:, :1], tp=tp[:, :1])
    refused(eng, "integer", exc=TypeError, tn=tn.float(), tp=tp)
    # and the same engine steps once the tables fit
    assert torch.isfinite(eng.step_slots(z, tn, tp)).all()
