"""The slot form of DPM-Solver++(2M) on the GPU ("slot timesteps" in include/avdiff_hip.h): the fused update alone against its
elementwise mirror and the numpy fp32 mirror per slot — bit for bit, history included —, the whole step on uniform tables against the
per-sample step, on mixed tables against the explicit composition and the CPU oracle, and the refusals."""
import numpy as np
import pytest
import torch

import _dpm_ref as D
import _slot_dpm_ref as SD
import _slot_ref as SR
from _kit import ABAR, audio_case, case, dev, engine, model, ts  # noqa: F401  (dev, model are fixtures)
from _tune import tuned
from conftest import rel_err
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

GS = 3.5
TOL = 1e-4          # the parity tolerance of test_gpu_slot_timesteps.test_mixed_tables_against_the_oracle


def _lib():
    from multimodal_diffusion_amd import _lib as L
    return L, L.lib()


def _inputs(dev, shape, n_tok, D_tok, tabs, slot_len):
    """fixed random (z, eps2 [2B, Nt, D], h0) on the device; h0 is NaN on the first-order slots that step, which must not read it"""
    g = torch.Generator().manual_seed(sum(shape) + slot_len)
    z = torch.randn(shape, generator=g)
    eps2 = torch.randn(2 * shape[0], n_tok, D_tok, generator=g)
    h0 = torch.randn(shape, generator=g)
    tl, tn, tp = tabs
    c1 = D.coefs(SD.ABAR, tl.reshape(-1).numpy(), tn.reshape(-1).numpy(), tp.reshape(-1).numpy())[2]
    first = torch.from_numpy(c1 == 0).view(tn.shape) & (tn != tp)
    assert first.any() and (~first & (tn != tp)).any()
    h0 = torch.where(SR.per_position(first, shape[2], slot_len, z), torch.full_like(h0, float("nan")), h0)
    return z.to(dev), eps2.to(dev), h0.to(dev)


def _check_update(z, h0, out, hist, eps_lat, tabs, slot_len):
    """fused (out, hist) == functional.dpmpp_2m_step_slots == the numpy fp32 mirror per slot, bit for bit; held slots keep z and h0"""
    from multimodal_diffusion_amd import functional as Fn
    tl, tn, tp = tabs
    hm = h0.clone()
    om = Fn.dpmpp_2m_step_slots(z, eps_lat.to(z.device), hm, tl, tn, tp, ABAR, slot_len)
    assert torch.equal(out, om), float((out - om).abs().max())
    assert torch.equal(hist, hm)
    on, hn = SD.mirror_slots(z.cpu(), eps_lat.cpu(), h0.cpu(), tl, tn, tp, slot_len)
    assert torch.equal(om.cpu(), on), float((om.cpu() - on).abs().max())
    assert torch.equal(hm.cpu(), hn)
    hold = (SR.per_position(tn, z.shape[2], slot_len, z) == SR.per_position(tp, z.shape[2], slot_len, z)).expand_as(z).to(z.device)
    assert hold.any() and torch.equal(out[hold], z[hold]) and torch.equal(hist[hold], h0[hold])
    assert torch.isfinite(out).all() and torch.isfinite(hist).all()
    assert not torch.equal(out[~hold], z[~hold])


# ------------------------------------------------------------------------------------------------- 1. the fused update alone
def _video_update(dev, shape, tube, tabs, z, eps2, h0):
    L, lib = _lib()
    B, Cc, T, H, W = shape
    tl, tn, tp = (t.to(dev) for t in tabs)
    out, hist, ab = torch.full(shape, float("nan"), device=dev), h0.clone(), ABAR.to(dev)
    L.check(lib.avd_cfg_unpatch_dpmpp_2m_slots_f32(eps2.data_ptr(), z.data_ptr(), tl.data_ptr(), tn.data_ptr(), tp.data_ptr(),
                                                   ab.data_ptr(), 1000, GS, T // tube[0], hist.data_ptr(), out.data_ptr(), B, Cc, T, H, W,
                                                   *tube, L.stream_ptr(dev)))
    return out, hist


# W = 32 / 16 / 8: the 8-token and the 4-token whole-line forms and the gather form; S = 2 and 4; B = 2 and 3
VIDEO_CASES = [((2, 8, 4, 16, 32), (2, 4, 4)), ((2, 8, 4, 16, 32), (1, 4, 4)), ((2, 8, 4, 16, 16), (2, 4, 4)),
               ((2, 8, 4, 16, 8), (2, 4, 4)), ((3, 8, 4, 16, 16), (2, 4, 4))]


@pytest.mark.parametrize("shape,tube", VIDEO_CASES)
def test_video_update_equals_its_mirrors(dev, shape, tube):
    B, Cc, T, H, W = shape
    S = T // tube[0]
    tabs = SD.tables3(B, S, seed=S * 8 + B)
    Dt = Cc * tube[0] * tube[1] * tube[2]
    z, eps2, h0 = _inputs(dev, shape, int(np.prod(shape[1:])) // Dt, Dt, tabs, tube[0])
    out, hist = _video_update(dev, shape, tube, tabs, z, eps2, h0)
    # the combine of the kernel, without contraction: two roundings, as torch's separate ops; the oracle's un-patch
    eps_tok = (eps2[B:] + GS * (eps2[:B] - eps2[B:])).cpu()
    _check_update(z, h0, out, hist, R.tube_unpatch(eps_tok, Cc, T, H, W, *tube), tabs, tube[0])
    with tuned(cfg_rows=0):                               # the rows forms (W = 32, 16) against the gather form
        og, hg = _video_update(dev, shape, tube, tabs, z, eps2, h0)
    assert torch.equal(out, og) and torch.equal(hist, hg)


def _audio_update(dev, shape, chunk, tabs, z, eps2, h0, slots):
    L, lib = _lib()
    B, Ca, F = shape
    tl, tn, tp = (t.to(dev) for t in tabs)
    out, hist, ab = torch.full(shape, float("nan"), device=dev), h0.clone(), ABAR.to(dev)
    L.check(lib.avd_cfg_untoken_dpmpp_2m_audio_slots_f32(eps2.data_ptr(), z.data_ptr(), tl.data_ptr(), tn.data_ptr(), tp.data_ptr(),
                                                         ab.data_ptr(), 1000, GS, slots, hist.data_ptr(), out.data_ptr(), B, Ca, F,
                                                         *chunk, L.stream_ptr(dev)))
    return out, hist


@pytest.mark.parametrize("F", [40, 42])          # 42: two uncovered frames, which follow the last slot with eps = 0, history included
def test_audio_update_equals_its_mirrors(dev, F):
    shape, S = (2, 8, F), 10
    tabs = SD.tables3(2, S, seed=F)
    z, eps2, h0 = _inputs(dev, shape, S, 32, tabs, 4)
    out, hist = _audio_update(dev, shape, (4, 4), tabs, z, eps2, h0, S)
    eps_tok = (eps2[2:] + GS * (eps2[:2] - eps2[2:])).cpu()
    eps_lat = R.audio_untokens(eps_tok, 8, 4, F, 4)
    assert F == 40 or (eps_lat[:, :, 40:] == 0).all()
    _check_update(z, h0, out, hist, eps_lat, tabs, 4)


def test_audio_update_refuses_overlapping_chunks(dev):
    L, _ = _lib()
    z = torch.zeros(2, 8, 40, device=dev)
    tabs = [torch.full((2, 19), v) for v in (-1, 999, 949)]
    with pytest.raises(L.AvdError, match="non-overlapping"):
        _audio_update(dev, (2, 8, 40), (4, 2), tabs, z, torch.zeros(4, 19, 32, device=dev), z.clone(), 19)


def test_misaligned_history_is_refused_and_nothing_is_written(dev):
    L, lib = _lib()
    shape, tube = (2, 8, 4, 16, 32), (2, 4, 4)
    tl, tn, tp = (t.to(dev) for t in SD.tables3(2, 2, seed=1))
    z = torch.randn(shape, device=dev)
    eps2 = torch.randn(4, 64, 256, device=dev)
    buf = torch.full((z.numel() + 1,), 7.0, device=dev)
    hist = buf[1:].view(shape)
    assert hist.data_ptr() % 16 != 0
    out, ab = torch.full(shape, 7.0, device=dev), ABAR.to(dev)
    with pytest.raises(L.AvdError, match="x0_hist must be 16-byte aligned") as e:
        L.check(lib.avd_cfg_unpatch_dpmpp_2m_slots_f32(eps2.data_ptr(), z.data_ptr(), tl.data_ptr(), tn.data_ptr(), tp.data_ptr(),
                                                       ab.data_ptr(), 1000, GS, 2, hist.data_ptr(), out.data_ptr(), *shape, *tube,
                                                       L.stream_ptr(dev)))
    assert f"[avd {L.EUNSUPPORTED}]" in str(e.value)          # the unsupported-argument error
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (buf == 7.0).all()


# ------------------------------------------------------------------------------------------------- 2. the whole step
def _uniform(t, B, S, dev):
    return torch.tensor(t, dtype=torch.long, device=dev)[:, None].expand(B, S).contiguous()


@pytest.mark.parametrize("split_streams", [False, True])
@pytest.mark.parametrize("matmul", ["f32", "bf16x3"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_uniform_tables_give_the_per_sample_step(dev, model, target, matmul, split_streams):
    z, zp, npr, h0 = case(dev, target, B=2)
    with tuned(s3_min_rows=0):          # these few hundred rows on the split-operand path where bf16x3 is asked for
        eng = engine(model[1], target, tuple(z.shape), npr, guidance=GS, matmul=matmul, split_streams=split_streams, solver="dpmpp_2m")
        eng.set_prompt(zp)
        tl, tn, tp = [999, -1], [981, 402], [961, -1]          # second order; a final step without a history
        eng.x0_hist.copy_(h0)
        ref = eng.step(z, ts(tn, dev), ts(tp, dev), t_last=ts(tl, dev))
        href = eng.x0_hist.clone()
        eng.x0_hist.copy_(h0)
        S = eng.slots
        out = eng.step_slots(z, _uniform(tn, 2, S, dev), _uniform(tp, 2, S, dev), t_last=_uniform(tl, 2, S, dev))
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref), float((out - ref).abs().max())
    assert torch.equal(eng.x0_hist, href) and not torch.equal(href, h0)


@pytest.mark.parametrize("matmul", ["f32", "bf16x3"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_mixed_tables_against_the_composition_and_the_oracle(dev, model, target, matmul):
    ws, mods = model
    z, zp, npr, h0 = case(dev, target, B=2)
    with tuned(s3_min_rows=0):
        eng = engine(mods, target, tuple(z.shape), npr, guidance=GS, matmul=matmul, solver="dpmpp_2m")
        eng.set_prompt(zp)
        tl, tn, tp = SD.tables3(2, eng.slots, seed=21)
        eng.x0_hist.copy_(h0)
        out = eng.step_slots(z, tn, tp, t_last=tl)
    hist, sl = eng.x0_hist.cpu(), eng.slot_len
    # the explicit composition: the step's own eps tokens -> CFG combine -> the oracle's un-patch / overlap-add -> the numpy mirror per slot
    tok = eng.eps_tokens().cpu()
    e_tok = tok[2:] + GS * (tok[:2] - tok[2:])
    zc = z.cpu()
    eps = R.tube_unpatch(e_tok, *zc.shape[1:], 2, 4, 4) if target == "video" else R.audio_untokens(e_tok, 8, 4, zc.shape[2], 4)
    ref, x0 = SD.mirror_slots(zc, eps, h0.cpu(), tl, tn, tp, sl)
    e_out, e_hist = rel_err(out.cpu(), ref), rel_err(hist, x0)
    print(f"slot DPM step vs composition ({target}, {matmul}): rel err out {e_out:.3e}, x0_hist {e_hist:.3e}")
    assert e_out <= 1e-6 and e_hist <= 1e-6          # the measure and bound of test_gpu_dpm_solver.py
    # the oracle's whole step with per-slot embedding
    oref, ox0 = SD.oracle_step_slots(ws, target, zc, zp.cpu(), h0.cpu(), tl, tn, tp, GS, sl)
    o_out, o_hist = rel_err(out.cpu(), oref), rel_err(hist, ox0)
    print(f"slot DPM step vs oracle ({target}, {matmul}): rel err out {o_out:.3e}, x0_hist {o_hist:.3e}")
    assert o_out < TOL and o_hist < TOL
    hold = (SR.per_position(tn, z.shape[2], sl, z) == SR.per_position(tp, z.shape[2], sl, z)).expand_as(z).to(dev)
    assert hold.any() and torch.equal(out[hold], z[hold]) and torch.equal(eng.x0_hist[hold], h0[hold])
    assert not torch.equal(out[~hold], z[~hold])


def test_step_slots_dpm_refusals_leave_out_and_history_untouched(dev, model):
    from multimodal_diffusion_amd import _lib as L
    mods = model[1]
    z, zp, npr, h0 = case(dev, "video", B=2)
    tl, tn, tp = (t.to(dev) for t in SD.tables3(2, 2, seed=2))
    out = torch.full_like(z, 7.0)

    def refused(eng, match, exc=ValueError, z=z, out=out, **tabs):
        eng.set_prompt(zp)
        if eng.x0_hist is not None:
            eng.x0_hist.copy_(h0)
        t = dict(dict(t_now=tn, t_prev=tp, t_last=tl), **tabs)
        with pytest.raises(exc, match=match):
            eng.step_slots(z, t["t_now"], t["t_prev"], out=out, t_last=t["t_last"])
        torch.cuda.synchronize()
        assert out is eng.x0_hist or (out == 7.0).all()
        assert eng.x0_hist is None or torch.equal(eng.x0_hist, h0)

    refused(engine(mods, "video", tuple(z.shape), npr, guidance=GS), "ddim")                                # t_last on a ddim engine
    refused(engine(mods, "video", tuple(z.shape), npr, guidance=GS, solver="dpmpp_2m", eta=0.5, noise_seed=1), "eta == 0")
    refused(engine(mods, "video", tuple(z.shape), npr, guidance=GS, eta=0.5, noise_seed=1), "eta == 0", t_last=None)
    eng = engine(mods, "video", tuple(z.shape), npr, guidance=GS, solver="dpmpp_2m")
    refused(eng, "solver", t_last=None)                                                                     # no t_last: names the solver
    refused(eng, r"\[B, S\]", t_last=tl[:, :1])
    refused(eng, r"\[B, S\]", t_now=tn[:1])
    refused(eng, "integer", exc=TypeError, t_last=tl.float())
    refused(eng, "alias", exc=L.AvdError, out=eng.x0_hist)
    refused(eng, "alias", exc=L.AvdError, z=eng.x0_hist)
    # and the same engine steps once the arguments fit
    eng.x0_hist.copy_(h0)
    assert torch.isfinite(eng.step_slots(z, tn, tp, t_last=tl)).all() and torch.isfinite(eng.x0_hist).all()
