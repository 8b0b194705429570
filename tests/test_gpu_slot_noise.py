"""Clip-keyed slot noise on the MI355X (include/avdiff_hip.h, "clip-keyed slot noise"): avd_slot_noise_f32 against the numpy mirror, and
the seeded slot forms of the fused update — DDIM and the SDE form of DPM-Solver++(2M) — against the per-sample and elementwise entries
fed those normals as explicit noise, bit for bit."""
import numpy as np
import pytest
import torch

import _slot_dpm_ref as SD
import _slot_noise_ref as SN
import _slot_ref as SR
from _kit import ABAR, dev  # noqa: F401  (dev is a fixture)
from _tune import tuned

pytestmark = pytest.mark.gpu

GS = 3.5
SEED = 0x5107_5EED_0001
# W = 32 / 16 / 8: the 8-token and the 4-token whole-line forms and the gather form; tube t = 1: S = T; B = 1 and 3 (the cases of
# test_gpu_slot_timesteps.py)
VIDEO_CASES = [((2, 8, 4, 16, 32), (2, 4, 4)), ((2, 8, 4, 16, 16), (2, 4, 4)), ((2, 8, 4, 16, 8), (2, 4, 4)),
               ((2, 8, 4, 16, 32), (1, 4, 4)), ((1, 8, 4, 16, 32), (2, 4, 4)), ((3, 8, 4, 16, 16), (2, 4, 4))]


def _lib():
    from multimodal_diffusion_amd import _lib as L
    return L, L.lib()


def cur(dev, v):
    return torch.tensor([v], dtype=torch.int32, device=dev)


def off(x):
    """a buffer of x's shape whose base is misaligned by one float"""
    v = torch.empty(x.numel() + 1, device=x.device)[1:].view(x.shape)
    assert v.data_ptr() % 16 != 0
    return v


# ------------------------------------------------------------------------------------------------- 1. slot_noise against the mirror
# video with 16-byte lanes, a video shape on the one-element path (inner = 15), audio (inner = 1)
NOISE_SHAPES = [((2, 8, 4, 16, 32), 2), ((2, 3, 4, 3, 5), 2), ((2, 8, 40), 4)]


@pytest.mark.parametrize("shape,slot_len", NOISE_SHAPES)
def test_slot_noise_equals_the_mirror(dev, shape, slot_len):
    from multimodal_diffusion_amd import functional as Fn
    B, L_ = shape[0], shape[2]
    S = L_ // slot_len
    tn, _ = SR.tables(B, S, seed=L_)
    last = 2 ** 32 // slot_len - 2 * S                  # the batch's last position is 2^32 - 1
    assert SN.clip_position(last, B - 1, S, slot_len, L_ - 1) == 2 ** 32 - 1
    for first in (0, 5, -3, last):
        out = Fn.slot_noise(SEED, tn, shape, slot_len, first=first)
        assert out.shape == shape and out.data_ptr() % 16 == 0
        ref = SN.normals(SEED, tn, shape, slot_len, first=first)
        err = float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max())
        assert err < 1e-5, (first, err)                 # the tolerance of test_gpu_canvas_noise.py
        # a base offset by one float takes the one-element lanes: the same bits
        assert torch.equal(Fn.slot_noise(SEED, tn, shape, slot_len, first=first, out=off(out)), out), first
    base = Fn.slot_noise(SEED, tn, shape, slot_len, first=5)
    assert abs(float(base.mean())) < 0.05 and abs(float(base.std()) - 1) < 0.05
    # a cursor adds to first; a negative one reads as 0; the stride moves the samples apart
    assert torch.equal(Fn.slot_noise(SEED, tn, shape, slot_len, first=-2, cursor=cur(dev, 7)), base)
    for m in (-1, -2 ** 31):
        assert torch.equal(Fn.slot_noise(SEED, tn, shape, slot_len, first=5, cursor=cur(dev, m)), base), m
    wide = Fn.slot_noise(SEED, tn, shape, slot_len, first=5, stride=S + 1)
    assert torch.equal(wide[0], base[0]) and not torch.equal(wide[1], base[1])
    ref = SN.normals(SEED, tn, shape, slot_len, first=5, stride=S + 1)
    assert float(np.abs(wide.cpu().numpy().astype(np.float64) - ref).max()) < 1e-5
    assert not torch.equal(Fn.slot_noise(SEED + 1, tn, shape, slot_len, first=5), base)


def test_slot_noise_follows_the_clip_slot_and_covers_the_audio_tail(dev):
    from multimodal_diffusion_amd import functional as Fn
    # the same clip slots, held by other samples at other places: two samples of 2 slots against one sample of 4
    tn = torch.tensor([[999, 749], [499, 249]])
    two = Fn.slot_noise(SEED, tn, (2, 8, 4, 16, 16), 2, first=3)
    one = Fn.slot_noise(SEED, tn.view(1, 4), (1, 8, 8, 16, 16), 2, first=3)
    assert torch.equal(torch.cat([two[0], two[1]], 1), one[0])
    # lookahead windows (stride 1) overlap: window 1 slot 0 is window 0 slot 1 when both carry its timestep
    win = Fn.slot_noise(SEED, torch.tensor([[999, 749], [749, 499]]), (2, 8, 4, 16, 16), 2, first=-1, stride=1)
    assert torch.equal(win[1, :, :2], win[0, :, 2:])
    # F = 42: two uncovered frames follow the last slot's timestep, at their own positions
    tn, _ = SR.tables(2, 10, seed=42)
    out = Fn.slot_noise(SEED, tn, (2, 8, 42), 4, first=2)
    ref = SN.normals(SEED, tn, (2, 8, 42), 4, first=2)
    assert float(np.abs(out.cpu().numpy().astype(np.float64) - ref).max()) < 1e-5
    assert torch.equal(out[:, :, :40], Fn.slot_noise(SEED, tn, (2, 8, 40), 4, first=2, stride=10))


def test_slot_noise_refusals(dev):
    from multimodal_diffusion_amd import functional as Fn
    tn = torch.full((2, 2), 999)
    for kw in (dict(first=2 ** 32), dict(stride=0), dict(cursor=torch.zeros(1, dtype=torch.int32)),
               dict(cursor=torch.zeros(1, dtype=torch.int64, device=dev)), dict(cursor=torch.zeros(2, dtype=torch.int32, device=dev))):
        with pytest.raises(ValueError):
            Fn.slot_noise(SEED, tn, (2, 8, 4, 16, 16), 2, **kw)
    with pytest.raises(ValueError, match="slots"):
        Fn.slot_noise(SEED, torch.full((2, 3), 999), (2, 8, 4, 16, 16), 2)          # 3 slots of 2 do not fit T = 4
    with pytest.raises(ValueError, match="B, S"):
        Fn.slot_noise(SEED, torch.full((3, 2), 999), (2, 8, 4, 16, 16), 2)


# ------------------------------------------------------------------------------------------------- 2. the fused DDIM update alone
def _video_inputs(dev, shape, tube):
    g = torch.Generator().manual_seed(sum(shape) + tube[0])
    z = torch.randn(shape, generator=g).to(dev)
    eps2 = torch.randn(2 * shape[0], z[0].numel(), generator=g).to(dev)           # [2B, Nt * D]
    return z, eps2


def _video_seeded(dev, shape, tube, z, eps2, tn, tp, eta, key, tl=None, hist=None):
    """z_out of avd_cfg_unpatch_ddim_slots_seeded_f32; tn / tp (/ tl) are [B, S] device tables"""
    L, lib = _lib()
    import ctypes as C
    B, Cc, T, H, W = shape
    out, ab = torch.full(shape, float("nan"), device=dev), ABAR.to(dev)
    L.check(lib.avd_cfg_unpatch_ddim_slots_seeded_f32(eps2.data_ptr(), z.data_ptr(), L.ptr(tl), tn.data_ptr(), tp.data_ptr(), ab.data_ptr(),
                                                      1000, GS, eta, C.byref(key), T // tube[0], L.ptr(hist), out.data_ptr(), B, Cc, T, H,
                                                      W, *tube, L.stream_ptr(dev)))
    return out


def _video_per_sample(dev, shape, tube, z, eps2, a, p, eta, noise):
    L, lib = _lib()
    out, ab = torch.full(shape, float("nan"), device=dev), ABAR.to(dev)
    L.check(lib.avd_cfg_unpatch_ddim_f32(eps2.data_ptr(), z.data_ptr(), a.data_ptr(), p.data_ptr(), ab.data_ptr(), 1000, GS, eta,
                                         L.ptr(noise), out.data_ptr(), *shape, *tube, L.stream_ptr(dev)))
    return out


def _masks(z, tn, tp, slot_len):
    """(held, stepping to t_prev >= 0) per element of z"""
    L_ = z.shape[2]
    a, p = SR.per_position(tn.to(z.device), L_, slot_len, z), SR.per_position(tp.to(z.device), L_, slot_len, z)
    return (a == p).expand_as(z), ((a != p) & (p >= 0)).expand_as(z)


@pytest.mark.parametrize("eta", [0.5, 1.0])
@pytest.mark.parametrize("shape,tube", VIDEO_CASES)
def test_video_update_equals_per_sample_entry_with_slot_noise(dev, shape, tube, eta):
    from multimodal_diffusion_amd import functional as Fn
    B, S = shape[0], shape[2] // tube[0]
    tn, tp = (t.to(dev) for t in SR.tables(B, S, seed=S * 8 + B))
    z, eps2 = _video_inputs(dev, shape, tube)
    first, stride, m = -1, S + 1, 3
    cursor = cur(dev, m) if B > 1 else None               # the key holds its address: it lives as long as the key
    key = Fn.slot_key(SEED, first, stride, cursor)
    out = _video_seeded(dev, shape, tube, z, eps2, tn, tp, eta, key)
    noise = Fn.slot_noise(SEED, tn, shape, tube[0], first=first + (m if B > 1 else 0), stride=stride)
    ref = SR.by_pairs(lambda a, p: _video_per_sample(dev, shape, tube, z, eps2, a, p, eta, noise), z, tn, tp, tube[0])
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref), float((out - ref).abs().max())
    plain = SR.by_pairs(lambda a, p: _video_per_sample(dev, shape, tube, z, eps2, a, p, 0.0, None), z, tn, tp, tube[0])
    hold, noisy = _masks(z, tn, tp, tube[0])
    assert hold.any() and torch.equal(out[hold], z[hold])                        # held slots: z, bit for bit
    assert noisy.any() or B * S == 2                      # B = 1, S = 2: a hold and a final step
    assert not noisy.any() or float((out[noisy] != plain[noisy]).float().mean()) > 0.99
    assert torch.equal(out[~hold & ~noisy], plain[~hold & ~noisy])               # the final step: sigma = 0
    # the gather and the whole-line forms agree
    with tuned(cfg_rows=0):
        assert torch.equal(_video_seeded(dev, shape, tube, z, eps2, tn, tp, eta, key), out)
    # eta == 0: the key is not read (a stride the checks would refuse), the bits of the unseeded slot entry
    L, _ = _lib()
    assert torch.equal(_video_seeded(dev, shape, tube, z, eps2, tn, tp, 0.0, L.SlotKey(SEED, 0, 0, None)), plain)


def _audio_inputs(dev, F, chunk=(4, 4)):
    g = torch.Generator().manual_seed(F)
    z = torch.randn((2, 8, F), generator=g).to(dev)
    eps2 = torch.randn(4, (F - chunk[0]) // chunk[1] + 1, 8 * chunk[0], generator=g).to(dev)
    return z, eps2


def _audio_seeded(dev, z, eps2, tn, tp, eta, key, tl=None, hist=None, chunk=(4, 4)):
    L, lib = _lib()
    import ctypes as C
    out, ab = torch.full_like(z, float("nan")), ABAR.to(dev)
    L.check(lib.avd_cfg_untoken_ddim_audio_slots_seeded_f32(eps2.data_ptr(), z.data_ptr(), L.ptr(tl), tn.data_ptr(), tp.data_ptr(),
                                                            ab.data_ptr(), 1000, GS, eta, C.byref(key), tn.shape[1], L.ptr(hist),
                                                            out.data_ptr(), *z.shape, *chunk, L.stream_ptr(dev)))
    return out


def _audio_per_sample(dev, z, eps2, a, p, eta, noise, chunk=(4, 4)):
    L, lib = _lib()
    out, ab = torch.full_like(z, float("nan")), ABAR.to(dev)
    L.check(lib.avd_cfg_untoken_ddim_audio_f32(eps2.data_ptr(), z.data_ptr(), a.data_ptr(), p.data_ptr(), ab.data_ptr(), 1000, GS, eta,
                                               L.ptr(noise), out.data_ptr(), *z.shape, *chunk, L.stream_ptr(dev)))
    return out


@pytest.mark.parametrize("eta", [0.5, 1.0])
@pytest.mark.parametrize("F", [40, 42])          # 42: two uncovered frames, which follow the last slot with eps = 0
def test_audio_update_equals_per_sample_entry_with_slot_noise(dev, F, eta):
    from multimodal_diffusion_amd import functional as Fn
    S = 10
    tn, tp = (t.to(dev) for t in SR.tables(2, S, seed=F))
    z, eps2 = _audio_inputs(dev, F)
    cursor = cur(dev, 2)
    key = Fn.slot_key(SEED, 4, S, cursor)
    out = _audio_seeded(dev, z, eps2, tn, tp, eta, key)
    noise = Fn.slot_noise(SEED, tn, tuple(z.shape), 4, first=6)
    ref = SR.by_pairs(lambda a, p: _audio_per_sample(dev, z, eps2, a, p, eta, noise), z, tn, tp, 4)
    assert torch.isfinite(out).all()
    assert torch.equal(out, ref), float((out - ref).abs().max())
    plain = SR.by_pairs(lambda a, p: _audio_per_sample(dev, z, eps2, a, p, 0.0, None), z, tn, tp, 4)
    hold, noisy = _masks(z, tn, tp, 4)
    assert hold.any() and torch.equal(out[hold], z[hold])
    assert noisy.any() and float((out[noisy] != plain[noisy]).float().mean()) > 0.99
    assert torch.equal(out[~hold & ~noisy], plain[~hold & ~noisy])


def test_functional_ddim_mirror_equals_fused_update(dev):
    """functional.ddim_step_slots(eta, noise = slot_noise) on the un-patched CFG eps is the fused seeded slot update, bit for bit"""
    from multimodal_diffusion_amd import functional as Fn
    shape, tube = (2, 8, 4, 16, 32), (2, 4, 4)
    tn, tp = (t.to(dev) for t in SR.tables(2, 2, seed=3))
    z, eps2 = _video_inputs(dev, shape, tube)
    out = _video_seeded(dev, shape, tube, z, eps2, tn, tp, 0.5, Fn.slot_key(SEED, 7, 2))
    e2 = eps2.view(4, 64, 256)
    eps_lat = Fn.tube_unpatch(e2[2:] + GS * (e2[:2] - e2[2:]), 8, 4, 16, 32, *tube)
    noise = Fn.slot_noise(SEED, tn, shape, 2, first=7)
    assert torch.equal(Fn.ddim_step_slots(z, tn, tp, eps_lat, ABAR, 2, eta=0.5, noise=noise), out)
    # the defaults keep the eta == 0 bits, and eta > 0 needs its noise
    assert torch.equal(Fn.ddim_step_slots(z, tn, tp, eps_lat, ABAR, 2), Fn.ddim_step_slots(z, tn, tp, eps_lat, ABAR, 2, eta=0.0, noise=noise))
    with pytest.raises(ValueError, match="noise"):
        Fn.ddim_step_slots(z, tn, tp, eps_lat, ABAR, 2, eta=0.5)


# ------------------------------------------------------------------------------------------------- 3. the SDE form of the DPM slot update
def _dpm_history(z, tabs, slot_len, seed):
    """a history that is NaN under the first-order slots that step, which must not read it"""
    tl, tn, tp = tabs
    h0 = torch.randn(z.shape, generator=torch.Generator().manual_seed(seed))
    first = ((tl < 0) & (tn != tp))
    assert first.any() and ((tl >= 0) & (tn != tp)).any()
    return torch.where(SR.per_position(first, z.shape[2], slot_len, z.cpu()), torch.full_like(h0, float("nan")), h0).to(z.device)


@pytest.mark.parametrize("eta", [0.5, 1.0])
@pytest.mark.parametrize("shape,tube", [VIDEO_CASES[0], VIDEO_CASES[2], VIDEO_CASES[3], VIDEO_CASES[5]])
def test_video_sde_update_equals_its_functional_mirror(dev, shape, tube, eta):
    from multimodal_diffusion_amd import functional as Fn
    B, Cc, T, H, W = shape
    S = T // tube[0]
    tabs = SD.tables3(B, S, seed=S * 8 + B)
    tl, tn, tp = (t.to(dev) for t in tabs)
    z, eps2 = _video_inputs(dev, shape, tube)
    h0 = _dpm_history(z, tabs, tube[0], 5)
    hist = h0.clone()
    cursor = cur(dev, 1)
    out = _video_seeded(dev, shape, tube, z, eps2, tn, tp, eta, Fn.slot_key(SEED, 2, S, cursor), tl=tl, hist=hist)
    Dt = Cc * tube[0] * tube[1] * tube[2]
    e2 = eps2.view(2 * B, -1, Dt)
    eps_lat = Fn.tube_unpatch(e2[B:] + GS * (e2[:B] - e2[B:]), Cc, T, H, W, *tube)
    hm = h0.clone()
    om = Fn.dpmpp_2m_sde_step_slots(z, eps_lat, hm, tl, tn, tp, ABAR, tube[0], eta, Fn.slot_noise(SEED, tn, shape, tube[0], first=3))
    assert torch.equal(out, om), float((out - om).abs().max())
    assert torch.equal(hist, hm)
    hold, noisy = _masks(z, tn, tp, tube[0])
    assert hold.any() and torch.equal(out[hold], z[hold]) and torch.equal(hist[hold], h0[hold])      # a held slot's history is untouched
    assert torch.isfinite(out).all() and torch.isfinite(hist).all()
    # against the ODE slot form: the same x0 in the history, another latent wherever a noise term exists
    h_ode = h0.clone()
    ode = Fn.dpmpp_2m_step_slots(z, eps_lat, h_ode, tl, tn, tp, ABAR, tube[0])
    assert torch.equal(hist, h_ode)
    assert noisy.any() and float((out[noisy] != ode[noisy]).float().mean()) > 0.99
    with tuned(cfg_rows=0):
        hg = h0.clone()
        og = _video_seeded(dev, shape, tube, z, eps2, tn, tp, eta, Fn.slot_key(SEED, 3, S), tl=tl, hist=hg)
    assert torch.equal(og, out) and torch.equal(hg, hist)
    # eta == 0: the ODE slot form's bits, the key not read
    L, _ = _lib()
    h_0 = h0.clone()
    assert torch.equal(_video_seeded(dev, shape, tube, z, eps2, tn, tp, 0.0, L.SlotKey(SEED, 0, 0, None), tl=tl, hist=h_0), ode)
    assert torch.equal(h_0, h_ode)


@pytest.mark.parametrize("F", [40, 42])
def test_audio_sde_update_equals_its_functional_mirror(dev, F):
    from multimodal_diffusion_amd import functional as Fn
    S, eta = 10, 1.0
    tabs = SD.tables3(2, S, seed=F)
    tl, tn, tp = (t.to(dev) for t in tabs)
    z, eps2 = _audio_inputs(dev, F)
    h0 = _dpm_history(z, tabs, 4, 6)
    hist = h0.clone()
    out = _audio_seeded(dev, z, eps2, tn, tp, eta, Fn.slot_key(SEED, -4, S), tl=tl, hist=hist)
    eps_lat = Fn.audio_untokens(eps2[2:] + GS * (eps2[:2] - eps2[2:]), 8, 4, F, 4)
    hm = h0.clone()
    om = Fn.dpmpp_2m_sde_step_slots(z, eps_lat, hm, tl, tn, tp, ABAR, 4, eta, Fn.slot_noise(SEED, tn, tuple(z.shape), 4, first=-4))
    assert torch.equal(out, om), float((out - om).abs().max())
    assert torch.equal(hist, hm)
    hold, _ = _masks(z, tn, tp, 4)
    assert hold.any() and torch.equal(out[hold], z[hold]) and torch.equal(hist[hold], h0[hold])
    assert torch.isfinite(out).all() and torch.isfinite(hist).all()
