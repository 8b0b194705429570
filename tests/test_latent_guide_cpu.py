"""CPU-only checks of the latent guide (inpainting / SDEdit; no GPU, no kernel launches): the numpy mirror of the known-noise stream
is a stream of its own with normal statistics, truncate_schedule keeps the right tail, the header declares the two entries and _lib
binds them, the C entries refuse bad arguments before any HIP call, and the Python API rejects misuse before it needs a device."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import _guide_ref as G
from _noise_ref import DOMAIN, normals
from conftest import ROOT


def test_known_noise_stream_is_its_own_and_normal():
    B, per = 4, 1 << 16
    k = G.known_normals(11, 3, B, per)
    assert k.shape == (B, per) and np.isfinite(k).all()
    assert G.TAG_K != DOMAIN
    # the same construction with the DDIM tag at t = 0 is the DDIM stream: the tag alone separates the two
    assert np.array_equal(G.known_normals(11, 3, B, per, tag=DOMAIN), normals(11, 3, [0] * B, per))
    assert np.abs(k - normals(11, 3, [0] * B, per)).max() > 1.0
    # samples and seeds draw different values
    assert not np.allclose(k[0], k[1])
    assert not np.allclose(k, G.known_normals(12, 3, B, per))
    # sample_offset is a shift of the global sample index
    assert np.array_equal(G.known_normals(11, 5, 2, per), k[2:])
    x = k.ravel()
    mean, var = x.mean(), x.var()
    kurt = ((x - mean) ** 4).mean() / var ** 2
    assert abs(mean) < 0.01 and abs(var - 1) < 0.01 and abs(kurt - 3) < 0.05, (mean, var, kurt)


def test_q_and_blend_reference():
    abar = np.linspace(0.99, 0.01, 10)
    known = np.random.default_rng(0).standard_normal((3, 2, 8))
    q = G.q_f64(known, [-1, 0, 20], abar, seed=1)
    assert np.array_equal(q[0], known[0])                        # tau < 0: x_k exactly
    n = G.known_normals(1, 0, 3, 16).reshape(3, 2, 8)
    assert np.allclose(q[2], np.sqrt(0.01) * known[2] + np.sqrt(0.99) * n[2])  # clamped to T - 1
    z = np.random.default_rng(1).standard_normal(q.shape)
    m = np.zeros((2, 8))
    m[0, :3], m[1, 5] = 1.0, 0.25
    out = G.blend_f64(m, q, z)
    assert np.array_equal(out[:, 0, :3], q[:, 0, :3]) and np.array_equal(out[:, 0, 3:], z[:, 0, 3:])
    assert np.allclose(out[:, 1, 5], 0.75 * z[:, 1, 5] + 0.25 * q[:, 1, 5])


def test_truncate_schedule():
    from multimodal_diffusion_amd import schedule_utils as su
    sched = su.make_sampling_schedule(1000, 50)
    assert torch.equal(su.truncate_schedule(sched, 1.0), sched)
    assert su.truncate_schedule(sched, 0.0).tolist() == [-1]       # no steps
    half = su.truncate_schedule(sched, 0.5)
    assert half.numel() == 26 and torch.equal(half, sched[25:])
    s7 = su.make_sampling_schedule(1000, 7)
    assert torch.equal(su.truncate_schedule(s7, 0.5), s7[4:])       # floor(3.5) = 3 steps
    assert torch.equal(su.truncate_schedule(s7, 0.6), s7[3:])       # floor(4.2) = 4 steps
    assert torch.equal(su.truncate_schedule(s7, 3 / 7), s7[4:])     # 3/7 * 7 rounds below 3 in fp64: the 1e-9 keeps 3 steps
    assert torch.equal(su.truncate_schedule(s7, 0.999), s7[1:])     # 6 steps
    for bad in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="strength"):
            su.truncate_schedule(sched, bad)


def test_header_declares_and_lib_binds_guide_entries():
    from multimodal_diffusion_amd import _lib as L
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    for name in ("avd_latent_guide_f32", "avd_denoise_step_guided_f32"):
        assert name in declared and name in L.SIGNATURES
        assert hasattr(L.lib(), name)
    assert "avd_latent_guide;" in header and "0x4B4E5731" in header
    assert C.sizeof(L.LatentGuide) == 40


def _desc(B=2, C_=8, T=4, H=16, W=32, eta=0.0):
    from multimodal_diffusion_amd import _lib as L
    s = L.StepDesc()
    s.embed.B, s.embed.C, s.embed.T, s.embed.H, s.embed.W = B, C_, T, H, W
    s.eta = eta
    return s


def test_guide_argument_errors_without_gpu():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    ok = 1 << 24
    B, per = 2, 8 * 4 * 16 * 32
    n = B * per * 4                                                  # bytes of one latent
    key = L.NoiseKey(1, 0)
    s = _desc()

    def step(g, k=None, tl=None, h=None, z=4 * ok, z_out=8 * ok, desc=s):
        return lib.avd_denoise_step_guided_f32(C.byref(desc), None if g is None else C.byref(g), None if k is None else C.byref(k), tl, h,
                                               z, 16, 16, 16, z_out, 16, ok, None)

    assert step(None) == L.EINVAL and b"null guide" in lib.avd_last_error()
    assert step(L.LatentGuide(None, None, 0, key)) == L.EINVAL and b"known" in lib.avd_last_error()
    assert step(L.LatentGuide(ok, None, 7, key)) == L.EINVAL and b"mask_batch_stride" in lib.avd_last_error()
    assert step(L.LatentGuide(ok + 4, None, 0, key)) == L.EUNSUPPORTED and b"aligned" in lib.avd_last_error()
    assert step(L.LatentGuide(ok, ok + 8, 0, key)) == L.EUNSUPPORTED
    # known / mask overlapping z_out or x0_hist
    assert step(L.LatentGuide(8 * ok + n - 16, None, 0, key)) == L.EINVAL and b"overlap" in lib.avd_last_error()
    assert step(L.LatentGuide(ok, 8 * ok - 16, 0, key)) == L.EINVAL
    assert step(L.LatentGuide(ok, 8 * ok - per * 4 + 16, per, key)) == L.EINVAL          # a per-sample mask spans the batch
    assert step(L.LatentGuide(ok, None, 0, key), tl=16, h=ok + 64) == L.EINVAL
    # the DPM pair goes together; unseeded eta > 0 is refused
    assert step(L.LatentGuide(ok, None, 0, key), tl=16) == L.EINVAL and b"together" in lib.avd_last_error()
    assert step(L.LatentGuide(ok, None, 0, key), desc=_desc(eta=0.5)) == L.EINVAL and b"noise key" in lib.avd_last_error()
    assert step(L.LatentGuide(ok, None, 0, key), tl=16, h=12 * ok, desc=_desc(eta=0.5)) == L.EINVAL
    assert lib.avd_denoise_step_guided_f32(None, None, None, None, None, 16, 16, 16, 16, 16, 16, ok, None) == L.EINVAL
    # the elementwise entry
    g = L.LatentGuide(ok, None, 0, key)
    assert lib.avd_latent_guide_f32(None, 16, 16, 1000, None, 2 * ok, B, per, None) == L.EINVAL
    assert lib.avd_latent_guide_f32(C.byref(g), 16, 16, 1000, None, ok + 64, B, per, None) == L.EINVAL   # out overlaps known
    assert lib.avd_latent_guide_f32(C.byref(g), None, 16, 1000, None, 2 * ok, B, per, None) == L.EINVAL
    assert lib.avd_latent_guide_f32(C.byref(g), 16, 16, 1000, None, 2 * ok, 0, per, None) == L.EINVAL
    assert lib.avd_latent_guide_f32(C.byref(L.LatentGuide(ok, None, 0, L.NoiseKey(1, 2 ** 32 - 1))), 16, 16, 1000, None, 2 * ok, B,
                                    per, None) == L.EINVAL                                              # sample index past 2^32


def test_frame_mask():
    import multimodal_diffusion_amd as A
    m = A.frame_mask((8, 6, 4, 4), 0, 2)
    assert m.dtype == torch.float32 and m.shape == (8, 6, 4, 4)
    assert bool((m[:, :2] == 1).all()) and bool((m[:, 2:] == 0).all())
    a = A.frame_mask((1, 8, 40), 30, 40)
    assert bool((a[..., 30:] == 1).all()) and float(a.sum()) == 80
    for bad in (((8, 6, 4, 4), 3, 2), ((8, 40), 0, 41), ((8,), 0, 1)):
        with pytest.raises(ValueError):
            A.frame_mask(*bad)


def _sample_kwargs(**kw):
    base = dict(cfg={}, vid_vae=None, aud_codec=None, adapt_v=None, adapt_a=None, core=None, head=None, tstep_dim=256,
                prompt_modality="audio", prompt_video=None, prompt_audio=np.zeros(16000, dtype=np.float32), device=torch.device("cpu"))
    base.update(kw)
    return base


def test_sample_one_direction_rejects_misuse_without_gpu():
    import multimodal_diffusion_amd as A
    with pytest.raises(ValueError, match="init"):
        A.sample_one_direction(**_sample_kwargs(mask=np.ones((8, 1, 4, 4), dtype=np.float32)))
    with pytest.raises(ValueError, match="init"):
        A.sample_one_direction(**_sample_kwargs(strength=0.5))
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match="strength"):
            A.sample_one_direction(**_sample_kwargs(strength=bad, init_video=np.zeros((4, 32, 32, 3), dtype=np.uint8)))
    with pytest.raises(ValueError, match="init_audio"):          # the audio->video direction's target is video
        A.sample_one_direction(**_sample_kwargs(init_audio=np.zeros(16000, dtype=np.float32)))
    with pytest.raises(ValueError, match="init_video"):
        A.sample_one_direction(**_sample_kwargs(prompt_modality="video", init_video=np.zeros((4, 32, 32, 3), dtype=np.uint8)))
    with pytest.raises(ValueError, match="not both"):
        A.sample_one_direction(**_sample_kwargs(init_video=np.zeros((4, 32, 32, 3), dtype=np.uint8),
                                                init_audio=np.zeros(16000, dtype=np.float32)))
