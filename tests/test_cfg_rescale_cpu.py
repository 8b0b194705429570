"""CPU-only checks of the CFG control (per-sample guidance, guidance rescale; no GPU, no kernel launches): the numpy mirror's
properties (phi = 0 is the identity, phi = 1 restores the conditional std, s_b is scale-invariant, sigma_y = 0 gives 1, diffusers'
rescale_noise_cfg per sample), the header declares the new entries and _lib binds them, the C entries refuse bad arguments before
any HIP call, and the Python value checks."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import _cfg_ref as CR
from conftest import ROOT


def _pair(B=3, per=5000, seed=0):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((B, per)).astype(np.float32)
    n = (0.5 * rng.standard_normal((B, per)) + 0.1).astype(np.float32)
    return c, n


def test_phi_zero_is_identity():
    c, n = _pair()
    y = CR.combine_f32(c, n, [2.0, 5.0, 7.5])
    out = CR.cfg_rescale(c, y, 0.0)
    assert out.dtype == np.float32 and np.array_equal(out, y)


def test_phi_one_restores_the_conditional_std():
    c, n = _pair()
    y = CR.combine_f32(c, n, [3.0, 5.0, 7.5])
    out = CR.cfg_rescale(c, y, 1.0)
    sc = CR.sigma_f64(c)
    assert np.allclose(CR.sigma_f64(out), sc, rtol=1e-6, atol=0)
    assert np.allclose(out.std(axis=1, ddof=1), c.astype(np.float64).std(axis=1, ddof=1), rtol=1e-6)
    assert (CR.sigma_f64(y) > 1.5 * sc).all()                  # the combine did inflate the std that phi = 1 undoes


def test_scale_invariant_to_scaling_cond_and_null():
    c, n = _pair()
    g = [3.0, 4.0, 2.5]
    s = CR.scale(c, CR.combine_f32(c, n, g))
    s4 = CR.scale(4 * c, CR.combine_f32(4 * c, 4 * n, g))    # a power of two scales every fp32 value exactly
    assert np.array_equal(s, s4)
    s37 = CR.scale(3.7 * c, CR.combine_f32(3.7 * c, 3.7 * n, g))
    assert np.allclose(s, s37, rtol=1e-6, atol=0)


def test_zero_sigma_y_gives_factor_one():
    c, _ = _pair(B=2)
    y = np.zeros_like(c)
    y[1] = 0.25                                                # constant: sigma_y == 0 as well
    assert np.array_equal(CR.scale(c, y), np.ones(2, np.float32))
    assert np.array_equal(CR.rescale_f32(y, 1.0, CR.scale(c, y)), y)


def test_matches_diffusers_rescale_noise_cfg_per_sample():
    c, n = _pair(B=2, per=3000, seed=4)
    g, phi = [3.5, 6.0], [0.7, 0.3]
    y = CR.combine_f32(c, n, g)
    out = CR.cfg_rescale(c, y, phi).astype(np.float64)
    tc, ty = torch.from_numpy(c).double(), torch.from_numpy(y).double()
    ref = []
    for b in range(2):                                          # rescale_noise_cfg on one sample at a time
        rescaled = ty[b] * (tc[b].std() / ty[b].std())
        ref.append(phi[b] * rescaled + (1 - phi[b]) * ty[b])
    ref = torch.stack(ref).numpy()
    assert np.abs(out - ref).max() <= 1e-6 * np.abs(ref).max()


def test_header_declares_and_lib_binds_cfg_entries():
    from multimodal_diffusion_amd import _lib as L
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    for name in ("avd_cfg_stats_bytes", "avd_cfg_rescale_f32", "avd_denoise_step_cfg_f32"):
        assert name in declared and name in L.SIGNATURES
        assert hasattr(L.lib(), name)
    assert "} avd_cfg_control;" in header
    assert C.sizeof(L.CfgControl) == 32


def test_stats_bytes():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    assert lib.avd_cfg_stats_bytes(1, 1) == -1 and lib.avd_cfg_stats_bytes(0, 100) == -1
    # one fp64 partial of 4 sums per 1024 elements, then the [B] scales, each part 16-byte aligned
    assert lib.avd_cfg_stats_bytes(1, 2) == 32 + 16
    assert lib.avd_cfg_stats_bytes(3, 1025) == 3 * 2 * 32 + 16
    assert lib.avd_cfg_stats_bytes(32, 98304) == 32 * 96 * 32 + 128


def _desc(B=2, C_=8, T=4, H=16, W=32, eta=0.0):
    from multimodal_diffusion_amd import _lib as L
    s = L.StepDesc()
    s.embed.B, s.embed.C, s.embed.T, s.embed.H, s.embed.W = B, C_, T, H, W
    s.eta = eta
    return s


def test_cfg_argument_errors_without_gpu():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    ok = 1 << 24
    B, per = 2, 8 * 4 * 16 * 32
    n = B * per * 4                                             # bytes of one latent
    nb = lib.avd_cfg_stats_bytes(B, per)
    s = _desc()

    def step(ctl, tl=None, h=None, z=4 * ok, z_out=8 * ok, desc=s, key=None):
        return lib.avd_denoise_step_cfg_f32(C.byref(desc), None if ctl is None else C.byref(ctl), None,
                                            None if key is None else C.byref(key), tl, h, z, 16, 16, 16, z_out, 16, ok, None)

    assert step(None) == L.EINVAL and b"null control" in lib.avd_last_error()
    assert step(L.CfgControl(None, ok, None, 0)) == L.EINVAL and b"scratch" in lib.avd_last_error()       # rescale without stats
    assert step(L.CfgControl(None, ok, 2 * ok + 8, nb)) == L.EUNSUPPORTED and b"aligned" in lib.avd_last_error()
    assert step(L.CfgControl(None, ok, 2 * ok, nb - 16)) == L.EINVAL and b"needed" in lib.avd_last_error()
    assert step(L.CfgControl(None, ok, 8 * ok + n - 16, nb)) == L.EINVAL and b"overlap" in lib.avd_last_error()   # z_out
    assert step(L.CfgControl(None, ok, 12 * ok, nb), tl=16, h=12 * ok + 64) == L.EINVAL and b"overlap" in lib.avd_last_error()
    assert step(L.CfgControl(ok, ok, 2 * ok, nb), tl=16) == L.EINVAL and b"together" in lib.avd_last_error()
    assert step(L.CfgControl(ok, None, None, 0), desc=_desc(eta=0.5)) == L.EINVAL and b"noise key" in lib.avd_last_error()
    assert step(L.CfgControl(ok, None, None, 0), desc=_desc(C_=1, T=1, H=1, W=1)) == L.EINVAL            # per_sample 1 < 2
    # the elementwise entry
    assert lib.avd_cfg_rescale_f32(ok, 2 * ok, 16, 4 * ok, 0, 6 * ok, B, 1, None) == L.EINVAL              # per_sample < 2
    assert lib.avd_cfg_rescale_f32(ok, 2 * ok, None, 4 * ok, nb, 6 * ok, B, per, None) == L.EINVAL       # no phi
    assert lib.avd_cfg_rescale_f32(ok, 2 * ok, 16, None, nb, 6 * ok, B, per, None) == L.EINVAL
    assert lib.avd_cfg_rescale_f32(ok, 2 * ok, 16, 4 * ok + 4, nb, 6 * ok, B, per, None) == L.EUNSUPPORTED
    assert lib.avd_cfg_rescale_f32(ok, 2 * ok, 16, 4 * ok, nb - 1, 6 * ok, B, per, None) == L.EINVAL
    assert lib.avd_cfg_rescale_f32(ok, 2 * ok, 16, 2 * ok + 64, nb, 6 * ok, B, per, None) == L.EINVAL    # stats overlaps e_cfg
    assert lib.avd_cfg_rescale_f32(ok, 2 * ok, 16, 4 * ok, nb, ok + 64, B, per, None) == L.EINVAL        # out overlaps e_cond


def test_cfg_values():
    from multimodal_diffusion_amd import functional as Fn
    assert Fn.cfg_values(3.5, 3, "g").tolist() == [3.5] * 3
    assert Fn.cfg_values([1.0, 2.0], 2, "g").tolist() == [1.0, 2.0]
    assert Fn.cfg_values(torch.tensor([0.0, 1.0]), 2, "phi", 0.0, 1.0).tolist() == [0.0, 1.0]
    for bad in (1.5, -0.1, float("nan"), [0.2, float("inf")]):
        with pytest.raises(ValueError, match="phi"):
            Fn.cfg_values(bad, 2, "phi", 0.0, 1.0)
    with pytest.raises(ValueError, match="one per sample"):
        Fn.cfg_values([1.0, 2.0, 3.0], 2, "guidance")
