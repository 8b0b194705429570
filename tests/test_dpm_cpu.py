"""CPU-only checks of the DPM-Solver++(2M) sampler (no GPU, no kernel launches): the numpy reference converges to the exact ODE
endpoint of a Gaussian data model far faster than DDIM (which validates the reference's coefficients), the header declares the new
entry points and _lib binds them, the C entries refuse bad arguments before any HIP call, and DenoiseEngine rejects an unknown solver
and eta > 0 with "dpmpp_2m" before it looks for a device."""
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch

import _dpm_ref as D
from conftest import ROOT
from oracle import ref_cpu as R

MU, S_DATA = 0.3, 0.5


def _eps_exact(x, a):
    """The exact noise prediction for x0 ~ N(MU, S_DATA^2) at alpha_bar a: sigma / (alpha^2 s^2 + sigma^2) (x - alpha mu)."""
    al, sg = math.sqrt(a), math.sqrt(1.0 - a)
    return sg / (al * al * S_DATA ** 2 + sg * sg) * (x - al * MU)


def _endpoint_error(kind, n_steps, solver):
    abar = R.alpha_bar_table(R.beta_table(1000, kind)).numpy()
    sched = [int(t) for t in R.sampling_schedule(1000, n_steps)]
    x = np.linspace(-3.0, 3.0, 121)[:, None]
    a = float(abar[999])
    exact = MU + S_DATA * (x - math.sqrt(a) * MU) / math.sqrt(a * S_DATA ** 2 + (1.0 - a))
    hist, t_last = np.zeros_like(x), -1
    for tn, tp in zip(sched[:-1], sched[1:]):
        eps = _eps_exact(x, float(abar[tn]))
        if solver == "dpmpp_2m":
            x, hist = D.step_f64(x, eps, hist, abar, [t_last], [tn], [tp])
        else:                                   # DDIM, eta = 0, fp64
            a_s, a_t = float(abar[tn]), (float(abar[tp]) if tp >= 0 else 1.0)
            x0 = (x - math.sqrt(1.0 - a_s) * eps) / math.sqrt(a_s)
            x = math.sqrt(a_t) * x0 + math.sqrt(1.0 - a_t) * eps
        t_last = tn
    return float(np.abs(x - exact).max())


@pytest.mark.parametrize("kind,steps", [("cosine", (20, 40, 80)), ("linear", (40, 80))])
def test_reference_converges_faster_than_ddim(kind, steps):
    for n in steps:
        e_ddim, e_dpm = _endpoint_error(kind, n, "ddim"), _endpoint_error(kind, n, "dpmpp_2m")
        assert e_dpm <= e_ddim / 10, (kind, n, e_ddim, e_dpm)
        # DDIM is first order: its error halves per doubling of the step count
        ratio = e_ddim / _endpoint_error(kind, 2 * n, "ddim")
        assert 1.7 < ratio < 2.3, (kind, n, ratio)


def test_reference_coefficients_edge_cases():
    abar = R.alpha_bar_table(R.beta_table(1000)).numpy().copy()
    abar[5] = 1.0
    tl = np.array([-1, 999, 600, 0, 40, 10, 100, 200])
    tn = np.array([999, 950, 500, 999, 20, 5, 100, 100])
    tp = np.array([950, 900, -1, 950, 5, 2, 60, 60])
    cx, c0, c1 = D.coefs(abar, tl, tn, tp)
    assert np.isfinite(cx).all() and np.isfinite(c0).all() and np.isfinite(c1).all()
    second = c1 != 0
    assert list(second) == [False, True, False, False, False, False, False, True]
    assert (cx[2], c0[2]) == (0.0, 1.0)                           # final step: x0_s exactly
    assert (cx[4], c0[4]) == (0.0, 1.0)                           # a_t == 1.0f: x0_s exactly (first order)
    assert (cx[5], c0[5], c1[5]) == (0.0, 1.0, 0.0)               # a_s == 1.0f: the step returns x0_s
    # a first-order step is DDIM at eta = 0: c_x = sigma_t / sigma_s, c_0 = alpha_t - c_x alpha_s
    a_s, a_t = float(abar[999]), float(abar[950])
    assert abs(float(cx[0]) - math.sqrt(1 - a_t) / math.sqrt(1 - a_s)) < 1e-7
    # the second-order weights sum to the first-order one
    assert abs(float(c0[1]) + float(c1[1]) - D.coefs(abar, [-1], [950], [900])[1][0]) < 1e-6
    # the fp32 mirror returns x0_s bit for bit at t_prev = -1, whatever the history holds
    x = np.random.default_rng(0).standard_normal((2, 33)).astype(np.float32)
    e = np.random.default_rng(1).standard_normal((2, 33)).astype(np.float32)
    h = np.full((2, 33), np.nan, dtype=np.float32)
    y, x0 = D.step_f32(x, e, h, abar, [-1, 600], [500, 500], [-1, -1])
    assert np.array_equal(y, x0)


def test_header_declares_and_lib_binds_dpm_entries():
    from multimodal_diffusion_amd import _lib as L
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    for name in ("avd_dpmpp_2m_step_f32", "avd_denoise_step_dpmpp_2m_f32", "avd_sched_advance_ms"):
        assert name in declared and name in L.SIGNATURES
        assert hasattr(L.lib(), name)
    assert "lambda_u < lambda_s < lambda_t" in header


def test_dpm_argument_errors_without_gpu():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    ok = 1 << 20
    # x0_hist overlapping x_t / x_out is refused before the launch
    assert lib.avd_dpmpp_2m_step_f32(ok, 2 * ok, ok + 64, 16, 16, 16, 16, 1000, 3 * ok, 2, 100, None) == L.EINVAL
    assert b"x0_hist" in lib.avd_last_error()
    assert lib.avd_dpmpp_2m_step_f32(ok, 2 * ok, 4 * ok, 16, 16, 16, 16, 1000, 4 * ok - 16, 2, 100, None) == L.EINVAL
    assert lib.avd_dpmpp_2m_step_f32(ok, 2 * ok, 4 * ok, None, 16, 16, 16, 1000, 3 * ok, 2, 100, None) == L.EINVAL
    assert b"null" in lib.avd_last_error()
    s = L.StepDesc()
    s.eta = 0.5
    assert lib.avd_denoise_step_dpmpp_2m_f32(C.byref(s), 16, 16, 16, 16, 16, 16, 16, 16, ok, None) == L.EINVAL
    assert b"eta" in lib.avd_last_error()
    assert lib.avd_denoise_step_dpmpp_2m_f32(None, 16, 16, 16, 16, 16, 16, 16, 16, ok, None) == L.EINVAL
    assert lib.avd_sched_advance_ms(16, 5, 16, None, 16, 16, 1, None) == L.EINVAL


def _engine_kwargs(**kw):
    base = dict(adapt_v=None, adapt_a=None, core=None, head=None, tstep_dim=256, target="video", latent_shape=(1, 8, 4, 16, 16),
                prompt_tokens=10, alpha_bar=torch.ones(1000), guidance=3.0)
    base.update(kw)
    return base


def test_engine_rejects_bad_solver_without_gpu():
    import multimodal_diffusion_amd as A
    with pytest.raises(ValueError, match="solver"):
        A.DenoiseEngine(**_engine_kwargs(solver="heun"))
    with pytest.raises(ValueError, match="eta"):
        A.DenoiseEngine(**_engine_kwargs(solver="dpmpp_2m", eta=0.5))
    assert A.DenoiseEngine.SOLVERS == ("ddim", "dpmpp_2m")
