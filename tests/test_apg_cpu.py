"""CPU-only checks of adaptive projected guidance (include/avdiff_hip.h, "adaptive projected guidance"; no GPU, no kernel launches):
the algebra of the numpy mirror against fp64 evaluations, the momentum recurrence, the parsing and refusals of ``sampling.apg`` and
of the parameter checks ``set_apg`` shares, the header / binding of the new entries, and the C entries' refusals, which all come
before any launch."""
import ctypes as C
import re
from pathlib import Path

import numpy as np
import pytest

import _apg_ref as AR
from _kit import pipeline_cfg

ROOT = Path(__file__).resolve().parent.parent
EPS32 = float(np.finfo(np.float32).eps)


def _inputs(seed=0, B=3, shape=(8, 4, 16, 20)):
    """null = 0.5 cond + 0.5 xi with xi an independent normal: the coefficient checks' inputs"""
    g = np.random.default_rng(seed)
    c = g.standard_normal((B,) + shape).astype(np.float32)
    u = (0.5 * c + 0.5 * g.standard_normal(c.shape)).astype(np.float32)
    return c, u


def _f64(c, u, g, r, eta_p):
    """the contract evaluated in fp64 throughout (no momentum): (e, update = d - k c, s)"""
    c, u = c.astype(np.float64), u.astype(np.float64)
    d = c - u
    sdd, sdc, scc = AR.moments(c, d)
    sh = (-1,) + (1,) * (c.ndim - 1)
    s = np.ones_like(sdd) if r == 0 else np.minimum(1.0, r / np.sqrt(sdd))
    k = (1.0 - eta_p) * sdc / scc
    upd = d - k.reshape(sh) * c
    gb = np.broadcast_to(np.asarray(g, np.float64).reshape(-1), sdd.shape)
    return c + ((gb - 1.0) * s).reshape(sh) * upd, upd, s


# ------------------------------------------------------------------------------------------------- algebra of the mirror
def test_neutral_parameters_are_cfg_to_rounding():
    c, u = _inputs()
    g = [3.5, 1.0, 7.0]
    e64, _, _ = _f64(c, u, g, 0.0, 1.0)
    gb = np.asarray(g, np.float64).reshape(-1, 1, 1, 1, 1)
    cfg64 = u.astype(np.float64) + gb * (c.astype(np.float64) - u.astype(np.float64))
    # c + (g - 1)(c - u) against u + g (c - u): three fp64 operations each on values of size <= g |c - u| + |c|
    scale = np.abs(c) + gb * np.abs(c.astype(np.float64) - u)
    assert (np.abs(e64 - cfg64) <= 4 * np.finfo(np.float64).eps * scale).all()
    e, d, (s, k, w) = AR.apg(c, u, g, 0.0, 1.0)
    assert (s == 1).all() and (k == 0).all() and np.array_equal(w, np.asarray(g, np.float32) - 1)
    assert np.array_equal(d, c - u)
    # the fp32 mirror: d, k c (= 0, exact), d - 0 (exact), w d, c + w d -> three roundings on values of size <= scale
    assert (np.abs(e.astype(np.float64) - cfg64) <= 3 * EPS32 * scale).all()


def test_eta_zero_update_is_orthogonal_to_cond():
    c, u = _inputs(seed=1)
    assert AR.cancellation_free(c, AR.direction(c, u))
    _, upd64, _ = _f64(c, u, 3.5, 0.0, 0.0)
    _, d, (s, k, w) = AR.apg(c, u, 3.5, 0.0, 0.0)
    upd32 = (d - k.reshape(-1, 1, 1, 1, 1) * c).astype(np.float32)
    for b in range(c.shape[0]):
        c64, nc = c[b].astype(np.float64).ravel(), float(np.linalg.norm(c[b].astype(np.float64)))
        # fp64 evaluation: orthogonal to the rounding of n fp64 products
        assert abs(upd64[b].ravel() @ c64) <= 1e-12 * np.linalg.norm(upd64[b]) * nc
        # fp32 mirror: every element of d - k c carries the roundings of c - u, k c and the subtraction, each <= eps/2 of a value
        # <= |d_i| + |k c_i|, and k itself is off by <= eps/2 |k|.  Summed against c (Cauchy-Schwarz over the n products):
        #   |sum upd_i c_i| <= eps (|d| |c| + 2.5 |k| |c|^2)
        nd, kb = float(np.linalg.norm(d[b].astype(np.float64))), abs(float(k[b]))
        bound = EPS32 * (nd * nc + 2.5 * kb * nc * nc)
        got = abs(upd32[b].astype(np.float64).ravel() @ c64)
        assert got <= bound, (got, bound)
        assert got / (np.linalg.norm(upd32[b].astype(np.float64)) * nc) < 1e-6


def test_norm_threshold_caps_the_direction():
    c, u = _inputs(seed=2)
    d = AR.direction(c, u)
    norms = np.sqrt(AR.moments(c, d)[0])
    for r in (0.25 * norms.min(), float(norms[1]), 4.0 * norms.max()):
        s, _, w = AR.coefficients(c, d, 2.0, r=r)
        capped = s.astype(np.float64) * norms
        assert (capped <= np.float32(r) * (1 + EPS32)).all()                        # s_b is rounded once: half an ulp over at most
        assert ((s == 1) == (norms <= np.float32(r))).all()
        assert np.array_equal(w, s)                                                 # g - 1 = 1
    assert (AR.coefficients(c, d, 2.0, r=0.0)[0] == 1).all()                        # r == 0: no cap
    z = np.zeros_like(c)
    s, k, w = AR.coefficients(z, z, 2.0, r=1.0, eta_p=0.3)                          # S_dd == 0 and S_cc == 0
    assert (s == 1).all() and (k == 0).all()


def test_momentum_recurrence_over_three_steps():
    beta = -0.5
    steps = [_inputs(seed=10 + i, B=2, shape=(8, 40)) for i in range(3)]
    # the mirror, the buffer carried from step to step, starting from zero
    m = np.zeros_like(steps[0][0])
    got = []
    for i, (c, u) in enumerate(steps):
        e, m, coef = AR.apg(c, u, 3.5, r=7.0, eta_p=0.2, beta=beta, m_prev=m)
        got.append((e, m.copy(), coef))
        if i == 0:
            assert np.array_equal(m, c - u)                                         # a zeroed buffer gives the first step d = d0
    # a hand-written loop over plain arrays
    f = np.float32
    d_prev = None
    for i, (c, u) in enumerate(steps):
        d = (c - u) if d_prev is None else ((c - u) + f(beta) * d_prev).astype(f)
        sdd, sdc, scc = (d.astype(np.float64) ** 2).sum((1, 2)), (d.astype(np.float64) * c).sum((1, 2)), (c.astype(np.float64) ** 2).sum((1, 2))
        s = np.minimum(1.0, np.float64(f(7.0)) / np.sqrt(sdd)).astype(f)
        k = ((1.0 - np.float64(f(0.2))) * sdc / scc).astype(f)
        w = (f(3.5) - f(1.0)) * s
        e = c + w[:, None, None] * (d - k[:, None, None] * c)
        assert np.array_equal(e, got[i][0]) and np.array_equal(d, got[i][1])
        assert all(np.array_equal(a, b) for a, b in zip((s, k, w), got[i][2]))
        d_prev = d
    # beta == 0 takes no buffer
    with pytest.raises(AssertionError):
        AR.direction(*steps[0], 0.0, np.zeros_like(steps[0][0]))


# ------------------------------------------------------------------------------------------------- parameters and config
def test_apg_params_and_dict():
    from multimodal_diffusion_amd import functional as Fn
    assert Fn.apg_params() == (0.0, 0.0, 0.0)
    assert Fn.apg_params(15, 0.25, np.float32(-0.5)) == (15.0, 0.25, -0.5)
    assert Fn.apg_from_dict(None) is None
    assert Fn.apg_from_dict({}) == (0.0, 0.0, 0.0)
    assert Fn.apg_from_dict({"momentum": -0.75, "norm_threshold": 2}) == (2.0, 0.0, -0.75)
    for bad in (dict(norm_threshold=-1.0), dict(norm_threshold=float("nan")), dict(norm_threshold=float("inf")),
                dict(eta_parallel=1.5), dict(eta_parallel=-0.1), dict(eta_parallel=float("nan")), dict(momentum=float("nan")),
                dict(momentum=float("-inf")), dict(momentum="0.5"), dict(eta_parallel=True), dict(norm_threshold=None)):
        with pytest.raises(ValueError, match="apg"):
            Fn.apg_params(**bad)
    with pytest.raises(ValueError, match="rescale"):
        Fn.apg_from_dict({"rescale": 0.5})
    with pytest.raises(ValueError, match="dict"):
        Fn.apg_from_dict(0.5)


def _read(cfg):
    from multimodal_diffusion_amd import _pipeline as P
    return P.read_config(cfg, "audio", guidance_interval=None, resample=None, has_init=False, has_mask=False, noise_seed=None)


def test_sampling_apg_parsing_and_refusals():
    def cfg(**sampling):
        return pipeline_cfg(clip_seconds=1.0, sampler_steps=4, sampling=sampling)

    assert _read(cfg()).apg is None
    assert _read(cfg(apg={"audio": {"momentum": -0.5}})).apg is None                # the prompt is audio: the target is video
    pc = _read(cfg(apg={"video": {"norm_threshold": 12.5, "eta_parallel": 0.5, "momentum": -0.5}, "audio": {}}))
    assert pc.target == "video" and pc.apg == (12.5, 0.5, -0.5)
    assert _read(cfg(apg={"video": {}})).apg == (0.0, 0.0, 0.0)
    assert _read(cfg(apg={"video": {}}, guidance_rescale={"audio": 0.7})).apg == (0.0, 0.0, 0.0)      # the other target's rescale
    for bad, what in (({"video": {"eta_parallel": 2.0}}, "eta_parallel"), ({"video": {"norm_threshold": float("nan")}}, "finite"),
                      ({"video": {"beta": 0.5}}, "beta"), ({"image": {}}, "modality"), ({"video": 0.5}, "dict"), (0.5, "modality")):
        with pytest.raises(ValueError, match=what):
            _read(cfg(apg=bad))
    with pytest.raises(ValueError, match="guidance_rescale"):
        _read(cfg(apg={"video": {}}, guidance_rescale={"video": 0.7}))


def test_engine_refuses_rescale_beside_apg():
    import torch
    from multimodal_diffusion_amd.sampler import DenoiseEngine
    assert DenoiseEngine._check_apg(None, torch.tensor([0.7])) is None
    assert DenoiseEngine._check_apg((0.0, 1.0, 0.0), torch.zeros(2)) == (0.0, 1.0, 0.0)
    with pytest.raises(ValueError, match="guidance_rescale"):
        DenoiseEngine._check_apg((0.0, 1.0, 0.0), torch.tensor([0.0, 0.3]))


# ------------------------------------------------------------------------------------------------- the C ABI
def test_header_declares_and_lib_binds_apg_entries():
    from multimodal_diffusion_amd import _lib as L
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    for name in ("avd_apg_stats_bytes", "avd_apg_guidance_f32", "avd_denoise_step_apg_f32"):
        assert name in declared and name in L.SIGNATURES
        assert hasattr(L.lib(), name)
    assert "} avd_apg_control;" in header and "MATHEMATICALLY BUT NOT IN BITS" in header
    assert C.sizeof(L.ApgControl) == 40 and C.sizeof(L.CfgControl) == 32          # avd_cfg_control keeps its layout


def test_apg_stats_bytes():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    assert lib.avd_apg_stats_bytes(1, 1) == -1 and lib.avd_apg_stats_bytes(0, 100) == -1 and lib.avd_apg_stats_bytes(65536, 100) == -1
    # one fp64 partial of 3 sums per 1024 elements (16-byte aligned as a whole), then (s, k, w, g) per sample
    assert lib.avd_apg_stats_bytes(1, 2) == 32 + 16
    assert lib.avd_apg_stats_bytes(3, 1025) == 3 * 2 * 24 + 48
    assert lib.avd_apg_stats_bytes(32, 98304) == 32 * 96 * 24 + 512


def _desc(B=2, C_=8, T=4, H=16, W=32, eta=0.0):
    from multimodal_diffusion_amd import _lib as L
    s = L.StepDesc()
    s.embed.B, s.embed.C, s.embed.T, s.embed.H, s.embed.W = B, C_, T, H, W
    s.eta = eta
    return s


def test_apg_argument_errors_without_gpu():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    ok = 1 << 24                                                # "pointers": multiples of ok, 16 MiB apart
    B, per = 2, 8 * 4 * 16 * 32
    n = B * per * 4                                             # bytes of one latent
    nb = lib.avd_apg_stats_bytes(B, per)
    s = _desc()
    Z, ZO, WS, ST, MOM, HIST = 4 * ok, 8 * ok, 16 * ok, 2 * ok, 12 * ok, 14 * ok

    def step(apg, ctl=None, tl=None, h=None, desc=s, key=None, chop=0, ghop=0, guide=None):
        return lib.avd_denoise_step_apg_f32(C.byref(desc), None if apg is None else C.byref(apg), None if ctl is None else C.byref(ctl),
                                            guide, None if key is None else C.byref(key), chop, ghop, tl, h, Z, 16, 16, 16, ZO, WS, ok,
                                            None)

    def A(r=0.0, eta_p=0.0, beta=0.0, mom=None, st=ST, sb=nb):
        return L.ApgControl(r, eta_p, beta, mom, st, sb)

    err = lib.avd_last_error
    assert step(None) == L.EINVAL and b"null APG control" in err()
    for bad in (A(r=-1.0), A(r=float("nan")), A(r=float("inf")), A(eta_p=1.5), A(eta_p=-0.5), A(eta_p=float("nan")),
                A(beta=float("nan"), mom=MOM), A(beta=float("inf"), mom=MOM)):
        assert step(bad) == L.EINVAL and b"apg_control" in err()
    assert step(A(), ctl=L.CfgControl(None, ok, 3 * ok, 1 << 20)) == L.EINVAL and b"rescale" in err()
    assert step(A(beta=-0.5)) == L.EINVAL and b"exactly when" in err()                      # momentum without a buffer
    assert step(A(mom=MOM)) == L.EINVAL and b"exactly when" in err()                        # a buffer without momentum
    assert step(A(st=None)) == L.EINVAL and b"scratch" in err()
    assert step(A(st=ST + 8)) == L.EUNSUPPORTED and b"aligned" in err()
    assert step(A(sb=nb - 16)) == L.EINVAL and b"needed" in err()
    assert step(A(beta=-0.5, mom=MOM + 4)) == L.EUNSUPPORTED and b"aligned" in err()
    for where in (Z + n - 16, ZO + 64, WS + 4096, HIST + n - 16):                           # z, z_out, the workspace (eps), x0_hist
        assert step(A(st=where), tl=16, h=HIST) == L.EINVAL and b"overlap" in err()
        assert step(A(beta=-0.5, mom=where), tl=16, h=HIST) == L.EINVAL and b"overlap" in err()
    assert step(A(beta=-0.5, mom=ST - n + 16)) == L.EINVAL and b"overlap" in err()          # the buffer's end on the scratch
    assert step(A(), desc=_desc(eta=0.5)) == L.EINVAL and b"noise key" in err()             # eta > 0 without a key
    assert step(A(), tl=16) == L.EINVAL and b"together" in err()
    assert step(A(), chop=2) == L.EINVAL and b"eta > 0" in err()                            # canvas keying at eta == 0
    assert step(A(), ghop=2) == L.EINVAL and b"guide" in err()                              # a guide hop without a guide
    assert step(A(), chop=-1) == L.EINVAL
    assert step(A(), desc=_desc(C_=1, T=1, H=1, W=1)) == L.EINVAL                           # per_sample 1 < 2
    # the elementwise entry
    g = lambda apg, c=ok, u=3 * ok, out=6 * ok, per_=per: lib.avd_apg_guidance_f32(c, u, None, 3.0, C.byref(apg), out, B, per_, None)  # noqa: E731
    assert g(A(), per_=1) == L.EINVAL
    assert g(A(eta_p=2.0)) == L.EINVAL and g(A(beta=-0.5)) == L.EINVAL and g(A(sb=nb - 1)) == L.EINVAL
    assert g(A(st=ST + 4)) == L.EUNSUPPORTED
    assert g(A(), out=ok + 64) == L.EINVAL and g(A(), out=3 * ok + 64) == L.EINVAL          # out on e_cond / e_null
    assert g(A(st=ok + 64)) == L.EINVAL and g(A(beta=0.5, mom=3 * ok + n - 16)) == L.EINVAL
    assert lib.avd_apg_guidance_f32(ok, 3 * ok, None, float("nan"), C.byref(A()), 6 * ok, B, per, None) == L.EINVAL
