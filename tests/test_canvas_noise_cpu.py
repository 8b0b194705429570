"""CPU-only checks of the canvas-keyed noise stream (include/avdiff_hip.h, "canvas-keyed noise"; no GPU, no kernel launches): the numpy
mirror agrees bit for bit wherever windows overlap and under a window offset, the noise term passes through the consensus mean in
float64, the new C entries are declared, bound and refuse bad arguments before any HIP call, the pinned ABI stays, and the Python entry
points check their arguments before any device work."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

import _canvas_noise_ref as CN
import _consensus_ref as W
from _kit import STREAM_HALF_SECOND, pipeline_cfg
from conftest import ROOT

SEED = 0xDEADBEEF12345678

CASES = [((5, 8, 6, 16, 16), 2), ((4, 3, 6, 3, 5), 2), ((3, 2, 5, 3, 6), 1), ((4, 8, 150), 50), ((4, 8, 150), 75), ((6, 3, 37), 5),
         ((4, 8, 30), 31), ((1, 8, 6, 4, 4), 2)]


@pytest.mark.parametrize("shape,hop", CASES)
def test_mirror_agrees_on_overlaps_and_is_the_gather_of_the_full_draw(shape, hop):
    N = shape[0]
    outer, L, inner = W.dims(shape)
    n = CN.canvas_normals(SEED, [731] * N, shape, hop)
    assert n.shape == shape and np.isfinite(n).all()
    assert W.overlaps_agree(n, hop)                                           # every window draws the same bits at a shared position
    P = (N - 1) * hop + L
    draw = CN.canvas_draw(SEED, 731, P, outer * inner)
    assert np.array_equal(n, CN.gather_windows(draw, shape, hop))
    # the definition holds no canvas length: a longer canvas keeps the positions already there
    assert np.array_equal(CN.canvas_draw(SEED, 731, P + 7, outer * inner)[:P], draw)
    # windows [lo, hi) drawn with window_offset = lo are that slice of the full batch
    for lo, hi in ((0, N), (N // 2, N), (N - 1, N)):
        part = CN.canvas_normals(SEED, [731] * (hi - lo), (hi - lo,) + shape[1:], hop, window_offset=lo)
        assert np.array_equal(part, n[lo:hi])
    # the timestep is live
    assert not np.array_equal(CN.canvas_normals(SEED, [730] * N, shape, hop), n)


def test_mirror_element_layout():
    """Element (o, l, i) of window b: sample p = (w0 + b)*hop + l, counter word e' >> 2 with e' = o*inner + i, value n[e' & 3]."""
    from _noise_ref import normals
    shape, hop, w0 = (3, 2, 5, 3, 6), 2, 4
    n = CN.canvas_normals(7, [9, 9, 9], shape, hop, window_offset=w0)
    b, o, l, h, w = 2, 1, 3, 2, 5
    p, e = (w0 + b) * hop + l, o * 18 + h * 6 + w
    assert n[b, o, l, h, w] == normals(7, p, [9], 36)[0, e]


@pytest.mark.parametrize("weighted", [False, True])
def test_noise_term_passes_through_the_consensus_mean(weighted):
    """z_out_k = det_k + sigma n(p): the weighted mean over the windows under p is mean_w(det_k) + sigma n(p).  float64, sums of at most
    a few terms: rtol 1e-12."""
    rng = np.random.default_rng(3)
    for shape, hop in (((5, 8, 6, 4, 4), 2), ((4, 8, 150), 50), ((6, 3, 37), 5), ((3, 2, 5, 3, 6), 1)):
        L = W.dims(shape)[1]
        w = rng.uniform(0.25, 2.0, L) if weighted else None
        det = rng.standard_normal(shape)
        sigma = 0.37
        n = CN.canvas_normals(SEED, [500] * shape[0], shape, hop)
        lhs = W.consensus_f64(det + sigma * n, hop, w)
        rhs = W.consensus_f64(det, hop, w) + sigma * n
        np.testing.assert_allclose(lhs, rhs, rtol=1e-12, atol=1e-12)
        # independent per-window noise does not: the variance over an overlap shrinks
        ind = rng.standard_normal(shape)
        assert not np.allclose(W.consensus_f64(det + sigma * ind, hop, w), W.consensus_f64(det, hop, w) + sigma * ind)


def test_header_declares_lib_binds_and_abi_stays():
    from multimodal_diffusion_amd import _lib as L
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    for name in ("avd_canvas_noise_f32", "avd_denoise_step_canvas_f32"):
        assert name in declared and name in L.SIGNATURES
        assert hasattr(L.lib(), name)
    assert "canvas-keyed noise" in header and "known-noise stream" in header
    assert L.ABI_VERSION == 7 and L.lib().avd_abi_version() == 7
    assert [f[0] for f in L.NoiseKey._fields_] == ["seed", "sample_offset"] and C.sizeof(L.NoiseKey) == 16


def _step_desc(L, eta, B=3):
    s = L.StepDesc()
    e = s.embed
    e.target_kind, e.target_first, e.B, e.d, e.tdim = 0, 1, B, 512, 256
    e.C, e.T, e.H, e.W, e.p0, e.p1, e.p2, e.Nt, e.Np = 8, 4, 16, 16, 2, 4, 4, 32, 10
    s.T_train, s.guidance, s.eta = 1000, 3.0, eta
    return s


def test_argument_errors_without_gpu():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    key = L.NoiseKey(1, 0)
    f = lib.avd_canvas_noise_f32
    assert f(None, 16, 16, 4, 8, 6, 2, 16, None) == L.EINVAL
    assert b"null" in lib.avd_last_error()
    assert f(C.byref(key), 16, 16, 4, 8, 6, 0, 16, None) == L.EINVAL
    assert b"hop" in lib.avd_last_error()
    assert f(C.byref(key), 16, 16, 4, 8, 6, -3, 16, None) == L.EINVAL
    assert f(C.byref(key), 16, 16, 0, 8, 6, 2, 16, None) == L.EINVAL
    assert f(C.byref(key), None, 16, 4, 8, 6, 2, 16, None) == L.EINVAL
    # the range: (sample_offset + N - 1)*hop + L <= 2^32
    top = L.NoiseKey(1, 2 ** 32 - 1)
    assert f(C.byref(top), 16, 16, 1, 8, 6, 2, 16, None) == L.EINVAL           # (2^32 - 1)*2 + 6
    assert b"2^32" in lib.avd_last_error()
    assert f(C.byref(top), 16, 16, 1, 8, 2, 1, 16, None) == L.EINVAL           # (2^32 - 1) + 2 = 2^32 + 1
    assert f(C.byref(top), 16, 16, 2, 8, 1, 1, 16, None) == L.EINVAL           # window index 2^32
    assert f(C.byref(L.NoiseKey(1, -1)), 16, 16, 4, 8, 6, 2, 16, None) == L.EINVAL
    assert f(C.byref(key), 16, 16, 4, 1 << 20, 6, 2, 1 << 14, None) == L.EINVAL      # outer*inner = 2^34
    assert b"2^34" in lib.avd_last_error()
    g = lib.avd_denoise_step_canvas_f32
    tail = (16, 16, 16, 16, 16, 16, 1 << 20, None)
    assert g(None, C.byref(key), 2, None, None, 0, *tail) == L.EINVAL
    assert g(C.byref(_step_desc(L, 0.5)), None, 2, None, None, 0, *tail) == L.EINVAL
    assert b"noise key" in lib.avd_last_error()
    assert g(C.byref(_step_desc(L, 0.0)), C.byref(key), 2, None, None, 0, *tail) == L.EINVAL
    assert b"eta" in lib.avd_last_error()
    assert g(C.byref(_step_desc(L, 0.5)), C.byref(key), 0, None, None, 0, *tail) == L.EINVAL
    assert b"hop" in lib.avd_last_error()
    assert g(C.byref(_step_desc(L, 0.5)), C.byref(top), 2, None, None, 0, *tail) == L.EINVAL
    assert b"2^32" in lib.avd_last_error()
    assert g(C.byref(_step_desc(L, 0.5)), C.byref(top), 2, None, None, 1, *tail) == L.EINVAL     # the cond-only form as well
    ctl = L.CfgControl(16, None, None, 0)
    assert g(C.byref(_step_desc(L, 0.5)), C.byref(key), 2, C.byref(ctl), None, 1, *tail) == L.EINVAL
    assert b"cond-only" in lib.avd_last_error()


def test_canvas_noise_python_checks_need_no_device():
    from multimodal_diffusion_amd import functional as Fn
    t = torch.zeros(4, dtype=torch.long)
    shape = (4, 8, 6, 4, 4)
    for bad_seed in (-1, 2 ** 64, 1.5, True):
        with pytest.raises(ValueError):
            Fn.canvas_noise(bad_seed, t, shape, 2)
    for bad_hop in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError):
            Fn.canvas_noise(1, t, shape, bad_hop)
    for bad_off in (-1, 1.5, 2 ** 32 - 1):
        with pytest.raises(ValueError):
            Fn.canvas_noise(1, t, shape, 2, window_offset=bad_off)
    for bad_shape in ((4, 8, 6, 4), (4, 8), (4, 0, 6, 4, 4)):
        with pytest.raises(ValueError):
            Fn.canvas_noise(1, t, bad_shape, 2)
    assert Fn.check_canvas_keying((1, 8, 2), 1, 2 ** 32 - 2) == 1               # the last canvas position is 2^32 - 1
    with pytest.raises(ValueError):
        Fn.check_canvas_keying((1, 8, 3), 1, 2 ** 32 - 2)


def test_stream_generate_refuses_canvas_keying_without_consensus_or_seed():
    """raised at the top of the function, before any device work: no module and no device is touched"""
    from multimodal_diffusion_amd import stream_infer as S
    assert inspect.signature(S.stream_generate).parameters["noise_keying"].default is None
    kw = dict(vid_vae=None, aud_codec=None, adapt_v=None, adapt_a=None, core=None, head=None, tstep_dim=256, prompt_modality="audio",
              prompt_video=None, prompt_audio=np.zeros(18000, dtype=np.float32), device=torch.device("cpu"))
    cfg = pipeline_cfg(clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND, sampling={"ddim_eta": 0.5})
    with pytest.raises(ValueError, match="consensus"):
        S.stream_generate(cfg=cfg, noise_keying="canvas", noise_seed=3, **kw)
    with pytest.raises(ValueError, match="noise_seed"):
        S.stream_generate(cfg=cfg, noise_keying="canvas", consensus="uniform", **kw)
    by_cfg = dict(cfg, streaming=dict(cfg["streaming"], noise_keying="canvas"))
    with pytest.raises(ValueError, match="consensus"):
        S.stream_generate(cfg=by_cfg, noise_seed=3, **kw)
    with pytest.raises(ValueError, match="noise_keying"):
        S.stream_generate(cfg=cfg, noise_keying="position", consensus="uniform", noise_seed=3, **kw)
    # the default keying keeps today's refusal, which now names the option
    with pytest.raises(ValueError, match="ddim_eta.*noise_keying='canvas'"):
        S.stream_generate(cfg=cfg, consensus="uniform", noise_seed=3, **kw)
    with pytest.raises(ValueError, match="halo"):
        S.stream_generate(cfg=cfg, consensus="uniform", noise_keying="canvas", noise_seed=3, shard=True, **kw)


def test_engine_keywords():
    import multimodal_diffusion_amd as A
    sig = inspect.signature(A.DenoiseEngine.__init__).parameters
    assert sig["noise_keying"].default == "sample" and sig["canvas_hop"].default is None
    assert A.DenoiseEngine.NOISE_KEYINGS == ("sample", "canvas")
