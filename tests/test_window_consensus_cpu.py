"""CPU-only checks of the latent window consensus (no GPU, no kernel launches): the numpy mirror does what the contract says, the
DPM-Solver++(2M) update commutes with it, the latent geometry of stream_generate, the canvas / window helpers, the new keywords, and
the C entry: declared, bound, exported, and refusing bad arguments before any HIP call."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

import _consensus_ref as W
import _dpm_ref as D
from conftest import ROOT


def _rng(seed):
    return np.random.default_rng(seed)


# ------------------------------------------------------------------------------------------------- the mirror
@pytest.mark.parametrize("shape,hop", [((5, 3, 6, 4, 5), 2), ((4, 3, 30), 15), ((4, 3, 30), 10), ((3, 2, 7, 3, 3), 3)])
def test_mirror_makes_overlaps_agree_and_leaves_single_cover_alone(shape, hop):
    z = _rng(0).standard_normal(shape).astype(np.float32)
    w = _rng(1).uniform(0.1, 2.0, W.dims(shape)[1]).astype(np.float32)
    assert not W.overlaps_agree(z, hop)
    for weights in (None, w):
        out = W.consensus_f32(z, hop, weights)
        assert out.dtype == np.float32 and W.overlaps_agree(out, hop)
        N, (outer, L, inner) = shape[0], W.dims(shape)
        a, b = z.reshape(N, outer, L, inner), out.reshape(N, outer, L, inner)
        n_single = 0
        for p in range((N - 1) * hop + L):
            lo, hi = W.window_range(p, L, hop, N)
            assert all(0 <= p - k * hop < L for k in range(lo, hi + 1))
            assert lo == 0 or p - (lo - 1) * hop >= L
            assert hi == N - 1 or p - (hi + 1) * hop < 0
            if lo == hi:
                n_single += 1
                assert a[lo, :, p - lo * hop, :].tobytes() == b[lo, :, p - lo * hop, :].tobytes()      # bit-unchanged
            else:
                assert not np.array_equal(a[lo, :, p - lo * hop, :], b[lo, :, p - lo * hop, :])
        assert n_single == 2 * hop + (N - 2) * max(0, 2 * hop - L)
    # no overlap, or one window: nothing changes
    assert W.consensus_f32(z, W.dims(shape)[1]).tobytes() == z.tobytes()
    assert W.consensus_f32(z[:1], hop).tobytes() == z[:1].tobytes()


def test_mirror_fixed_point_and_two_window_mean():
    canvas = _rng(2).standard_normal((3, 14, 2, 2)).astype(np.float32)
    z = W.windows_from_canvas(canvas, 6, 2)                    # 5 windows, three-fold cover
    assert W.overlaps_agree(z, 2)
    out = W.consensus_f32(z, 2)
    # (x + x + x) / 3 is x up to two roundings; with non-uniform weights (w0 x + w1 x + w2 x) / (w0 + w1 + w2) likewise
    assert np.abs(out - z).max() <= 4 * np.finfo(np.float32).eps * np.abs(z).max()
    out = W.consensus_f32(z, 2, np.linspace(0.5, 1.5, 6, dtype=np.float32))
    assert np.abs(out - z).max() <= 8 * np.finfo(np.float32).eps * np.abs(z).max()
    # two windows, equal weights: (a + b) / 2 on the overlap, in fp32
    a, b = _rng(3).standard_normal((2, 4, 8)).astype(np.float32)     # two audio windows [Ca = 4, F = 8], hop 4
    out = W.consensus_f32(np.stack([a, b]), 4, np.full(8, 0.75, dtype=np.float32))
    assert np.array_equal(out[0, :, :4], a[:, :4]) and np.array_equal(out[1, :, 4:], b[:, 4:])
    mean = (a[:, 4:] + b[:, :4]) / np.float32(2)
    # weights 0.75: two rounded products, a rounded sum and a rounded quotient, each within eps / 2 of terms no larger than |a| + |b|
    assert (np.abs(out[0, :, 4:] - mean) <= 2 * np.finfo(np.float32).eps * (np.abs(a[:, 4:]) + np.abs(b[:, :4]))).all()
    assert np.array_equal(out[0, :, 4:], out[1, :, :4])
    out1 = W.consensus_f32(np.stack([a, b]), 4)                # weights 1: the products are exact, (a + b) / 2 bit for bit
    assert np.array_equal(out1[0, :, 4:], mean)


# ------------------------------------------------------------------------------------------------- DPM-Solver++(2M) commutes
def test_dpm_update_commutes_with_consensus():
    """All windows share the timesteps, so the 2M update is one linear map of (z, eps, x0_hist) for every window: the consensus of
    the outputs is the output of the consensed inputs.  fp64, 1e-12 relative."""
    abar = np.cos(np.linspace(0.0, 1.0, 1000) * np.pi / 2 * 0.999).astype(np.float32) ** 2
    N, hop = 4, 2
    shape = (N, 3, 6, 2, 2)
    r = _rng(4)
    z, eps, hist = (r.standard_normal(shape) for _ in range(3))
    w = r.uniform(0.2, 1.8, 6)
    for tl, tn, tp in ((-1, 900, 700), (900, 700, 500), (700, 500, -1)):       # first order, second order, the last step
        t = [[v] * N for v in (tl, tn, tp)]
        y, x0 = D.step_f64(z, eps, hist, abar, *t)
        lhs = W.consensus_f64(y, hop, w)
        rhs, x0c = D.step_f64(W.consensus_f64(z, hop, w), W.consensus_f64(eps, hop, w), W.consensus_f64(hist, hop, w), abar, *t)
        assert np.abs(lhs - rhs).max() <= 1e-12 * np.abs(rhs).max()
        assert np.abs(W.consensus_f64(x0, hop, w) - x0c).max() <= 1e-12 * np.abs(x0c).max()
        assert not W.overlaps_agree(y, hop)


# ------------------------------------------------------------------------------------------------- latent geometry
def _geom_cfg(win_s, hop_s, fps=16, t_down=4, Fa=150):
    return {"video": {"fps": fps, "latent": {"t_down": t_down}}, "audio": {"latent": {"frames_per_clip": Fa}},
            "streaming": {"window_seconds": win_s, "hop_seconds": hop_s}}


def test_latent_hop():
    from multimodal_diffusion_amd import stream_infer as S
    cfg = _geom_cfg(3.0, 1.0)                                   # the shipped geometry
    assert S.latent_hop(cfg, "video") == (4, 12) and S.latent_hop(cfg, "audio") == (50, 150)
    assert S.latent_hop({k: v for k, v in cfg.items() if k != "streaming"}, "video") == (4, 12)      # the defaults are 3 s / 1 s
    cfg = _geom_cfg(0.5, 0.25)                                  # the GPU tests' geometry
    assert S.latent_hop(cfg, "video") == (1, 2) and S.latent_hop(cfg, "audio") == (75, 150)
    with pytest.raises(ValueError, match="t_down"):
        S.latent_hop(_geom_cfg(0.5, 0.125), "video")           # 2 frames per hop, t_down 4
    with pytest.raises(ValueError, match="whole number"):
        S.latent_hop(_geom_cfg(0.7, 0.25), "audio")            # 150 * 0.25 / 0.7 latent frames
    assert S.latent_hop(_geom_cfg(0.7, 0.25), "video") == (1, 2)
    with pytest.raises(ValueError):
        S.latent_hop(cfg, "text")


def test_canvas_window_round_trip():
    from multimodal_diffusion_amd import stream_infer as S
    g = torch.Generator().manual_seed(5)
    for canvas, L_, hop in ((torch.randn(3, 14, 2, 5, generator=g), 6, 2), (torch.randn(3, 300, generator=g), 150, 75),
                            (torch.randn(3, 250, generator=g), 150, 50), (torch.randn(2, 6, generator=g), 6, 4)):
        z = S.windows_from_canvas(canvas, L_, hop)
        N = (canvas.shape[1] - L_) // hop + 1
        assert tuple(z.shape) == (N, canvas.shape[0], L_) + tuple(canvas.shape[2:]) and z.is_contiguous()
        assert np.array_equal(z.numpy(), W.windows_from_canvas(canvas.numpy(), L_, hop))
        assert W.overlaps_agree(z.numpy(), hop)
        assert torch.equal(S.canvas_from_windows(z, hop), canvas)
        assert tuple(W.dims(tuple(z.shape))) == (canvas.shape[0], L_, int(np.prod(canvas.shape[2:])))
    with pytest.raises(ValueError):
        S.windows_from_canvas(torch.zeros(3, 15, 2, 2), 6, 2)      # 15 is not (N-1)*2 + 6
    with pytest.raises(ValueError):
        S.windows_from_canvas(torch.zeros(3, 4, 6), 2, 1)          # neither layout
    with pytest.raises(ValueError):
        S.canvas_from_windows(torch.zeros(3, 4), 1)


def test_keywords_and_defaults():
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd import stream_infer as S
    sig = inspect.signature(S.stream_generate).parameters
    assert sig["consensus"].default is None and sig["return_latents"].default is False
    assert inspect.signature(A.DenoiseEngine.set_window_consensus).parameters["weights"].default is None
    assert "hop" in inspect.signature(A.DenoiseEngine.set_window_consensus).parameters
    assert callable(A.DenoiseEngine.clear_window_consensus)
    assert inspect.signature(Fn.window_consensus).parameters["weights"].default is None


def test_python_checks_need_no_device():
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn
    assert Fn.window_dims((4, 8, 12, 32, 32)) == (8, 12, 1024) and Fn.window_dims((4, 8, 150)) == (8, 150, 1)
    with pytest.raises(ValueError):
        Fn.window_dims((4, 8, 12, 32))
    assert torch.equal(Fn.consensus_weights(None, 5), torch.ones(5))
    assert Fn.consensus_weights([1, 2, 3], 3).dtype == torch.float32
    for bad in ([1.0, 2.0], [1.0, 0.0, 1.0], [1.0, -1.0, 1.0], [1.0, float("nan"), 1.0], [1.0, float("inf"), 1.0]):
        with pytest.raises(ValueError):
            Fn.consensus_weights(bad, 3)
    with pytest.raises(L.AvdError):
        Fn.window_consensus(torch.zeros(2, 3, 8), 4)               # a CPU tensor: no fallback


# ------------------------------------------------------------------------------------------------- ABI
def test_header_declares_lib_binds_and_exports_the_entry():
    from multimodal_diffusion_amd import _lib as L
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    assert "avd_window_consensus_f32" in declared and "avd_window_consensus_f32" in L.SIGNATURES
    assert hasattr(L.lib(), "avd_window_consensus_f32")
    assert hasattr(C.CDLL(str(L.LIB_PATH)), "avd_window_consensus_f32")      # exported by the built library itself


def test_argument_errors_without_gpu():
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    ok = 1 << 24
    f = lib.avd_window_consensus_f32
    assert f(None, ok, 4, 8, 6, 2, 16, None) == L.EINVAL and b"window_consensus" in lib.avd_last_error()
    assert f(ok, None, 4, 8, 6, 2, 16, None) == L.EINVAL
    for N, outer, L_, hop, inner in ((0, 8, 6, 2, 16), (-1, 8, 6, 2, 16), (4, 0, 6, 2, 16), (4, 8, 0, 2, 16), (4, 8, 6, 0, 16),
                                     (4, 8, 6, -2, 16), (4, 8, 6, 2, 0)):
        assert f(ok, ok, N, outer, L_, hop, inner, None) == L.EINVAL
    # nothing to agree on: valid, and returns before any launch (there is no device here)
    assert f(ok, ok, 1, 8, 6, 2, 16, None) == 0
    assert f(ok, ok, 4, 8, 6, 6, 16, None) == 0 and f(ok, ok, 4, 8, 6, 9, 16, None) == 0
