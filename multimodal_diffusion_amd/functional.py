"""Tensor-level wrappers over the C ABI (one function per ``avd_*`` kernel entry point).

Each wrapper validates shapes the way the reference op it stands under does (AssertionError / ValueError),
allocates the output with torch (plumbing) and enqueues the HIP kernel on torch's current stream.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import Optional

import torch

from . import _lib as L

Tensor = torch.Tensor


def _st(t: Tensor) -> int:
    return L.stream_ptr(t.device)


def rmsnorm(x: Tensor, scale: Tensor, eps: float = 1e-6) -> Tensor:
    """RMSNorm with eps outside the sqrt — avdiff/models/mmdt.py:39-42."""
    x = L.dev_f32(x, "x")
    scale = L.dev_f32(scale, "scale")
    d = x.shape[-1]
    y = torch.empty_like(x)
    L.check(L.lib().avd_rmsnorm_f32(x.data_ptr(), scale.data_ptr(), y.data_ptr(), x.numel() // d, d, eps, _st(x)))
    return y


def linear(x: Tensor, weight: Tensor, bias: Optional[Tensor] = None, act: int = L.ACT_NONE,
           residual: Optional[Tensor] = None) -> Tensor:
    """act(x @ weight.T + bias) + residual on the fp32 matrix cores (torch.nn.Linear semantics)."""
    x = L.dev_f32(x, "x")
    weight = L.dev_f32(weight, "weight")
    n, k = weight.shape
    if x.shape[-1] != k:
        raise RuntimeError(f"mat1 and mat2 shapes cannot be multiplied ({tuple(x.shape)} x {k}->{n})")
    m = x.numel() // k
    out = torch.empty(*x.shape[:-1], n, device=x.device, dtype=torch.float32)
    b = None if bias is None else L.dev_f32(bias, "bias")
    r = None
    if residual is not None:
        r = L.dev_f32(residual, "residual")
        if r.shape != out.shape:
            raise RuntimeError("residual shape mismatch")
    L.check(L.lib().avd_gemm_bias_act_f32(x.data_ptr(), k, weight.data_ptr(), L.ptr(b), L.ptr(r), n, out.data_ptr(), n,
                                          m, n, k, act, _st(x)))
    return out


def linear_rmsfold(x: Tensor, weight_n: Tensor, bias: Optional[Tensor] = None, act: int = L.ACT_NONE,
                   residual: Optional[Tensor] = None, ss_in: Optional[Tensor] = None, eps: float = 1e-6, want_ss: bool = False):
    """The folded-RMSNorm Linear of the MMDiT composite (avd_gemm_rmsfold_f32).  ``weight_n`` = weight * norm_scale[None, :]
    when ``ss_in`` (the per-row sums of squares of x, [M, cols]) is given.  Returns (y, ss_out or None)."""
    x = L.dev_f32(x, "x")
    weight_n = L.dev_f32(weight_n, "weight")
    n, k = weight_n.shape
    m = x.numel() // k
    y = torch.empty(*x.shape[:-1], n, device=x.device, dtype=torch.float32)
    ss_out = torch.empty(m, n // 32, device=x.device, dtype=torch.float32) if want_ss else None
    cols = 0 if ss_in is None else ss_in.shape[-1]
    L.check(L.lib().avd_gemm_rmsfold_f32(x.data_ptr(), weight_n.data_ptr(), L.ptr(bias), L.ptr(residual), y.data_ptr(), m, n, k,
                                         act, L.ptr(ss_in), cols, eps, L.ptr(ss_out), _st(x)))
    return y, ss_out


def key_padding_bytes(mask: Optional[Tensor], B: int, N: int, device: torch.device) -> Optional[Tensor]:
    """nn.MultiheadAttention's key_padding_mask ([B,N], True / non-zero = ignore this key) as the uint8 table the kernels read.
    Float masks (additive) are not supported: the reference documents the boolean form (mmdt.py:120-123)."""
    if mask is None:
        return None
    if mask.is_floating_point():
        raise NotImplementedError("key_padding_mask must be boolean / integer (True = padding), as MMDiT.forward documents")
    if tuple(mask.shape) != (B, N):
        raise RuntimeError(f"key_padding_mask shape {tuple(mask.shape)} != {(B, N)}")
    if not mask.is_cuda:
        raise L.AvdError("key_padding_mask must be on the ROCm device (no CPU fallback)")
    return (mask != 0).to(torch.uint8).contiguous()


def attention(qkv: Tensor, n_heads: int, n_query: Optional[int] = None, key_padding_mask: Optional[Tensor] = None) -> Tensor:
    """softmax(q k^T / sqrt(Dh)) v over packed qkv [B,N,3d] -> [B,N,d] (head_dim must be 64)."""
    qkv = L.dev_f32(qkv, "qkv")
    B, N, d3 = qkv.shape
    kpm = key_padding_bytes(key_padding_mask, B, N, qkv.device)
    d = d3 // 3
    dh = d // n_heads
    out = torch.empty(B, N, d, device=qkv.device, dtype=torch.float32) if n_query in (None, N) else \
        torch.zeros(B, N, d, device=qkv.device, dtype=torch.float32)
    L.check(L.lib().avd_attn_fwd_f32(qkv.data_ptr(), out.data_ptr(), B, N, n_heads, dh, 1.0 / math.sqrt(dh),
                                     N if n_query is None else n_query, L.ptr(kpm), _st(qkv)))
    return out


def layernorm_act(x: Tensor, weight: Tensor, bias: Tensor, eps: float = 1e-5, act: int = L.ACT_NONE) -> Tensor:
    x = L.dev_f32(x, "x")
    d = x.shape[-1]
    y = torch.empty_like(x)
    L.check(L.lib().avd_layernorm_act_f32(x.data_ptr(), L.dev_f32(weight).data_ptr(), L.dev_f32(bias).data_ptr(),
                                          y.data_ptr(), x.numel() // d, d, eps, act, _st(x)))
    return y


_FREQS = {}


def temb_freqs(dim: int, max_period: int, device: torch.device) -> Tensor:
    """f_i = exp(-ln(max_period) * i / half), built on the host with the reference's fp32 op sequence
    (schedule_utils.py:80) and uploaded once per (dim, max_period, device)."""
    key = (dim, max_period, str(device))
    if key not in _FREQS:
        half = dim // 2
        f = torch.exp(-math.log(max_period) * torch.arange(0, half, dtype=torch.float32) / half)
        _FREQS[key] = f.to(device)
    return _FREQS[key]


def timestep_embedding(t: Tensor, dim: int, max_period: int = 10000) -> Tensor:
    if not t.is_cuda:
        raise L.AvdError("timesteps must be on the ROCm device (no CPU fallback)")
    if t.is_floating_point():
        # the reference accepts float timesteps; the kernel takes int64 like every caller on the hot path
        if not torch.equal(t, t.round()):
            raise L.AvdError("fractional timesteps are not supported by the HIP path")
    t = L.dev_i64(t, t.device)
    out = torch.empty(t.shape[0], dim, device=t.device, dtype=torch.float32)
    fr = temb_freqs(dim, max_period, t.device) if dim >= 2 else None
    L.check(L.lib().avd_timestep_embedding_f32(t.data_ptr(), L.ptr(fr), out.data_ptr(), t.shape[0], dim,
                                               float(max_period), _st(out)))
    return out


def tube_patch(z: Tensor, t: int, h: int, w: int) -> Tensor:
    z = L.dev_f32(z, "z")
    B, C_, T, H, W = z.shape
    assert T % t == 0 and H % h == 0 and W % w == 0, "tube sizes must divide latent dims"
    n = (T // t) * (H // h) * (W // w)
    tok = torch.empty(B, n, C_ * t * h * w, device=z.device, dtype=torch.float32)
    L.check(L.lib().avd_tube_patch_f32(z.data_ptr(), tok.data_ptr(), B, C_, T, H, W, t, h, w, _st(z)))
    return tok


def tube_unpatch(tokens: Tensor, C_: int, T: int, H: int, W: int, t: int, h: int, w: int) -> Tensor:
    tokens = L.dev_f32(tokens, "tokens")
    B, N, D = tokens.shape
    assert D == C_ * t * h * w, "token width mismatch"
    assert N == (T // t) * (H // h) * (W // w), "token count mismatch"
    z = torch.empty(B, C_, T, H, W, device=tokens.device, dtype=torch.float32)
    L.check(L.lib().avd_tube_unpatch_f32(tokens.data_ptr(), z.data_ptr(), B, C_, T, H, W, t, h, w, _st(z)))
    return z


def audio_tokens(z_a: Tensor, length: int, stride: int) -> Tensor:
    z_a = L.dev_f32(z_a, "z_a")
    B, Ca, F = z_a.shape
    if length <= 0 or stride <= 0 or F < length:      # no token to allocate: refused here, in the words of audio_tokens_f32 (csrc/tokens.hip)
        raise L.AvdError(f"audio_tokens: need 0 < len <= F and stride > 0 (got F={F} len={length} stride={stride})")
    na = (F - length) // stride + 1
    tok = torch.empty(B, na, Ca * length, device=z_a.device, dtype=torch.float32)
    L.check(L.lib().avd_audio_tokens_f32(z_a.data_ptr(), tok.data_ptr(), B, Ca, F, length, stride, _st(z_a)))
    return tok


def audio_untokens(tokens: Tensor, Ca: int, length: int, frames: int, stride: int, window: Optional[Tensor] = None) -> Tensor:
    tokens = L.dev_f32(tokens, "tokens")
    if window is not None:
        window = L.dev_f32(window, "window")
        assert window.numel() == length
    B, na, D = tokens.shape
    assert D == Ca * length
    if na != (frames - length) // stride + 1:
        raise L.AvdError("audio_untokens: token count does not match (frames, length, stride)")
    z = torch.empty(B, Ca, frames, device=tokens.device, dtype=torch.float32)
    L.check(L.lib().avd_audio_untokens_f32(tokens.data_ptr(), L.ptr(window), z.data_ptr(), B, Ca, frames, length, stride, _st(z)))
    return z


def ddim_step(x_t: Tensor, t_now: Tensor, t_prev: Tensor, eps_hat: Tensor, alpha_bar: Tensor, eta: float = 0.0,
              noise: Optional[Tensor] = None) -> Tensor:
    x_t = L.dev_f32(x_t, "x_t")
    eps_hat = L.dev_f32(eps_hat, "eps_hat")
    if eps_hat.shape != x_t.shape:
        raise RuntimeError("eps_hat must have the shape of x_t")
    dev = x_t.device
    ab = alpha_bar if (alpha_bar.is_cuda and alpha_bar.dtype == torch.float32) else alpha_bar.to(dev, torch.float32)
    ab = ab.contiguous()
    tn, tp = L.dev_i64(t_now, dev), L.dev_i64(t_prev, dev)
    B = x_t.shape[0]
    if tn.numel() != B or tp.numel() != B:
        raise RuntimeError("t_now / t_prev must have one entry per sample")
    if eta > 0.0 and noise is None:
        noise = torch.randn_like(x_t)          # the reference draws randn_like here (schedule_utils.py:197)
    nz = None if noise is None else L.dev_f32(noise, "noise")
    out = torch.empty_like(x_t)
    L.check(L.lib().avd_ddim_step_f32(x_t.data_ptr(), eps_hat.data_ptr(), tn.data_ptr(), tp.data_ptr(), ab.data_ptr(),
                                      ab.numel(), float(eta), L.ptr(nz), out.data_ptr(), B, x_t.numel() // B, _st(x_t)))
    return out


def dpmpp_2m_step(x_t: Tensor, eps_hat: Tensor, x0_hist: Tensor, t_last: Tensor, t_now: Tensor, t_prev: Tensor,
                  alpha_bar: Tensor) -> Tensor:
    """One DPM-Solver++(2M) update (avd_dpmpp_2m_step_f32; contract in include/avdiff_hip.h) from t_now to t_prev, the previous step
    having come from t_last (int [B]; < 0: no history, first order).  Returns x_{t_prev}; ``x0_hist`` (float32 [B, ...] on the
    device, the shape of x_t, not overlapping x_t / eps_hat) is read by a second-order step and overwritten with this step's x0."""
    x_t = L.dev_f32(x_t, "x_t")
    eps_hat = L.dev_f32(eps_hat, "eps_hat")
    if eps_hat.shape != x_t.shape:
        raise RuntimeError("eps_hat must have the shape of x_t")
    if not (x0_hist.is_cuda and x0_hist.dtype == torch.float32 and x0_hist.is_contiguous() and x0_hist.shape == x_t.shape):
        raise RuntimeError("x0_hist must be a contiguous float32 device tensor of x_t's shape (it is updated in place)")
    dev = x_t.device
    ab = alpha_bar if (alpha_bar.is_cuda and alpha_bar.dtype == torch.float32) else alpha_bar.to(dev, torch.float32)
    ab = ab.contiguous()
    tl, tn, tp = L.dev_i64(t_last, dev), L.dev_i64(t_now, dev), L.dev_i64(t_prev, dev)
    B = x_t.shape[0]
    if tl.numel() != B or tn.numel() != B or tp.numel() != B:
        raise RuntimeError("t_last / t_now / t_prev must have one entry per sample")
    out = torch.empty_like(x_t)
    L.check(L.lib().avd_dpmpp_2m_step_f32(x_t.data_ptr(), eps_hat.data_ptr(), x0_hist.data_ptr(), tl.data_ptr(), tn.data_ptr(),
                                          tp.data_ptr(), ab.data_ptr(), ab.numel(), out.data_ptr(), B, x_t.numel() // B, _st(x_t)))
    return out


def dpmpp_2m_sde_step(x_t: Tensor, eps_hat: Tensor, x0_hist: Tensor, t_last: Tensor, t_now: Tensor, t_prev: Tensor,
                      alpha_bar: Tensor, eta: float, noise: Optional[Tensor] = None) -> Tensor:
    """One SDE-DPM-Solver++(2M) update (avd_dpmpp_2m_sde_step_f32; contract in include/avdiff_hip.h): ``dpmpp_2m_step`` with the
    exponential coefficients of ``eta`` > 0 and the noise term c_n * ``noise``.  ``noise`` (float32, the shape of x_t, not overlapping
    x0_hist) is explicit and required when eta > 0 — ``gaussian_noise`` / ``canvas_noise`` give the normals the fused step draws; at
    eta == 0 it is not read and the result has the bits of ``dpmpp_2m_step``."""
    x_t = L.dev_f32(x_t, "x_t")
    eps_hat = L.dev_f32(eps_hat, "eps_hat")
    if eps_hat.shape != x_t.shape:
        raise RuntimeError("eps_hat must have the shape of x_t")
    if not (x0_hist.is_cuda and x0_hist.dtype == torch.float32 and x0_hist.is_contiguous() and x0_hist.shape == x_t.shape):
        raise RuntimeError("x0_hist must be a contiguous float32 device tensor of x_t's shape (it is updated in place)")
    if eta > 0.0 and noise is None:
        raise ValueError("dpmpp_2m_sde_step: eta > 0 needs `noise` (gaussian_noise / canvas_noise give the seeded stream's normals)")
    nz = None if noise is None else L.dev_f32(noise, "noise")
    if nz is not None and nz.shape != x_t.shape:
        raise RuntimeError("noise must have the shape of x_t")
    dev = x_t.device
    ab = alpha_bar if (alpha_bar.is_cuda and alpha_bar.dtype == torch.float32) else alpha_bar.to(dev, torch.float32)
    ab = ab.contiguous()
    tl, tn, tp = L.dev_i64(t_last, dev), L.dev_i64(t_now, dev), L.dev_i64(t_prev, dev)
    B = x_t.shape[0]
    if tl.numel() != B or tn.numel() != B or tp.numel() != B:
        raise RuntimeError("t_last / t_now / t_prev must have one entry per sample")
    out = torch.empty_like(x_t)
    L.check(L.lib().avd_dpmpp_2m_sde_step_f32(x_t.data_ptr(), eps_hat.data_ptr(), x0_hist.data_ptr(), tl.data_ptr(), tn.data_ptr(),
                                              tp.data_ptr(), ab.data_ptr(), ab.numel(), float(eta), L.ptr(nz), out.data_ptr(), B,
                                              x_t.numel() // B, _st(x_t)))
    return out


def _alpha_bar(alpha_bar: Tensor, dev: torch.device) -> Tensor:
    """the alpha_bar table as a contiguous float32 tensor on ``dev``"""
    ab = alpha_bar if (alpha_bar.is_cuda and alpha_bar.dtype == torch.float32) else alpha_bar.to(dev, torch.float32)
    return ab.contiguous()


def _positive_shape(shape, what: str = "shape must have positive sizes") -> tuple:
    shape = tuple(int(s) for s in shape)
    if len(shape) < 1 or any(s < 1 for s in shape):
        raise ValueError(f"{what}, got {shape}")
    return shape


def _check_out(out: Optional[Tensor], shape: tuple, z: Optional[Tensor] = None) -> None:
    """an ``out`` to fill: None, or a contiguous float32 device tensor of ``shape``, on z's device where the pass reads a ``z``"""
    ok = out is None or (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == tuple(shape))
    if z is not None and not (ok and (out is None or out.device == z.device)):
        raise ValueError(f"out must be a contiguous float32 tensor of shape {tuple(shape)} on z's device")
    if not ok:
        raise ValueError(f"out must be a contiguous float32 device tensor of shape {tuple(shape)}")


def _slot_table(t: Tensor, name: str, B: int, L_: int, slot_len) -> tuple:
    """(table, S): an int [B, S] table whose S slots of ``slot_len`` positions fit the sliding length ``L_``"""
    t = torch.as_tensor(t)
    if t.dim() != 2 or t.shape[0] != B or t.is_floating_point() or t.dtype == torch.bool:
        raise ValueError(f"{name} must be an int [B, S] table with B = {B}, got {t.dtype} {tuple(t.shape)}")
    S = int(t.shape[1])
    if isinstance(slot_len, bool) or not isinstance(slot_len, int) or slot_len < 1 or S < 1 or S * slot_len > L_:
        raise ValueError(f"S = {S} slots of slot_len {slot_len!r} must fit the sliding length {L_}")
    return t, S


def noise_key(seed: int, sample_offset: int = 0) -> "L.NoiseKey":
    """avd_noise_key after the checks the engine and gaussian_noise share: 0 <= seed < 2**64, sample_offset >= 0."""
    if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"noise seed must be an int in [0, 2**64), got {seed!r}")
    if isinstance(sample_offset, bool) or not isinstance(sample_offset, int) or sample_offset < 0:
        raise ValueError(f"sample_offset must be an int >= 0, got {sample_offset!r}")
    return L.NoiseKey(seed, sample_offset)


def latent_guide_desc(known: Tensor, mask: Optional[Tensor], seed: int, sample_offset: int = 0) -> "L.LatentGuide":
    """avd_latent_guide over ``known`` (contiguous float32 [B, ...] on the device) and ``mask`` (None = 1 everywhere; contiguous
    float32 of known.shape[1:] (shared by the batch) or of known.shape).  The struct holds raw pointers: keep both tensors alive."""
    if not (known.is_cuda and known.dtype == torch.float32 and known.is_contiguous()):
        raise ValueError("known must be a contiguous float32 device tensor")
    B = known.shape[0]
    per = known.numel() // B
    stride = 0
    if mask is not None:
        if not (mask.is_cuda and mask.dtype == torch.float32 and mask.is_contiguous() and mask.device == known.device):
            raise ValueError("mask must be a contiguous float32 tensor on known's device")
        if tuple(mask.shape) == tuple(known.shape):
            stride = per
        elif tuple(mask.shape) != tuple(known.shape[1:]):
            raise ValueError(f"mask shape {tuple(mask.shape)} must be {tuple(known.shape[1:])} (one sample, shared) or "
                             f"{tuple(known.shape)}")
    return L.LatentGuide(known.data_ptr(), L.ptr(mask), stride, noise_key(seed, sample_offset))


def latent_guide(known: Tensor, tau: Tensor, alpha_bar: Tensor, z: Optional[Tensor] = None, mask: Optional[Tensor] = None, *,
                 seed: int = 0, sample_offset: int = 0, canvas_hop: Optional[int] = None, window_offset: int = 0) -> Tensor:
    """The latent guide's blend (avd_latent_guide_f32; contract in include/avdiff_hip.h): out[b] = blend(mask, q(tau[b]), z[b]) with
    q(tau) = sqrt(a) known + sqrt(1 - a) n_k, n_k the known-noise stream of (seed, sample_offset + b).  ``z`` None: out = q (the known
    latent forward-noised to tau; tau < 0 returns ``known`` itself).  ``mask``: see latent_guide_desc.  ``tau``: int [B].
    ``canvas_hop`` (default None = the per-sample keying above): ``known`` is a batch of consecutive windows of one canvas
    ([N,C,T,H,W] video, [N,Ca,F] audio), ``canvas_hop`` positions apart, window 0 at global window index ``window_offset``, and n_k is
    keyed by canvas position (avd_latent_guide_canvas_f32; "canvas-keyed known noise"): every window over a position holds the same
    normal there.  ``sample_offset`` belongs to the per-sample keying, ``window_offset`` to the canvas one."""
    if canvas_hop is None:
        if window_offset != 0:
            raise ValueError("window_offset belongs to the canvas keying: pass canvas_hop")
        offset = sample_offset
    else:
        if sample_offset != 0:
            raise ValueError("sample_offset belongs to the per-sample keying: with canvas_hop pass window_offset")
        noise_key(seed, window_offset)                       # the offset's type and sign, before it enters the range check
        canvas_hop = check_canvas_keying(tuple(known.shape), canvas_hop, window_offset)
        offset = window_offset
    known = L.dev_f32(known, "known").contiguous()
    dev = known.device
    B = known.shape[0]
    m = None if mask is None else L.dev_f32(mask, "mask").contiguous()
    g = latent_guide_desc(known, m, seed, offset)
    tn = L.dev_i64(tau, dev)
    if tn.numel() != B:
        raise ValueError(f"tau has {tn.numel()} entries, known has {B} samples")
    zz = None
    if z is not None:
        zz = L.dev_f32(z, "z").contiguous()
        if zz.shape != known.shape:
            raise ValueError(f"z shape {tuple(zz.shape)} != known shape {tuple(known.shape)}")
    return latent_guide_launch(g, canvas_hop, tn, _alpha_bar(alpha_bar, dev), zz, torch.empty_like(known))


def latent_guide_launch(g: "L.LatentGuide", canvas_hop: Optional[int], tau: Tensor, ab: Tensor, z: Optional[Tensor], out: Tensor) -> Tensor:
    """avd_latent_guide_f32 (``canvas_hop`` None) or avd_latent_guide_canvas_f32 on checked device tensors: ``tau`` int64 [B], ``ab``
    the float32 alpha_bar table, ``z`` None or of out's shape.  Fills and returns ``out``."""
    B = out.shape[0]
    args = (C.byref(g), tau.data_ptr(), ab.data_ptr(), ab.numel(), L.ptr(z), out.data_ptr(), B)
    if canvas_hop is None:
        L.check(L.lib().avd_latent_guide_f32(*args, out.numel() // B, _st(out)))
    else:
        outer, L_, inner = window_dims(out.shape)
        L.check(L.lib().avd_latent_guide_canvas_f32(*args, outer, L_, canvas_hop, inner, _st(out)))
    return out


def check_visit(visit) -> int:
    """the `visit` word of the renoise stream: an int in [0, 2**32)"""
    if isinstance(visit, bool) or not isinstance(visit, int) or not 0 <= visit < 2 ** 32:
        raise ValueError(f"visit must be an int in [0, 2**32), got {visit!r}")
    return visit


def renoise(z: Tensor, t_from: Tensor, t_to: Tensor, alpha_bar: Tensor, seed: int, visit: int, sample_offset: int = 0,
            guide: Optional["L.LatentGuide"] = None, canvas_hop: Optional[int] = None, out: Optional[Tensor] = None) -> Tensor:
    """The forward jump of RePaint resampling (avd_renoise_f32 / avd_renoise_canvas_f32; contract in include/avdiff_hip.h, "renoise"):
    per sample b with rho = a(t_to[b]) / a(t_from[b]) < 1, out[b] = sqrt(rho) z[b] + sqrt(1 - rho) n_r, n_r the renoise stream of
    (seed, sample_offset + b, visit); out[b] = z[b] bit for bit where a(t_to[b]) is not below a(t_from[b]).  ``visit`` names the
    jump: another visit draws fresh normals.  ``guide`` (``latent_guide_desc``): the call ends in blend(mask, q(t_to), out), so a held
    region stays on its forward path.  ``canvas_hop`` (default None = per-sample keying): ``z`` is a batch of consecutive windows of one
    canvas ([N,C,T,H,W] video, [N,Ca,F] audio), window 0 at global window index ``sample_offset``, and the renoise stream and the
    guide's known noise are keyed by canvas position; the guide's key must carry the same offset.  ``out``: a contiguous float32
    device tensor of z's shape, which may be ``z`` itself (in place)."""
    z = L.dev_f32(z, "z")
    dev, B = z.device, z.shape[0]
    visit = check_visit(visit)
    key = noise_key(seed, sample_offset)
    if canvas_hop is not None:
        canvas_hop = check_canvas_keying(tuple(z.shape), canvas_hop, sample_offset)
    elif sample_offset + B > 2 ** 32:
        raise ValueError(f"sample_offset {sample_offset} + batch {B} exceeds the stream's 2**32 sample indices")
    if guide is not None and not isinstance(guide, L.LatentGuide):
        raise TypeError("guide must be an avd_latent_guide (functional.latent_guide_desc)")
    tf, tt = L.dev_i64(t_from, dev), L.dev_i64(t_to, dev)
    if tf.numel() != B or tt.numel() != B:
        raise ValueError(f"t_from / t_to have {tf.numel()} / {tt.numel()} entries, z has {B} samples")
    _check_out(out, z.shape, z)
    if out is None:
        out = torch.empty_like(z)
    ab = _alpha_bar(alpha_bar, dev)
    args = (C.byref(key), visit, None if guide is None else C.byref(guide), tf.data_ptr(), tt.data_ptr(), ab.data_ptr(), ab.numel(),
            z.data_ptr(), out.data_ptr(), B)
    if canvas_hop is None:
        L.check(L.lib().avd_renoise_f32(*args, z.numel() // B, _st(out)))
    else:
        outer, L_, inner = window_dims(z.shape)
        L.check(L.lib().avd_renoise_canvas_f32(*args, outer, L_, canvas_hop, inner, _st(out)))
    return out


def cfg_values(v, B: int, name: str, lo: Optional[float] = None, hi: Optional[float] = None) -> Tensor:
    """A per-sample CFG value (a number for every sample, or B numbers as a sequence / array / tensor) as a CPU float32 [B] tensor,
    after the checks DenoiseEngine, set_cfg and cfg_rescale share: finite, and within [lo, hi] where given (the kernels trust the
    device values of include/avdiff_hip.h, avd_cfg_control)."""
    t = torch.as_tensor(v.detach().cpu() if isinstance(v, Tensor) else v, dtype=torch.float32).reshape(-1)
    if t.numel() == 1:
        t = t.expand(B)
    if t.numel() != B:
        raise ValueError(f"{name} has {t.numel()} values, expected 1 or {B} (one per sample)")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name} must be finite, got {t.tolist()}")
    if lo is not None and not bool(((t >= lo) & (t <= hi)).all()):
        raise ValueError(f"{name} must lie in [{lo:g}, {hi:g}], got {t.tolist()}")
    return t.contiguous()


def cfg_rescale(e_cond: Tensor, e_cfg: Tensor, phi, *, return_scale: bool = False):
    """Guidance rescale on latent-layout tensors (avd_cfg_rescale_f32; contract in include/avdiff_hip.h, avd_cfg_control): per sample
    b, s_b = std(e_cond[b]) / std(e_cfg[b]) (unbiased, fp64 moments, rounded once) and out[b] = r(e_cfg[b]) = phi_b (e s_b) +
    (1 - phi_b) e (e at phi 0, e s_b at phi 1).  ``phi``: a number or B numbers in [0, 1].  ``return_scale``: also return s (float32
    [B] on the device)."""
    ec, ey = L.dev_f32(e_cond, "e_cond"), L.dev_f32(e_cfg, "e_cfg")
    if ec.shape != ey.shape or ec.device != ey.device:
        raise ValueError(f"e_cond {tuple(ec.shape)} and e_cfg {tuple(ey.shape)} must have one shape on one device")
    B = ey.shape[0]
    per = ey.numel() // B
    ph = cfg_values(phi, B, "phi", 0.0, 1.0).to(ey.device)
    nb = L.lib().avd_cfg_stats_bytes(B, per)
    if nb < 0:
        raise ValueError(f"cfg_rescale needs >= 2 elements per sample (got {per}) and 1 <= B")
    stats = torch.empty(nb, dtype=torch.uint8, device=ey.device)
    out = torch.empty_like(ey)
    L.check(L.lib().avd_cfg_rescale_f32(ec.data_ptr(), ey.data_ptr(), ph.data_ptr(), stats.data_ptr(), nb, out.data_ptr(), B, per,
                                        _st(out)))
    if return_scale:
        off = nb - ((4 * B + 15) // 16) * 16           # the scale slot ends the scratch
        return out, stats[off:off + 4 * B].view(torch.float32).clone()
    return out


def apg_params(norm_threshold=0.0, eta_parallel=0.0, momentum=0.0) -> tuple:
    """(norm_threshold, eta_parallel, momentum) of adaptive projected guidance as floats, after the checks DenoiseEngine, set_apg,
    ``sampling.apg`` and apg_guidance share: numbers (not bools), finite, norm_threshold >= 0 (0: no norm cap), eta_parallel in [0, 1]."""
    vals = []
    for name, v in (("norm_threshold", norm_threshold), ("eta_parallel", eta_parallel), ("momentum", momentum)):
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise ValueError(f"apg {name} must be a number, got {v!r}")
        v = float(v)
        if not math.isfinite(v):
            raise ValueError(f"apg {name} must be finite, got {v}")
        vals.append(v)
    if vals[0] < 0:
        raise ValueError(f"apg norm_threshold must be >= 0 (0: no norm cap), got {vals[0]}")
    if not 0.0 <= vals[1] <= 1.0:
        raise ValueError(f"apg eta_parallel must lie in [0, 1], got {vals[1]}")
    return tuple(vals)


def apg_from_dict(apg) -> Optional[tuple]:
    """``apg``: None, or a mapping with any of norm_threshold / eta_parallel / momentum (nothing else) -> None or ``apg_params``"""
    if apg is None:
        return None
    if not isinstance(apg, dict):
        raise ValueError(f"apg must be None or a dict of norm_threshold / eta_parallel / momentum, got {apg!r}")
    extra = set(apg) - {"norm_threshold", "eta_parallel", "momentum"}
    if extra:
        raise ValueError(f"apg takes norm_threshold, eta_parallel and momentum, not {sorted(extra)}")
    return apg_params(**apg)


def apg_guidance(e_cond: Tensor, e_null: Tensor, guidance, *, norm_threshold: float = 0.0, eta_parallel: float = 0.0,
                 momentum: float = 0.0, momentum_buf: Optional[Tensor] = None, return_coef: bool = False):
    """Adaptive projected guidance on latent-layout tensors (avd_apg_guidance_f32; contract in include/avdiff_hip.h, "adaptive
    projected guidance"): per sample b, d = (e_cond - e_null) + momentum * momentum_buf, and out = e_cond + (g_b - 1) s_b (d - k_b
    e_cond) with s_b = min(1, norm_threshold / |d|) (1 at norm_threshold 0) and k_b = (1 - eta_parallel) <d, e_cond> / <e_cond,
    e_cond>: the component of d parallel to e_cond is scaled by eta_parallel, the orthogonal one kept.  ``guidance``: a number or B
    numbers.  ``momentum_buf``: a contiguous float32 device tensor of e_cond's shape, required exactly when momentum != 0; it is
    read, then overwritten in place with d.  ``return_coef``: also return (s, k, w), float32 [B] each on the device, w = (g - 1) s."""
    ec, en = L.dev_f32(e_cond, "e_cond"), L.dev_f32(e_null, "e_null")
    if ec.shape != en.shape or ec.device != en.device:
        raise ValueError(f"e_cond {tuple(ec.shape)} and e_null {tuple(en.shape)} must have one shape on one device")
    r, eta_p, beta = apg_params(norm_threshold, eta_parallel, momentum)
    B = ec.shape[0]
    per = ec.numel() // B
    g = cfg_values(guidance, B, "guidance").to(ec.device)
    if (beta != 0.0) != (momentum_buf is not None):
        raise ValueError("momentum_buf goes with momentum != 0: pass both or neither")
    if momentum_buf is not None and not (momentum_buf.is_cuda and momentum_buf.dtype == torch.float32 and momentum_buf.is_contiguous()
                                         and momentum_buf.shape == ec.shape and momentum_buf.device == ec.device):
        raise ValueError(f"momentum_buf must be a contiguous float32 tensor of shape {tuple(ec.shape)} on e_cond's device")
    nb = L.lib().avd_apg_stats_bytes(B, per)
    if nb < 0:
        raise ValueError(f"apg_guidance needs >= 2 elements per sample (got {per}) and 1 <= B <= 65535")
    stats = torch.empty(nb, dtype=torch.uint8, device=ec.device)
    ctl = L.ApgControl(r, eta_p, beta, L.ptr(momentum_buf), stats.data_ptr(), nb)
    out = torch.empty_like(ec)
    L.check(L.lib().avd_apg_guidance_f32(ec.data_ptr(), en.data_ptr(), g.data_ptr(), 0.0, C.byref(ctl), out.data_ptr(), B, per, _st(out)))
    if return_coef:
        coef = stats[nb - 16 * B:].view(torch.float32).view(B, 4)      # the coefficient slot ends the scratch: (s, k, w, g)
        return out, (coef[:, 0].clone(), coef[:, 1].clone(), coef[:, 2].clone())
    return out


def window_dims(shape) -> tuple:
    """(outer, L, inner) of a window batch for ``avd_window_consensus_f32``: a video latent [N,C,T,H,W] slides along T, an audio latent
    [N,Ca,F] along F."""
    shape = tuple(int(s) for s in shape)
    if len(shape) == 5:
        return shape[1], shape[2], shape[3] * shape[4]
    if len(shape) == 3:
        return shape[1], shape[2], 1
    raise ValueError(f"a window batch is a video latent [N,C,T,H,W] or an audio latent [N,Ca,F], got shape {shape}")


def consensus_weights(weights, L_: int) -> Tensor:
    """The [L] per-position weight table of ``window_consensus`` as a CPU fp32 tensor: None = uniform; checked to be of shape (L,),
    finite and > 0 (the kernel divides by their sum unclamped)."""
    if weights is None:
        return torch.ones(L_, dtype=torch.float32)
    w = torch.as_tensor(weights).detach().to("cpu", torch.float32)
    if tuple(w.shape) != (L_,):
        raise ValueError(f"consensus weights have shape {tuple(w.shape)}, expected ({L_},): one weight per window position")
    if not bool((torch.isfinite(w) & (w > 0)).all()):
        raise ValueError("consensus weights must be finite and > 0")
    return w.contiguous()


def window_consensus(z: Tensor, hop: int, weights: Optional[Tensor] = None) -> Tensor:
    """Latent window consensus, in place (``avd_window_consensus_f32``, contract in include/avdiff_hip.h): ``z`` is a batch of N
    consecutive windows of one canvas, window k at canvas positions k*hop .. k*hop + L - 1 of the sliding axis (T of a video latent
    [N,C,T,H,W], F of an audio latent [N,Ca,F]); every canvas position under several windows is replaced in each of them by their
    weighted mean, a position under one window keeps its bits.  ``weights`` [L] > 0, None = uniform (MultiDiffusion's choice).
    Returns ``z``."""
    if not z.is_cuda:
        raise L.AvdError(f"z is on {z.device}: the HIP hot path needs ROCm device tensors (no CPU fallback)")
    if z.dtype != torch.float32 or not z.is_contiguous():
        raise TypeError("window_consensus works in place: z must be a contiguous float32 tensor")
    outer, L_, inner = window_dims(z.shape)
    hop = int(hop)
    if hop <= 0:
        raise ValueError(f"hop must be > 0, got {hop}")
    if z.numel() == 0:
        raise ValueError(f"empty window batch {tuple(z.shape)}")
    w = torch.ones(L_, dtype=torch.float32, device=z.device) if weights is None else consensus_weights(weights, L_).to(z.device)
    L.check(L.lib().avd_window_consensus_f32(z.data_ptr(), w.data_ptr(), z.shape[0], outer, L_, hop, inner, _st(z)))
    return z


def gaussian_noise(seed: int, sample_offset: int, t_now: Tensor, shape) -> Tensor:
    """The seeded normal stream of the DDIM eta > 0 noise (avd_gaussian_noise_f32; contract in include/avdiff_hip.h): a
    float32 tensor of ``shape`` = (B, ...) whose row b holds sample ``sample_offset + b``'s normals at timestep ``t_now[b]``,
    element e of the row in row-major order of shape[1:].  The same values the seeded DenoiseEngine draws inside its step, so the
    result can be passed as ``noise`` to ``schedule_utils.ddim_step`` / ``DenoiseEngine.step``.  ``t_now``: int [B] (moved to the
    current ROCm device if it is not on one)."""
    shape = _positive_shape(shape, "shape must be (B, ...) with positive sizes")
    key = noise_key(seed, sample_offset)
    dev = t_now.device if t_now.is_cuda else torch.device("cuda", torch.cuda.current_device())
    tn = L.dev_i64(t_now, dev)
    B = shape[0]
    if tn.numel() != B:
        raise ValueError(f"t_now has {tn.numel()} entries, shape asks for {B} samples")
    out = torch.empty(shape, device=dev, dtype=torch.float32)
    L.check(L.lib().avd_gaussian_noise_f32(C.byref(key), tn.data_ptr(), out.data_ptr(), B, out.numel() // B, _st(out)))
    return out


def check_canvas_keying(shape, hop, window_offset: int = 0) -> int:
    """The limits of the canvas-keyed noise stream (include/avdiff_hip.h, "canvas-keyed noise") for a window batch ``shape`` whose
    window 0 has the global index ``window_offset``: an integer hop >= 1, every canvas position below 2**32 and one position's slice
    below 2**34 elements.  Returns hop as an int."""
    outer, L_, inner = window_dims(shape)
    if isinstance(hop, bool) or not isinstance(hop, int) or hop < 1:
        raise ValueError(f"canvas_hop must be an int >= 1 (latent positions from one window to the next), got {hop!r}")
    if hop >= 2 ** 31:
        raise ValueError(f"canvas_hop {hop} does not fit the C ABI's int")
    N = int(shape[0])
    if N < 1 or (window_offset + N - 1) * hop + L_ > 2 ** 32:
        raise ValueError(f"(window_offset {window_offset} + N {N} - 1) * hop {hop} + L {L_} exceeds the stream's 2**32 canvas positions")
    if outer * inner >= 2 ** 34:
        raise ValueError(f"one canvas position holds outer * inner = {outer * inner} elements, the stream keys < 2**34")
    return hop


def canvas_noise(seed: int, t_now: Tensor, shape, hop: int, window_offset: int = 0, out: Optional[Tensor] = None) -> Tensor:
    """The canvas-keyed form of the seeded normal stream (avd_canvas_noise_f32; contract in include/avdiff_hip.h, "canvas-keyed
    noise"): a float32 tensor of ``shape``, a batch of N consecutive windows of one canvas ([N,C,T,H,W] video, [N,Ca,F] audio), ``hop``
    positions apart along the sliding axis, window 0 at global window index ``window_offset``.  Element (o, l, i) of window b holds
    the normal of canvas position p = (window_offset + b)*hop + l: the value ``gaussian_noise(seed, 0, t, (P, outer, inner))`` has at
    [p, o, i] — every window covering p gets the same bits.  The values a canvas-keyed DenoiseEngine draws inside its step, so the
    result can be passed as ``noise`` to an unseeded engine's ``step``.  ``t_now``: int [N] (moved to the current ROCm device if it
    is not on one).  ``out``: a contiguous float32 device tensor of ``shape`` to fill instead of a new one."""
    outer, L_, inner = window_dims(shape)
    shape = _positive_shape(shape)
    key = noise_key(seed, window_offset)
    hop = check_canvas_keying(shape, hop, window_offset)
    _check_out(out, shape)
    dev = out.device if out is not None else (t_now.device if t_now.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    tn = L.dev_i64(t_now, dev)
    if tn.numel() != shape[0]:
        raise ValueError(f"t_now has {tn.numel()} entries, shape asks for {shape[0]} windows")
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.float32)
    L.check(L.lib().avd_canvas_noise_f32(C.byref(key), tn.data_ptr(), out.data_ptr(), shape[0], outer, L_, hop, inner, _st(out)))
    return out


def slot_tables(t_now: Tensor, t_prev: Tensor, B: int, S: int, device: torch.device, t_last: Optional[Tensor] = None):
    """The [B, S] timestep tables of the slot entries (include/avdiff_hip.h, "slot timesteps") as contiguous int64 device tensors,
    after the shape check every caller shares: [t_now, t_prev], with ``t_last`` (the multistep solver's third table) behind them when
    it is given."""
    out = []
    for name, t in (("t_now", t_now), ("t_prev", t_prev)) + ((("t_last", t_last),) if t_last is not None else ()):
        t = torch.as_tensor(t)
        if t.is_floating_point() or t.dtype == torch.bool:
            raise TypeError(f"{name} must hold integer timesteps, got {t.dtype}")
        if tuple(t.shape) != (B, S):
            raise ValueError(f"{name} has shape {tuple(t.shape)}, expected [B, S] = {(B, S)}: one timestep per sample and slot")
        out.append(L.dev_i64(t, device))
    return out


def slot_key(seed: int, first: int = 0, stride: int = 1, cursor: Optional[Tensor] = None,
             device: Optional[torch.device] = None) -> "L.SlotKey":
    """avd_slot_key (include/avdiff_hip.h, "clip-keyed slot noise") after the checks its users share: 0 <= seed < 2**64, an int
    ``first`` with |first| < 2**32 (the clip slot of slot 0 of sample 0; negative slots wrap), an int ``stride`` in [1, 2**31) (clip
    slots from one sample to the next) and ``cursor`` None or one int32 in device memory (on ``device`` when that is given), whose
    value, read at each launch and clamped at 0, is added to ``first``.  The struct holds the cursor's raw pointer: keep it alive."""
    noise_key(seed, 0)
    if isinstance(first, bool) or not isinstance(first, int) or abs(first) >= 2 ** 32:
        raise ValueError(f"clip_first must be an int with |first| < 2**32 (the clip slot of slot 0 of sample 0), got {first!r}")
    if isinstance(stride, bool) or not isinstance(stride, int) or not 1 <= stride < 2 ** 31:
        raise ValueError(f"clip_stride must be an int in [1, 2**31) (clip slots from one sample to the next), got {stride!r}")
    if cursor is not None:
        if not isinstance(cursor, Tensor):
            raise ValueError("a cursor is one int32 in device memory (a 1-element int32 tensor on the buffers' device)")
        _cursor(cursor, cursor.device if device is None else device)
    return L.SlotKey(seed, first, stride, L.ptr(cursor))


def slot_noise(seed: int, t_now: Tensor, shape, slot_len: int, first: int = 0, stride: Optional[int] = None,
               cursor: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """The clip-keyed normals of the slot entries' eta > 0 noise (avd_slot_noise_f32; contract in include/avdiff_hip.h, "clip-keyed
    slot noise"): a float32 tensor of ``shape`` ([B,C,T,H,W] video, [B,Ca,F] audio).  ``t_now``: int [B, S]; sliding position l is in
    slot min(l // slot_len, S - 1) and sits on clip position ((first + max(*cursor, 0) + b*stride) * slot_len + l) mod 2**32, whose
    normal at the slot's timestep it holds: the values ``DenoiseEngine.step_slots(clip_first=...)`` draws inside its step, so the
    result can be passed as ``noise`` to ``ddim_step_slots`` / ``dpmpp_2m_sde_step_slots`` or, with a uniform table, to an unseeded
    engine's ``step``.  ``stride`` None = S; ``cursor``: see ``slot_key``; ``out``: a contiguous float32 device tensor of ``shape``
    to fill instead of a new one."""
    outer, L_, inner = window_dims(shape)
    shape = _positive_shape(shape)
    t_now, S = _slot_table(t_now, "t_now", shape[0], L_, slot_len)
    if outer * inner >= 2 ** 34:
        raise ValueError(f"one clip position holds outer * inner = {outer * inner} elements, the stream keys < 2**34")
    _check_out(out, shape)
    dev = out.device if out is not None else (t_now.device if t_now.is_cuda else torch.device("cuda", torch.cuda.current_device()))
    key = slot_key(seed, first, S if stride is None else stride, cursor, dev)
    tn = L.dev_i64(t_now, dev)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.float32)
    L.check(L.lib().avd_slot_noise_f32(C.byref(key), tn.data_ptr(), out.data_ptr(), shape[0], outer, L_, S, slot_len, inner, _st(out)))
    return out


SLOT_LEAVE = L.SLOT_LEAVE      # a tau entry of clip_guide_slots that leaves its slot as z (AVD_SLOT_LEAVE)


def _clip_canvas(t: Tensor, name: str, like: Optional[Tensor] = None) -> Tensor:
    if not (isinstance(t, Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() in (2, 4)):
        raise ValueError(f"{name} must be a contiguous float32 device canvas [C, P, H, W] (video) or [Ca, P] (audio)")
    if like is not None and (tuple(t.shape) != tuple(like.shape) or t.device != like.device):
        raise ValueError(f"{name} shape {tuple(t.shape)} must be the known canvas's {tuple(like.shape)}, on its device")
    return t


def clip_guide(known: Tensor, mask: Optional[Tensor], seed: int, first: int = 0, stride: int = 1, cursor: Optional[Tensor] = None,
               shape=None) -> "L.ClipGuide":
    """avd_clip_guide (include/avdiff_hip.h, "clip-keyed latent guide") after the checks its users share: ``known`` the clean clip
    canvas, contiguous float32 on the device, [C, P, H, W] (video) or [Ca, P] (audio); ``mask`` None (1 everywhere) or a canvas of the
    same shape with values in [0, 1] (what ``sampler.canvas_frame_mask`` returns); ``seed`` / ``first`` / ``stride`` / ``cursor`` as
    ``slot_key``.  ``shape``: the batch the guide will ride with ([B,C,T,H,W] / [B,Ca,F]), whose channel and spatial sizes must be the
    canvas's.  The struct holds raw pointers: keep the tensors alive."""
    known = _clip_canvas(known, "known")
    if mask is not None:
        _clip_canvas(mask, "mask", known)
    if known.shape[1] < 1 or known.shape[1] > 2 ** 32:
        raise ValueError(f"the known canvas holds {known.shape[1]} clip positions, a clip guide takes 1 .. 2**32")
    if shape is not None:
        shape = tuple(int(s) for s in shape)
        if len(shape) != known.dim() + 1 or shape[1] != known.shape[0] or tuple(shape[3:]) != tuple(known.shape[2:]):
            raise ValueError(f"a known canvas of shape {tuple(known.shape)} does not guide a batch of shape {shape}: the channels and "
                             "the spatial sizes must agree")
    k = slot_key(seed, first, stride, cursor, known.device)
    return L.ClipGuide(known.data_ptr(), L.ptr(mask), known.shape[1], k.seed, k.first, k.stride, k.cursor)


def clip_guide_slots(known: Tensor, tau: Tensor, alpha_bar: Tensor, z: Tensor, mask: Optional[Tensor] = None, *, slot_len: int,
                     seed: int, first: int = 0, stride: Optional[int] = None, cursor: Optional[Tensor] = None,
                     everywhere: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """The clip-keyed latent guide's blend per slot (avd_clip_guide_slots_f32; contract in include/avdiff_hip.h, "clip-keyed latent
    guide"): ``z`` is a batch [B,C,T,H,W] (video) or [B,Ca,F] (audio), ``tau`` int [B, S]; sliding position l of sample b is in slot
    min(l // slot_len, S - 1) and sits on clip position p = (first + max(*cursor, 0) + b*stride) * slot_len + l (signed, not wrapped).
    Where 0 <= p < P the result is blend(mask[:, p], q_p(tau[b, s]), z) with q_p = sqrt(a) known[:, p] + sqrt(1 - a) n_k(p), n_k the
    canvas-keyed known noise of ``seed`` at position p; elsewhere, and in every slot whose tau is ``SLOT_LEAVE``, it is ``z`` bit for
    bit.  ``mask`` None = 1 everywhere; ``everywhere`` reads the mask as 1 on every in-canvas position (SDEdit's start).  ``stride``
    None = S.  ``out``: a contiguous float32 tensor of z's shape to write — ``z`` itself for an in-place call, which touches only the
    slots that are not left — None allocates one."""
    known = _clip_canvas(known, "known")
    z = L.dev_f32(z, "z")
    shape = tuple(z.shape)
    outer, L_, inner = window_dims(shape)
    tau, S = _slot_table(tau, "tau", shape[0], L_, slot_len)
    m = None if mask is None else L.dev_f32(mask, "mask")
    g = clip_guide(known, m, seed, first, S if stride is None else stride, cursor, shape)
    _check_out(out, shape, z)
    if out is None:
        out = torch.empty_like(z)
    tn = L.dev_i64(tau, z.device)
    ab = _alpha_bar(alpha_bar, z.device)
    L.check(L.lib().avd_clip_guide_slots_f32(C.byref(g), tn.data_ptr(), ab.data_ptr(), ab.numel(), 1 if everywhere else 0, z.data_ptr(),
                                             out.data_ptr(), shape[0], outer, L_, S, slot_len, inner, _st(z)))
    return out


# ---- clip batch keying (include/avdiff_hip.h, "clip batch keying"): the batch is K queues, each under its own seeds and canvases ----
def queue_seeds(seeds, queues: Optional[int] = None, device=None) -> Tensor:
    """The K per-queue seeds of a clip batch as ``clip_seeds``' int64 tensor on ``device`` (None: the CPU): K ints, or that tensor
    already made (a loop uploads it once), which must then be int64 [K] on ``device``.  ``queues`` None takes K from ``seeds``."""
    if isinstance(seeds, Tensor):
        d = None if device is None else torch.device(device)      # an index-free device names the current one
        if not (seeds.dtype == torch.int64 and seeds.is_contiguous() and seeds.dim() == 1 and seeds.numel() >= 1 and
                (queues is None or seeds.numel() == queues) and
                (d is None or (seeds.device.type == d.type and (d.index is None or seeds.device.index == d.index)))):
            raise ValueError(f"a seeds tensor must be clip_seeds' int64 [{'K' if queues is None else queues}] on {device or 'the CPU'}, got "
                             f"{seeds.dtype} {tuple(seeds.shape)} on {seeds.device}")
        return seeds
    if isinstance(seeds, (str, bytes)) or not hasattr(seeds, "__len__"):
        raise ValueError(f"seeds must be a sequence of ints, one per queue, got {seeds!r}")
    return clip_seeds(seeds, len(seeds) if queues is None else queues, device)


def _seed_ints(seeds: Tensor):
    """the unsigned values of a ``clip_seeds`` tensor"""
    return [s + 2 ** 64 if s < 0 else s for s in seeds.tolist()]


def clip_queues(queues: int, B: int, step_seeds: Optional[Tensor] = None, guide_seeds: Optional[Tensor] = None) -> "L.ClipQueues":
    """avd_clip_queues for a batch of ``B`` samples: ``queues`` = K >= 1 must divide B; the seeds are ``queue_seeds`` tensors on the
    buffers' device, or None where the call does not read them.  The struct holds raw pointers: keep the tensors alive."""
    if isinstance(queues, bool) or not isinstance(queues, int) or queues < 1 or B % queues:
        raise ValueError(f"queues {queues!r} must be an int >= 1 that divides the batch {B}")
    for name, s in (("step_seeds", step_seeds), ("guide_seeds", guide_seeds)):
        if s is not None and not (isinstance(s, Tensor) and s.is_cuda and s.dtype == torch.int64 and s.is_contiguous() and
                                  tuple(s.shape) == (queues,)):
            raise ValueError(f"{name} must be queue_seeds' int64 [{queues}] on the device")
    return L.ClipQueues(queues, L.ptr(step_seeds), L.ptr(guide_seeds))


def slot_noise_clips(seeds, t_now: Tensor, shape, slot_len: int, first: int = 0, stride: Optional[int] = None,
                     cursor: Optional[Tensor] = None, out: Optional[Tensor] = None) -> Tensor:
    """``slot_noise`` for a FIFO clip batch (avd_slot_noise_clips_f32; contract in include/avdiff_hip.h, "clip batch keying"): ``shape``
    is K = len(seeds) queues of B / K samples; sample b is sample b' = b % (B / K) of queue k = b // (B / K), sits on clip position
    ((first + max(*cursor, 0) + b'*stride) * slot_len + l) mod 2**32 and draws under ``seeds[k]``.  ``seeds``: K ints, or the int64
    device tensor ``queue_seeds`` makes of them.  Everything else as ``slot_noise``; the values
    ``DenoiseEngine.step_slots(clip_queues=K, clip_seeds=seeds)`` draws inside its step.
    A device ``out`` (or none) takes the one launch.  A CPU ``out`` takes the torch statement below, which is the reference: per queue
    ``slot_noise`` under the queue's seed on the queue's slice of ``t_now``."""
    shape = _positive_shape(shape)
    statement = out is not None and isinstance(out, Tensor) and not out.is_cuda
    dev = None if statement else (out.device if out is not None else
                                  (t_now.device if isinstance(t_now, Tensor) and t_now.is_cuda else torch.device("cuda", torch.cuda.current_device())))
    seeds = queue_seeds(seeds, None, dev)
    K, B = seeds.numel(), shape[0]
    if B % K:
        raise ValueError(f"{K} seeds for a batch of {B}: the queues must divide the batch")
    Bq = B // K
    if statement:
        if tuple(out.shape) != shape or out.dtype != torch.float32:
            raise ValueError(f"out must be a float32 tensor of shape {shape}")
        t_now = torch.as_tensor(t_now)
        for k, s in enumerate(_seed_ints(seeds)):
            sl = slice(k * Bq, (k + 1) * Bq)
            out[sl] = slot_noise(s, t_now[sl], (Bq,) + shape[1:], slot_len, first, stride, cursor).to(out.device)
        return out
    outer, L_, inner = window_dims(shape)
    t_now, S = _slot_table(t_now, "t_now", B, L_, slot_len)
    if outer * inner >= 2 ** 34:
        raise ValueError(f"one clip position holds outer * inner = {outer * inner} elements, the stream keys < 2**34")
    _check_out(out, shape)
    key = slot_key(0, first, S if stride is None else stride, cursor, dev)      # the seed is not read: the queues' are
    cq = clip_queues(K, B, step_seeds=seeds)
    tn = L.dev_i64(t_now, dev)
    if out is None:
        out = torch.empty(shape, device=dev, dtype=torch.float32)
    L.check(L.lib().avd_slot_noise_clips_f32(C.byref(key), C.byref(cq), tn.data_ptr(), out.data_ptr(), B, outer, L_, S, slot_len, inner,
                                             _st(out)))
    return out


def stack_clip_canvases(canvases, name: str = "known") -> Tensor:
    """K clip canvases of one shape — a sequence of tensors, or one stacked tensor [K, C, P, H, W] (video) / [K, Ca, P] (audio) — as
    the stacked tensor; ValueError for none, for differing shapes and for a wrong rank"""
    if isinstance(canvases, Tensor):
        t = canvases
    else:
        cs = list(canvases)
        if not cs or any(not isinstance(c, Tensor) or c.shape != cs[0].shape for c in cs):
            raise ValueError(f"the {name} canvases must be K >= 1 tensors of one shape (the clips run in lockstep), got "
                             f"{[tuple(c.shape) if isinstance(c, Tensor) else c for c in cs]}")
        t = torch.stack(cs)
    if t.dim() not in (3, 5) or t.shape[0] < 1:
        raise ValueError(f"the {name} canvases must stack to [K, C, P, H, W] (video) or [K, Ca, P] (audio), got {tuple(t.shape)}")
    return t


def clip_guide_slots_clips(known: Tensor, tau: Tensor, alpha_bar: Tensor, z: Tensor, masks: Optional[Tensor] = None, *, slot_len: int,
                           seeds, first: int = 0, stride: Optional[int] = None, cursor: Optional[Tensor] = None,
                           everywhere: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """``clip_guide_slots`` for a FIFO clip batch (avd_clip_guide_slots_clips_f32; contract in include/avdiff_hip.h, "clip batch
    keying"): ``known`` holds K canvases, [K, C, P, H, W] / [K, Ca, P] (``masks`` None or the same shape), ``z`` is K queues of B / K
    samples; sample b' of queue k sits on clip position (first + max(*cursor, 0) + b'*stride) * slot_len + l, reads canvas k there
    and takes the known noise of ``seeds[k]``.  ``seeds``: K ints or ``queue_seeds``' device tensor.  Everything else as
    ``clip_guide_slots``: one in-place call (``out=z``) with ``SLOT_LEAVE`` everywhere but each queue's tail slot puts all K entering
    slots on their forward paths.
    A device ``z`` takes the one launch.  A CPU ``z`` takes the torch statement below, which is the reference: per queue
    ``clip_guide_slots`` with the queue's canvas, mask and seed on the queue's slices of ``tau`` and ``z``.  ``clip_guide_slots``
    launches on a device, so where there is one the slices go to the current device and the result comes back to ``z``'s."""
    known = stack_clip_canvases(known)
    if masks is not None:
        masks = stack_clip_canvases(masks, "mask")
        if masks.shape != known.shape:
            raise ValueError(f"masks shape {tuple(masks.shape)} must be the known canvases' {tuple(known.shape)}")
    if not isinstance(z, Tensor) or z.dim() != known.dim():
        raise ValueError("z must be a batch [B,C,T,H,W] (video) or [B,Ca,F] (audio) of the canvases' rank")
    K, B = known.shape[0], z.shape[0]
    seeds = queue_seeds(seeds, K, z.device if z.is_cuda else None)
    if B % K:
        raise ValueError(f"{K} canvases for a batch of {B}: the queues must divide the batch")
    Bq = B // K
    if not z.is_cuda:
        tau = torch.as_tensor(tau)
        res = torch.empty_like(z) if out is None else out
        on = (lambda t: t.cuda().contiguous()) if torch.cuda.is_available() else (lambda t: t)
        for k, s in enumerate(_seed_ints(seeds)):
            sl = slice(k * Bq, (k + 1) * Bq)
            r = clip_guide_slots(on(known[k]), tau[sl], alpha_bar, on(z[sl]), None if masks is None else on(masks[k]), slot_len=slot_len,
                                 seed=s, first=first, stride=stride, cursor=cursor, everywhere=everywhere)
            res[sl] = r.to(res.device)
        return res
    z = L.dev_f32(z, "z")
    shape = tuple(z.shape)
    outer, L_, inner = window_dims(shape)
    tau, S = _slot_table(tau, "tau", B, L_, slot_len)
    if not (known.is_cuda and known.dtype == torch.float32 and known.is_contiguous() and known.device == z.device):
        raise ValueError("known must be contiguous float32 device canvases [K, C, P, H, W] (video) or [K, Ca, P] (audio) on z's device")
    if masks is not None and not (masks.is_cuda and masks.dtype == torch.float32 and masks.is_contiguous() and masks.device == z.device):
        raise ValueError("masks must be contiguous float32 device canvases of the known canvases' shape, on z's device")
    g = clip_guide(known[0], None if masks is None else masks[0], 0, first, S if stride is None else stride, cursor, shape)
    cq = clip_queues(K, B, guide_seeds=seeds)
    _check_out(out, shape, z)
    if out is None:
        out = torch.empty_like(z)
    tn = L.dev_i64(tau, z.device)
    ab = _alpha_bar(alpha_bar, z.device)
    L.check(L.lib().avd_clip_guide_slots_clips_f32(C.byref(g), C.byref(cq), tn.data_ptr(), ab.data_ptr(), ab.numel(), 1 if everywhere else 0,
                                                   z.data_ptr(), out.data_ptr(), B, outer, L_, S, slot_len, inner, _st(z)))
    return out


def _slot_step_noise(eta: float, noise: Optional[Tensor], x_t: Tensor, what: str) -> Optional[Tensor]:
    """the explicit noise of the slot mirrors: required when eta > 0 (``slot_noise`` gives the fused step's normals), not read at 0"""
    if isinstance(eta, bool) or not isinstance(eta, (int, float)) or not eta >= 0:
        raise ValueError(f"eta must be a number >= 0, got {eta!r}")
    if eta == 0:
        return None
    if noise is None:
        raise ValueError(f"{what}: eta > 0 needs `noise` (slot_noise gives the clip-keyed normals the fused step draws)")
    nz = L.dev_f32(noise, "noise")
    if nz.shape != x_t.shape:
        raise RuntimeError("noise must have the shape of x_t")
    return nz


def ddim_step_slots(x_t: Tensor, t_now: Tensor, t_prev: Tensor, eps_hat: Tensor, alpha_bar: Tensor, slot_len: int, eta: float = 0.0,
                    noise: Optional[Tensor] = None) -> Tensor:
    """The elementwise mirror of the slot form of the fused update (include/avdiff_hip.h, "slot timesteps"): ``x_t`` and
    ``eps_hat`` are latents ([B,C,T,H,W] video, [B,Ca,F] audio), ``t_now`` / ``t_prev`` int [B, S]; sliding position l is in slot
    min(l // slot_len, S - 1).  Every slot takes ``ddim_step`` (avd_ddim_step_f32) with its pair, one launch per distinct pair of the
    tables; a slot with t_prev == t_now keeps ``x_t`` bit for bit (the hold).
    ``eta`` > 0 ("clip-keyed slot noise") needs ``noise``, a float32 tensor of x_t's shape — ``slot_noise`` gives the normals the
    fused step draws — and every stepping slot takes its pair's sigma(eta) times it; at the default 0 ``noise`` is not read."""
    x_t = L.dev_f32(x_t, "x_t")
    eps_hat = L.dev_f32(eps_hat, "eps_hat")
    if eps_hat.shape != x_t.shape:
        raise RuntimeError("eps_hat must have the shape of x_t")
    nz = _slot_step_noise(eta, noise, x_t, "ddim_step_slots")
    _, L_, _ = window_dims(x_t.shape)
    B = x_t.shape[0]
    S = _check_slot_len(slot_len, L_)
    tn, tp = slot_tables(t_now, t_prev, B, S, x_t.device)
    slot = torch.clamp(torch.arange(L_, device=x_t.device) // slot_len, max=S - 1)
    view = (B, 1, L_) + (1,) * (x_t.dim() - 3)
    tn_l, tp_l = tn[:, slot].view(view), tp[:, slot].view(view)      # the pair of every sliding position
    out = x_t.clone()
    for a, p in sorted({(int(a), int(p)) for a, p in zip(tn.reshape(-1).tolist(), tp.reshape(-1).tolist())}):
        if a == p:
            continue
        full = ddim_step(x_t, torch.full((B,), a), torch.full((B,), p), eps_hat, alpha_bar, float(eta) if nz is not None else 0.0, nz)
        out = torch.where((tn_l == a) & (tp_l == p), full, out)
    return out


def _check_slot_len(slot_len, L_: int) -> int:
    if isinstance(slot_len, bool) or not isinstance(slot_len, int) or slot_len < 1 or slot_len > L_:
        raise ValueError(f"slot_len must be an int in [1, {L_}], got {slot_len!r}")
    return L_ // slot_len


def dpmpp_2m_step_slots(x_t: Tensor, eps_hat: Tensor, x0_hist: Tensor, t_last: Tensor, t_now: Tensor, t_prev: Tensor,
                        alpha_bar: Tensor, slot_len: int) -> Tensor:
    """The elementwise mirror of the slot form of the fused DPM-Solver++(2M) update (include/avdiff_hip.h, "slot timesteps"), built as
    ``ddim_step_slots``: ``t_last`` / ``t_now`` / ``t_prev`` are int [B, S] tables and every slot takes ``dpmpp_2m_step``
    (avd_dpmpp_2m_step_f32) with its triple, one launch per distinct triple of the tables, kept on that triple's slots in the returned
    latent and in ``x0_hist`` (updated in place, as by ``dpmpp_2m_step``).  A slot with t_prev == t_now keeps ``x_t`` and its
    history bit for bit (the hold)."""
    x_t = L.dev_f32(x_t, "x_t")
    eps_hat = L.dev_f32(eps_hat, "eps_hat")
    if eps_hat.shape != x_t.shape:
        raise RuntimeError("eps_hat must have the shape of x_t")
    if not (x0_hist.is_cuda and x0_hist.dtype == torch.float32 and x0_hist.is_contiguous() and x0_hist.shape == x_t.shape):
        raise RuntimeError("x0_hist must be a contiguous float32 device tensor of x_t's shape (it is updated in place)")
    _, L_, _ = window_dims(x_t.shape)
    B = x_t.shape[0]
    S = _check_slot_len(slot_len, L_)
    tn, tp, tl = slot_tables(t_now, t_prev, B, S, x_t.device, t_last)
    slot = torch.clamp(torch.arange(L_, device=x_t.device) // slot_len, max=S - 1)
    view = (B, 1, L_) + (1,) * (x_t.dim() - 3)
    tl_l, tn_l, tp_l = (t[:, slot].view(view) for t in (tl, tn, tp))      # the triple of every sliding position
    out, hist = x_t.clone(), x0_hist.clone()
    for u, a, p in sorted(set(zip(tl.reshape(-1).tolist(), tn.reshape(-1).tolist(), tp.reshape(-1).tolist()))):
        if a == p:
            continue
        h = x0_hist.clone()
        full = dpmpp_2m_step(x_t, eps_hat, h, torch.full((B,), u), torch.full((B,), a), torch.full((B,), p), alpha_bar)
        on = (tl_l == u) & (tn_l == a) & (tp_l == p)
        out, hist = torch.where(on, full, out), torch.where(on, h, hist)
    x0_hist.copy_(hist)
    return out


def dpmpp_2m_sde_step_slots(x_t: Tensor, eps_hat: Tensor, x0_hist: Tensor, t_last: Tensor, t_now: Tensor, t_prev: Tensor,
                            alpha_bar: Tensor, slot_len: int, eta: float, noise: Optional[Tensor] = None) -> Tensor:
    """``dpmpp_2m_step_slots`` for the solver's SDE form (include/avdiff_hip.h, "clip-keyed slot noise"): every slot takes
    ``dpmpp_2m_sde_step`` (avd_dpmpp_2m_sde_step_f32) with its triple, ``eta`` and the explicit ``noise`` (float32, x_t's shape;
    ``slot_noise`` gives the normals the fused step draws; required when eta > 0).  A held slot keeps ``x_t`` and its history bit for
    bit; at eta == 0 ``noise`` is not read and the result has ``dpmpp_2m_step_slots``'s bits."""
    x_t = L.dev_f32(x_t, "x_t")
    eps_hat = L.dev_f32(eps_hat, "eps_hat")
    if eps_hat.shape != x_t.shape:
        raise RuntimeError("eps_hat must have the shape of x_t")
    if not (x0_hist.is_cuda and x0_hist.dtype == torch.float32 and x0_hist.is_contiguous() and x0_hist.shape == x_t.shape):
        raise RuntimeError("x0_hist must be a contiguous float32 device tensor of x_t's shape (it is updated in place)")
    nz = _slot_step_noise(eta, noise, x_t, "dpmpp_2m_sde_step_slots")
    _, L_, _ = window_dims(x_t.shape)
    B = x_t.shape[0]
    S = _check_slot_len(slot_len, L_)
    tn, tp, tl = slot_tables(t_now, t_prev, B, S, x_t.device, t_last)
    slot = torch.clamp(torch.arange(L_, device=x_t.device) // slot_len, max=S - 1)
    view = (B, 1, L_) + (1,) * (x_t.dim() - 3)
    tl_l, tn_l, tp_l = (t[:, slot].view(view) for t in (tl, tn, tp))      # the triple of every sliding position
    out, hist = x_t.clone(), x0_hist.clone()
    for u, a, p in sorted(set(zip(tl.reshape(-1).tolist(), tn.reshape(-1).tolist(), tp.reshape(-1).tolist()))):
        if a == p:
            continue
        h = x0_hist.clone()
        full = dpmpp_2m_sde_step(x_t, eps_hat, h, torch.full((B,), u), torch.full((B,), a), torch.full((B,), p), alpha_bar,
                                 float(eta) if nz is not None else 0.0, nz)
        on = (tl_l == u) & (tn_l == a) & (tp_l == p)
        out, hist = torch.where(on, full, out), torch.where(on, h, hist)
    x0_hist.copy_(hist)
    return out


def _queue_dims(shape, slot_len) -> tuple:
    """(outer, S, inner) of a queue of layout ``shape`` whose sliding length is S slots of ``slot_len`` positions"""
    outer, L_, inner = window_dims(shape)
    if isinstance(slot_len, bool) or not isinstance(slot_len, int) or slot_len < 1 or L_ % slot_len:
        raise ValueError(f"slot_len must be an int >= 1 that divides the sliding length {L_}, got {slot_len!r}")
    return outer, L_ // slot_len, inner


def _check_clip_slot(c, t, slot_len: int, n_out: Optional[int] = None, at: str = "") -> None:
    """the clip slot and timestep of a tail draw: ints >= 0, every slot the draw can name (``c`` alone, or ``c0`` .. ``c0 + n_out - 1``
    off a cursor) inside the stream's 2**32 canvas positions"""
    for name, v in (("c" if n_out is None else "c0", c), ("t", t)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"{name} must be an int >= 0{at}, got {v!r}")
    if n_out is None and (c + 1) * slot_len > 2 ** 32:
        raise ValueError(f"(c {c} + 1) * slot_len {slot_len} exceeds the stream's 2**32 canvas positions")
    if n_out is not None and (c + n_out) * slot_len > 2 ** 32:
        raise ValueError(f"(c0 {c} + n_out {n_out}) * slot_len {slot_len} exceeds the stream's 2**32 canvas positions")


def _check_like(x, name: str, ref: Tensor, of: str = "z's", on: str = "z's device") -> None:
    if not (isinstance(x, Tensor) and x.dtype == torch.float32 and x.is_contiguous() and x.shape == ref.shape and x.device == ref.device):
        raise ValueError(f"{name} must be a contiguous float32 tensor of {of} shape {tuple(ref.shape)} on {on}")


def _check_rider(z: Tensor, name: str, x: Optional[Tensor], x_out: Optional[Tensor], out_like_z: bool = True) -> None:
    """a rider pair of a queue move: ``x_out`` goes with ``x``, and both are contiguous float32 tensors of z's shape on z's device"""
    if x is None and x_out is not None:
        raise ValueError(f"{name}_out goes with {name}")
    if x is not None:
        _check_like(x, name, z)
    if x_out is not None:
        _check_like(x_out, f"{name}_out", *((z,) if out_like_z else (x, f"{name}'s", "its device")))


def fifo_shift(z: Tensor, c: int, seed: int, t: int, slot_len: int, hist: Optional[Tensor] = None, hist_out: Optional[Tensor] = None,
               guide: Optional[dict] = None):
    """The queue step of FIFO diagonal denoising (avd_fifo_shift_f32; contract in include/avdiff_hip.h, "FIFO queue shift"): ``z``
    ([B,C,T,H,W] video, [B,Ca,F] audio, sliding length L = S * slot_len) is a queue of B * S slots.  Returns (z_out, popped): z_out
    slot q = z slot q + 1 across sample boundaries, popped = z slot 0 ([C, slot_len, H, W] or [Ca, slot_len]), and the tail slot of
    z_out holds the seeded normals of clip slot ``c`` at timestep ``t`` — ``canvas_noise(seed, [t], one slot's shape, slot_len,
    window_offset=c)`` bit for bit.
    With ``hist`` (float32 on z's device, z's shape: a multistep solver's per-element history, ``x0_hist`` of the slot form of
    DPM-Solver++(2M)) the same launch carries it along with its slot (avd_fifo_shift_hist_f32) and the result is (z_out, popped,
    hist_out): hist_out slot q = hist slot q + 1, zeros in the tail slot, the head's history dropped.  ``hist_out``: a buffer to
    write it to (hist's shape, not overlapping it), None allocates one.
    ``guide`` (avd_fifo_shift_guided_f32; "clip-keyed latent guide") = {"known":, "alpha_bar":, "seed":, "mask": None, "everywhere":
    False}, the arguments of ``clip_guide_slots``: the same launch blends the entering tail slot with the known canvas forward-noised
    to ``t`` at clip positions c * slot_len + j — bit for bit this shift followed by the in-place ``clip_guide_slots`` call on the
    tail slot alone.  Everything else is the plain shift's."""
    z = L.dev_f32(z, "z")
    _check_rider(z, "hist", hist, hist_out, out_like_z=False)
    outer, S, inner = _queue_dims(z.shape, slot_len)
    _check_clip_slot(c, t, slot_len)
    key = noise_key(seed, 0)
    out = torch.empty_like(z)
    popped = torch.empty((z.shape[1], slot_len) + tuple(z.shape[3:]), device=z.device, dtype=torch.float32)
    if hist is None and guide is None:
        L.check(L.lib().avd_fifo_shift_f32(C.byref(key), t, c, z.data_ptr(), out.data_ptr(), popped.data_ptr(), z.shape[0], outer,
                                           S, slot_len, inner, _st(z)))
        return out, popped
    if hist is not None and hist_out is None:
        hist_out = torch.empty_like(hist)
    if guide is not None:
        if not isinstance(guide, dict) or set(guide) - {"known", "alpha_bar", "seed", "mask", "everywhere"} or \
                not {"known", "alpha_bar", "seed"} <= set(guide):
            raise ValueError(f"guide must be a dict with known, alpha_bar, seed and optionally mask, everywhere, got {guide!r}")
        m = None if guide.get("mask") is None else L.dev_f32(guide["mask"], "mask")
        g = clip_guide(guide["known"], m, guide["seed"], shape=tuple(z.shape))
        ab = guide["alpha_bar"]
        ab = (ab if (ab.is_cuda and ab.dtype == torch.float32) else ab.to(z.device, torch.float32)).contiguous()
        L.check(L.lib().avd_fifo_shift_guided_f32(C.byref(key), t, c, C.byref(g), ab.data_ptr(), ab.numel(),
                                                  1 if guide.get("everywhere") else 0, z.data_ptr(), out.data_ptr(), popped.data_ptr(),
                                                  L.ptr(hist), L.ptr(hist_out), z.shape[0], outer, S, slot_len, inner, _st(z)))
        return (out, popped) if hist is None else (out, popped, hist_out)
    L.check(L.lib().avd_fifo_shift_hist_f32(C.byref(key), t, c, z.data_ptr(), out.data_ptr(), popped.data_ptr(), hist.data_ptr(),
                                            hist_out.data_ptr(), z.shape[0], outer, S, slot_len, inner, _st(z)))
    return out, popped, hist_out


def fifo_lookahead(z: Tensor, ctx: int, shift: int, slot_len: int, c: Optional[int] = None, seed: Optional[int] = None,
                   t: Optional[int] = None, hist: Optional[Tensor] = None, hist_out: Optional[Tensor] = None):
    """The queue step of FIFO lookahead denoising (avd_fifo_lookahead_f32 / _hist_f32; contract in include/avdiff_hip.h, "FIFO
    lookahead"): ``z`` ([B,C,T,H,W] video, [B,Ca,F] audio, sliding length L = S * slot_len) is B overlapping windows of a logical
    queue of ctx + B * (S - ctx) slots, window k holding logical slots k * (S - ctx) .. + S - 1, its first ``ctx`` slots context only.
    Returns (z_out, popped): z_out window k slot s = the owner copy of logical slot k * (S - ctx) + s + shift.
    ``shift=1``: the queue moves by one slot; popped ([C, slot_len, H, W] or [Ca, slot_len]) is the head, which becomes the last
    context slot, and the tail holds the seeded normals of clip slot ``c`` at timestep ``t`` (``fifo_shift``'s draw; ``c``, ``seed``
    and ``t`` are required).  ``shift=0``: only the duplicates are refreshed from their owners; popped is None and ``c``, ``seed``,
    ``t`` must be left None.  ``ctx=0, shift=1`` gives ``fifo_shift``'s bits.
    With ``hist`` (as in ``fifo_shift``) the result is (z_out, popped, hist_out): the history follows the same map on the stepping
    positions, zeros in the entering tail slot and on every context position."""
    z = L.dev_f32(z, "z")
    _check_rider(z, "hist", hist, hist_out, out_like_z=False)
    outer, S, inner = _queue_dims(z.shape, slot_len)
    if isinstance(ctx, bool) or not isinstance(ctx, int) or not 0 <= ctx < S:
        raise ValueError(f"the lookahead ctx must be an int in [0, S = {S}), got {ctx!r}")
    if isinstance(shift, bool) or shift not in (0, 1):
        raise ValueError(f"shift must be 0 or 1, got {shift!r}")
    popped, key = None, None
    if shift:
        _check_clip_slot(c, t, slot_len, at=" at shift=1")
        if seed is None:
            raise ValueError("shift=1 draws the entering slot's noise from a seed: pass one")
        key = C.byref(noise_key(seed, 0))
        popped = torch.empty((z.shape[1], slot_len) + tuple(z.shape[3:]), device=z.device, dtype=torch.float32)
    elif c is not None or seed is not None or t is not None:
        raise ValueError("shift=0 draws nothing: leave c, seed and t None")
    out = torch.empty_like(z)
    head = (key, t or 0, c or 0, shift, z.data_ptr(), out.data_ptr(), L.ptr(popped))
    tail = (z.shape[0], outer, S, ctx, slot_len, inner, _st(z))
    if hist is None:
        L.check(L.lib().avd_fifo_lookahead_f32(*head, *tail))
        return out, popped
    hist_out = torch.empty_like(hist) if hist_out is None else hist_out
    L.check(L.lib().avd_fifo_lookahead_hist_f32(*head, hist.data_ptr(), hist_out.data_ptr(), *tail))
    return out, popped, hist_out


def fifo_carry(buf: Tensor, slots: int, slot_len: int, ctx: int = 0, shift: int = 1, out: Optional[Tensor] = None) -> Tensor:
    """A slot-attached buffer through the queue move (avd_fifo_carry_f32; contract in include/avdiff_hip.h, "slot APG momentum"):
    ``buf`` has the queue's layout ([B,C,T,H,W] video, [B,Ca,F] audio, sliding length ``slots`` * ``slot_len``) and holds per-element
    state of the slots, the slot APG momentum.  The result follows ``fifo_lookahead``'s history map: with h = slots - ctx, window b
    position s >= ctx receives the owner copy of logical slot b*h + s + shift; the entering tail slot (``shift=1``) and every context
    position s < ctx are zero.  ``ctx=0, shift=1`` is ``fifo_shift``'s history map, ``shift=0`` copies the stepping positions.
    A CPU tensor takes the torch statement below, which is the reference; a device tensor one out-of-place launch (``out``: a buffer
    of buf's shape that does not overlap it, None allocates one)."""
    if not (isinstance(buf, Tensor) and buf.dtype == torch.float32 and buf.dim() in (3, 5)):
        raise ValueError("buf must be a float32 tensor of the queue's layout, [B,C,T,H,W] or [B,Ca,F]")
    outer, L_, inner = window_dims(buf.shape)
    for name, v in (("slots", slots), ("slot_len", slot_len)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 1:
            raise ValueError(f"{name} must be an int >= 1, got {v!r}")
    if slots * slot_len != L_:
        raise ValueError(f"slots {slots} * slot_len {slot_len} must be the sliding length {L_}")
    if isinstance(ctx, bool) or not isinstance(ctx, int) or not 0 <= ctx < slots:
        raise ValueError(f"ctx must be an int in [0, slots = {slots}), got {ctx!r}")
    if isinstance(shift, bool) or shift not in (0, 1):
        raise ValueError(f"shift must be 0 or 1, got {shift!r}")
    B = buf.shape[0]
    if out is not None:
        _check_like(out, "out", buf, "buf's", "its device")
    if buf.is_cuda:
        buf = buf.contiguous()
        out = torch.empty_like(buf) if out is None else out
        L.check(L.lib().avd_fifo_carry_f32(buf.data_ptr(), out.data_ptr(), B, outer, slots, ctx, shift, slot_len, inner, _st(buf)))
        return out
    h = slots - ctx
    v = buf.reshape(B, outer, slots, slot_len, inner)
    queue = v[:, :, ctx:].permute(0, 2, 1, 3, 4).reshape(B * h, outer, slot_len, inner)      # the stepping owners: logical slots ctx ..
    moved = torch.zeros_like(queue)
    moved[:B * h - shift] = queue[shift:]                                                     # the entering tail slot stays zero
    res = torch.zeros_like(v)
    res[:, :, ctx:] = moved.reshape(B, h, outer, slot_len, inner).permute(0, 2, 1, 3, 4)
    res = res.reshape(buf.shape)
    return res if out is None else out.copy_(res)


def slot_apg_reference(cond: Tensor, null: Tensor, guidance, norm_threshold: float = 0.0, eta_parallel: float = 0.0,
                       momentum: float = 0.0, m_prev: Optional[Tensor] = None):
    """The slot APG of "slot CFG control" / "slot APG momentum" for stepping slots given as rows, in torch on the host: ``cond`` /
    ``null`` [n, per_slot] (any trailing shape), one slot per row in the slot's own order; ``guidance`` a number or n numbers;
    ``m_prev`` the slots' momentum elements (required exactly when ``momentum`` != 0).  Returns (e, d), float32: d = (cond - null) +
    momentum * m_prev with one fp32 rounding per operation — what the fused update stores back — and e = cond + w (d - k cond) with
    the coefficients from fp64 moments over the row, each rounded once to fp32.  The device sums its moments in 1024-element chunks,
    so its coefficients may differ from these in the last places."""
    r, eta_p, beta = apg_params(norm_threshold, eta_parallel, momentum)
    c, u = cond.detach().cpu().to(torch.float32), null.detach().cpu().to(torch.float32)
    if c.shape != u.shape or c.dim() < 2:
        raise ValueError(f"cond {tuple(c.shape)} and null {tuple(u.shape)} must have one shape [n, per_slot, ...]")
    if (beta != 0.0) != (m_prev is not None):
        raise ValueError("m_prev goes with momentum != 0: pass both or neither")
    n = c.shape[0]
    d = c - u
    if beta != 0.0:
        m = m_prev.detach().cpu().to(torch.float32)
        if m.shape != c.shape:
            raise ValueError(f"m_prev must have cond's shape {tuple(c.shape)}")
        d = d + torch.tensor(beta, dtype=torch.float32) * m
    c64, d64 = c.reshape(n, -1).double(), d.reshape(n, -1).double()
    sdd, sdc, scc = (d64 * d64).sum(1), (d64 * c64).sum(1), (c64 * c64).sum(1)
    r64 = float(torch.tensor(r, dtype=torch.float32))
    eta64 = float(torch.tensor(eta_p, dtype=torch.float32))
    s = torch.minimum(torch.ones_like(sdd), r64 / sdd.sqrt()).to(torch.float32)
    s = torch.where((sdd == 0) | ~torch.isfinite(s) | torch.tensor(r64 == 0.0), torch.ones_like(s), s)
    k = ((1.0 - eta64) * sdc / scc).to(torch.float32)
    k = torch.where((scc == 0) | ~torch.isfinite(k), torch.zeros_like(k), k)
    g = torch.as_tensor(guidance, dtype=torch.float32).reshape(-1).expand(n)
    w = (g - 1.0) * s
    shape = (n,) + (1,) * (c.dim() - 1)
    e = c + w.reshape(shape) * (d - k.reshape(shape) * c)
    return e, d


# ---- FIFO device cursors (include/avdiff_hip.h, "FIFO device cursors"): the host numbers of a FIFO iteration read off the device ----
def _cursor(cursor: Tensor, device: torch.device) -> Tensor:
    if not (isinstance(cursor, Tensor) and cursor.is_cuda and cursor.dtype == torch.int32 and cursor.numel() == 1 and
            cursor.device == device):
        raise ValueError("a cursor is one int32 in device memory (a 1-element int32 tensor on the buffers' device)")
    return cursor


def cursor_add(cursor: Tensor, delta: int = 1) -> None:
    """*cursor += delta on the current stream (avd_cursor_add): how a FIFO cursor moves, in a launch of its own behind its readers."""
    L.check(L.lib().avd_cursor_add(_cursor(cursor, cursor.device).data_ptr(), int(delta), _st(cursor)))


def stack_slot_tables(rows: Tensor) -> Tensor:
    """[n_rows, B, S] int tables (a ramp table of ``schedule_utils.fifo_plan`` / ``fifo_plan_last``) -> contiguous int64 [n_rows, B*S],
    the layout ``slot_tables_select`` reads: row r reshaped to [B, S] is ``rows[r]``.  Any device."""
    rows = torch.as_tensor(rows)
    if rows.dim() != 3 or rows.is_floating_point() or rows.dtype == torch.bool:
        raise ValueError(f"slot tables are integer [n_rows, B, S], got {rows.dtype} {tuple(rows.shape)}")
    return rows.to(torch.long).reshape(rows.shape[0], rows.shape[1] * rows.shape[2]).contiguous()


def slot_tables_select(tables, cursor: Tensor, outs) -> None:
    """One launch (avd_slot_tables_select) copies row min(max(*cursor, 0), n_rows - 1) of each of the two or three ``tables``
    (contiguous int64 [n_rows, n] on the device, ``stack_slot_tables``) into its buffer of ``outs`` (contiguous int64, n elements: the
    fixed [B, S] tables ``step_slots`` reads).  The cursor is read, not moved."""
    tables, outs = list(tables), list(outs)
    if len(tables) not in (2, 3) or len(outs) != len(tables):
        raise ValueError("slot_tables_select takes two or three tables and as many buffers")
    dev = tables[0].device
    n_rows, n = (int(v) for v in tables[0].shape) if tables[0].dim() == 2 else (0, 0)
    for t in tables:
        if not (t.is_cuda and t.dtype == torch.long and t.is_contiguous() and t.dim() == 2 and tuple(t.shape) == (n_rows, n) and t.device == dev):
            raise ValueError("tables must be contiguous int64 [n_rows, n] device tensors of one shape")
    for o in outs:
        if not (o.is_cuda and o.dtype == torch.long and o.is_contiguous() and o.numel() == n and o.device == dev):
            raise ValueError(f"every buffer must be a contiguous int64 device tensor of {n} elements")
    p = [t.data_ptr() for t in tables] + [None] * (3 - len(tables))
    q = [o.data_ptr() for o in outs] + [None] * (3 - len(outs))
    L.check(L.lib().avd_slot_tables_select(*p, n_rows, n, _cursor(cursor, dev).data_ptr(), *q, L.stream_ptr(dev)))


def fifo_prompt_gather(prompt_canvas: Tensor, cursor: Tensor, B: int, S: int, prompt_hop: int, prompt_len: int,
                       out: Optional[Tensor] = None) -> Tensor:
    """``stream_infer.fifo_prompt_windows(prompt_canvas, m = max(*cursor, 0), ...)`` in one launch with m read off the device
    (avd_fifo_prompt_gather_f32): [B, C, prompt_len, H, W] from a video prompt canvas [C, P, H, W], [B, Ca, prompt_len] from an audio
    one [Ca, P], zeros beyond the canvas end.  ``out``: a contiguous float32 buffer of that shape that does not overlap the canvas."""
    pc = prompt_canvas
    if not (isinstance(pc, Tensor) and pc.is_cuda and pc.dtype == torch.float32 and pc.is_contiguous() and pc.dim() in (2, 4)):
        raise ValueError("a prompt canvas is a contiguous float32 device tensor [C, P, H, W] (video) or [Ca, P] (audio)")
    for name, v in (("B", B), ("S", S), ("prompt_hop", prompt_hop), ("prompt_len", prompt_len)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v < 2 ** 31:
            raise ValueError(f"{name} must be an int in [1, 2**31), got {v!r}")
    shape = (B, pc.shape[0], prompt_len) + tuple(pc.shape[2:])
    if out is None:
        out = torch.empty(shape, device=pc.device, dtype=torch.float32)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape and out.device == pc.device):
        raise ValueError(f"out must be a contiguous float32 tensor of shape {shape} on the canvas's device")
    inner = pc.shape[2] * pc.shape[3] if pc.dim() == 4 else 1
    L.check(L.lib().avd_fifo_prompt_gather_f32(pc.data_ptr(), _cursor(cursor, pc.device).data_ptr(), out.data_ptr(), B, S, prompt_hop,
                                               pc.shape[0], pc.shape[1], prompt_len, inner, _st(pc)))
    return out


PROMPT_INTERPS = ("nearest", "linear")      # avd_fifo_prompt_gather_frac_f32's `interp`, by index


def check_prompt_frac(num: int, den: int, interp: Optional[str], what: str = "prompt_hop") -> None:
    """the hop num / den and the mode of a fractional prompt walk (include/avdiff_hip.h, "fractional prompt hop"): ValueError unless
    both are ints in [1, 2**31), ``interp`` is None or one of ``PROMPT_INTERPS``, and a den > 1 comes with a mode"""
    for name, v in ((what, num), ("prompt_den", den)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v < 2 ** 31:
            raise ValueError(f"{name} must be an int in [1, 2**31), got {v!r}")
    if interp is not None and interp not in PROMPT_INTERPS:
        raise ValueError(f"prompt_interp must be None or one of {PROMPT_INTERPS}, got {interp!r}")
    if den > 1 and interp is None:
        raise ValueError(f"prompt_den {den} > 1 is a fractional prompt hop: it needs prompt_interp, one of {PROMPT_INTERPS}, to say how a "
                         "window that starts between two prompt positions is read")


def fifo_prompt_gather_frac(prompt_canvas: Tensor, cursor: Optional[Tensor], B: int, first: int, stride: int, num: int, den: int,
                            interp: str, prompt_len: int, out: Optional[Tensor] = None) -> Tensor:
    """``stream_infer.fifo_prompt_windows`` on a rational hop ``num / den`` in one launch (avd_fifo_prompt_gather_frac_f32;
    include/avdiff_hip.h, "fractional prompt hop"): sample k is the prompt window of clip slot q = first + max(*cursor, 0) + k*stride,
    read by ``interp`` ("nearest" or "linear"); zeros before the canvas start and past its end.  ``cursor``: one int32 on the device,
    or None (reads as 0: pass m in ``first``).  ``first`` may be negative.  Shapes and ``out`` as ``fifo_prompt_gather``; ``den == 1``
    gives its bits in either mode."""
    pc = prompt_canvas
    if not (isinstance(pc, Tensor) and pc.is_cuda and pc.dtype == torch.float32 and pc.is_contiguous() and pc.dim() in (2, 4)):
        raise ValueError("a prompt canvas is a contiguous float32 device tensor [C, P, H, W] (video) or [Ca, P] (audio)")
    for name, v in (("B", B), ("stride", stride), ("prompt_len", prompt_len)):
        if isinstance(v, bool) or not isinstance(v, int) or not 1 <= v < 2 ** 31:
            raise ValueError(f"{name} must be an int in [1, 2**31), got {v!r}")
    if isinstance(first, bool) or not isinstance(first, int) or not -2 ** 31 < first < 2 ** 31:
        raise ValueError(f"first must be an int with |first| < 2**31, got {first!r}")
    check_prompt_frac(num, den, interp, "num")
    if interp is None:
        raise ValueError(f"interp must be one of {PROMPT_INTERPS}, got None")
    shape = (B, pc.shape[0], prompt_len) + tuple(pc.shape[2:])
    if out is None:
        out = torch.empty(shape, device=pc.device, dtype=torch.float32)
    elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == shape and out.device == pc.device):
        raise ValueError(f"out must be a contiguous float32 tensor of shape {shape} on the canvas's device")
    inner = pc.shape[2] * pc.shape[3] if pc.dim() == 4 else 1
    cur = None if cursor is None else _cursor(cursor, pc.device).data_ptr()
    L.check(L.lib().avd_fifo_prompt_gather_frac_f32(pc.data_ptr(), cur, out.data_ptr(), B, first, stride, num, den,
                                                    PROMPT_INTERPS.index(interp), pc.shape[0], pc.shape[1], prompt_len, inner, _st(pc)))
    return out


def fifo_shift_cursor(z: Tensor, c0: int, cursor: Tensor, clip: Tensor, seed: int, t: int, slot_len: int, out: Optional[Tensor] = None,
                      hist: Optional[Tensor] = None, hist_out: Optional[Tensor] = None):
    """``fifo_shift`` with the clip slot on the device (avd_fifo_shift_cursor_f32 / _hist_f32; contract in include/avdiff_hip.h, "FIFO
    queue shift off a device cursor"): with m = *cursor the queue shifts as ``fifo_shift(z, c0 + m, ...)`` and the finished head is
    written straight into slot m of ``clip``, the clip canvas [C, n_out * slot_len, H, W] / [Ca, n_out * slot_len] — nowhere when m is
    outside [0, n_out).  Returns z_out, or (z_out, hist_out) with ``hist``.  ``out`` / ``hist_out``: buffers to write to (z's shape).
    The cursor is read, not moved."""
    z = L.dev_f32(z, "z")
    outer, S, inner = _queue_dims(z.shape, slot_len)
    if not (isinstance(clip, Tensor) and clip.is_cuda and clip.dtype == torch.float32 and clip.is_contiguous() and clip.device == z.device and
            clip.dim() == z.dim() - 1 and clip.shape[0] == z.shape[1] and tuple(clip.shape[2:]) == tuple(z.shape[3:]) and
            clip.shape[1] >= slot_len and clip.shape[1] % slot_len == 0):
        raise ValueError(f"clip must be a contiguous float32 canvas [{z.shape[1]}, n_out * {slot_len}, ...] of z's slice shape on z's device")
    n_out = clip.shape[1] // slot_len
    _check_clip_slot(c0, t, slot_len, n_out)
    if out is not None:
        _check_like(out, "out", z)
    _check_rider(z, "hist", hist, hist_out)
    key = noise_key(seed, 0)
    out = torch.empty_like(z) if out is None else out
    head = (C.byref(key), t, c0, _cursor(cursor, z.device).data_ptr(), n_out, z.data_ptr(), out.data_ptr(), clip.data_ptr())
    tail = (z.shape[0], outer, S, slot_len, inner, _st(z))
    if hist is None:
        L.check(L.lib().avd_fifo_shift_cursor_f32(*head, *tail))
        return out
    hist_out = torch.empty_like(hist) if hist_out is None else hist_out
    L.check(L.lib().avd_fifo_shift_cursor_hist_f32(*head, hist.data_ptr(), hist_out.data_ptr(), *tail))
    return out, hist_out


def clip_seeds(seeds, queues: int, device=None) -> Tensor:
    """The K seeds of a FIFO clip batch as the int64 tensor ``fifo_shift_clips`` passes to its launch (the kernel reads the same 64
    bits unsigned): ``seeds`` is a sequence of ``queues`` ints, each checked as ``noise_key`` checks a seed.  ``device`` None keeps it
    on the CPU."""
    if isinstance(seeds, Tensor) or isinstance(seeds, (str, bytes)) or not hasattr(seeds, "__len__"):
        raise ValueError(f"seeds must be a sequence of {queues} ints, got {seeds!r}")
    if len(seeds) != queues:
        raise ValueError(f"{len(seeds)} seeds for {queues} queues: fifo_shift_clips needs one seed per queue")
    for s in seeds:
        noise_key(s, 0)
    t = torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in seeds], dtype=torch.int64)
    return t if device is None else t.to(device)


def fifo_shift_clips(z: Tensor, queues: int, c: int, seeds, t: int, slot_len: int, clips: Tensor, m: int, hist: Optional[Tensor] = None,
                     hist_out: Optional[Tensor] = None, carry: Optional[Tensor] = None, carry_out: Optional[Tensor] = None, *,
                     tails: Optional[Tensor] = None):
    """The queue step of a FIFO clip batch (avd_fifo_shift_clips_f32; contract in include/avdiff_hip.h, "FIFO clip batch"): ``z``
    ([B,C,T,H,W] video, [B,Ca,F] audio, sliding length L = S * slot_len) is ``queues`` = K independent queues in lockstep, queue k the
    samples k * B/K .. (k + 1) * B/K - 1.  Every queue shifts as ``fifo_shift`` shifts its batch, never into its neighbour: the tail
    slot of queue k holds the seeded normals of clip slot ``c`` at timestep ``t`` under ``seeds[k]``, and its head is written into slot
    ``m`` of ``clips[k]`` (``clips``: [K, C, n_clip * slot_len, H, W] / [K, Ca, n_clip * slot_len], written in place; ``m`` outside
    [0, n_clip) writes no head).  ``seeds``: K ints, or the int64 device tensor ``clip_seeds`` makes of them (a loop uploads it once).
    ``hist`` / ``carry`` (z's shape) are riders that take the same map with zeros in every entering slot — the DPM-Solver++(2M)
    history and the slot APG momentum; ``hist_out`` / ``carry_out``: buffers to write them to, None allocates.  Returns z_out, or the
    tuple (z_out, hist_out and / or carry_out) with riders.
    A device tensor takes the one launch.  A CPU tensor takes the torch statement below, which is the reference: per queue a roll by one
    slot and the tail; ``tails`` ([K, C, slot_len, H, W] / [K, Ca, slot_len]) hands the entering slots in, None draws them with
    ``canvas_noise`` (which needs a device: a CPU-only caller passes ``tails``).  ``tails`` is refused with a device tensor."""
    if not (isinstance(z, Tensor) and z.dtype == torch.float32 and z.dim() in (3, 5)):
        raise ValueError("z must be a float32 tensor of the queue's layout, [B,C,T,H,W] or [B,Ca,F]")
    B, L_ = z.shape[0], z.shape[2]
    if isinstance(queues, bool) or not isinstance(queues, int) or queues < 1 or B % queues:
        raise ValueError(f"queues {queues!r} must be an int >= 1 that divides the batch {B}")
    outer, S, inner = _queue_dims(z.shape, slot_len)
    _check_clip_slot(c, t, slot_len)
    if isinstance(m, bool) or not isinstance(m, int):
        raise ValueError(f"m must be an int (the clip slot the heads go to), got {m!r}")
    if isinstance(seeds, Tensor):
        if not (seeds.dtype == torch.int64 and seeds.is_contiguous() and tuple(seeds.shape) == (queues,) and seeds.device == z.device):
            raise ValueError(f"a seeds tensor must be clip_seeds' int64 [{queues}] on z's device, got {seeds.dtype} "
                             f"{tuple(seeds.shape)} on {seeds.device}")
    else:
        seeds = clip_seeds(seeds, queues, z.device)
    slice_shape = (z.shape[1],) + tuple(z.shape[3:])
    if not (isinstance(clips, Tensor) and clips.dtype == torch.float32 and clips.is_contiguous() and clips.device == z.device and
            clips.dim() == z.dim() and clips.shape[0] == queues and (clips.shape[1],) + tuple(clips.shape[3:]) == slice_shape and
            clips.shape[2] >= slot_len and clips.shape[2] % slot_len == 0):
        raise ValueError(f"clips must be a contiguous float32 [{queues}, {z.shape[1]}, n_clip * {slot_len}, ...] of z's slice shape on "
                         f"z's device, got {tuple(clips.shape) if isinstance(clips, Tensor) else clips!r}")
    n_clip = clips.shape[2] // slot_len
    riders = []
    for name, a, b in (("hist", hist, hist_out), ("carry", carry, carry_out)):
        _check_rider(z, name, a, b)
        if a is not None:
            riders.append([a, torch.empty_like(a) if b is None else b])
    if z.is_cuda:
        if tails is not None:
            raise ValueError("tails belongs to the CPU statement: the launch draws the entering slots itself")
        z = z.contiguous()
        out = torch.empty_like(z)
        h, k = ((hist, riders[0][1]) if hist is not None else (None, None)), ((carry, riders[-1][1]) if carry is not None else (None, None))
        L.check(L.lib().avd_fifo_shift_clips_f32(seeds.data_ptr(), t, c, z.data_ptr(), out.data_ptr(), clips.data_ptr(), n_clip, m,
                                                 L.ptr(h[0]), L.ptr(h[1]), L.ptr(k[0]), L.ptr(k[1]), B, queues, outer,
                                                 S, slot_len, inner, _st(z)))
        return out if not riders else (out,) + tuple(r[1] for r in riders)
    Bq = B // queues
    if tails is None:
        vals = [s + 2 ** 64 if s < 0 else s for s in seeds.tolist()]
        tails = torch.stack([canvas_noise(s, torch.tensor([t]), (1,) + slice_shape[:1] + (slot_len,) + slice_shape[1:], slot_len,
                                          window_offset=c)[0].cpu() for s in vals])
    elif not (isinstance(tails, Tensor) and tuple(tails.shape) == (queues, z.shape[1], slot_len) + tuple(z.shape[3:])):
        raise ValueError(f"tails must be the entering slots, shape {(queues, z.shape[1], slot_len) + tuple(z.shape[3:])}")

    def roll(x: Tensor, tail: Tensor) -> Tensor:
        """one queue [Bq, C, L, ...] rolled by one slot towards its head, ``tail`` [C, slot_len, ...] in its last slot"""
        q = x.movedim(2, 1).reshape((Bq * (L_ // slot_len), slot_len) + slice_shape)      # [queue slot, j, C, ...]
        q = torch.roll(q, -1, 0)
        q[-1] = tail.movedim(1, 0)
        return q.reshape((Bq, L_) + slice_shape).movedim(1, 2)

    out = torch.empty_like(z)
    for k in range(queues):
        sl = slice(k * Bq, (k + 1) * Bq)
        if 0 <= m < n_clip:
            clips[k, :, m * slot_len:(m + 1) * slot_len] = z[k * Bq, :, :slot_len]
        out[sl] = roll(z[sl], tails[k].to(torch.float32))
        for a, b in riders:
            b[sl] = roll(a[sl], torch.zeros_like(tails[k], dtype=torch.float32))
    return out if not riders else (out,) + tuple(r[1] for r in riders)


# ---- "bf16x3": fp32-accurate Linear on the bf16 matrix pipe (csrc/gemm_bf16x3.hip) ----
def _image_like(rows: int, d: int, device: torch.device, who: str) -> Tensor:
    """an uninitialised operand image for a [rows, d] matrix; a width the image geometry does not cover is refused here"""
    nbytes = L.lib().avd_split3_bytes(rows, d)
    if nbytes < 0:
        raise L.AvdError(f"{who}: need rows > 0 and d % 16 == 0 (rows={rows} d={d})")
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def _image_scale(scale: float, who: str) -> float:
    """a caller's f16x2 image scale: positive and finite, or refused before anything is allocated or launched"""
    scale = float(scale)
    if not (0.0 < scale < math.inf):
        raise L.AvdError(f"{who}: the f16x2 image scale must be positive and finite, got {scale}")
    return scale


def split3(x: Tensor, out: Optional[Tensor] = None) -> Tensor:
    """fp32 [rows, K] -> its split3 image (uint8; three bf16 planes, tiled).  K must be a multiple of 16.
    ``out``: an existing image of the same size to overwrite (keeps its address)."""
    x = L.dev_f32(x, "x")
    k = x.shape[-1]
    rows = x.numel() // k
    nbytes = L.lib().avd_split3_bytes(rows, k)
    if nbytes < 0:
        raise L.AvdError(f"split3: K={k} must be a multiple of 16")
    if out is None or out.numel() != nbytes or out.device != x.device:
        out = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    L.check(L.lib().avd_split3_f32(x.data_ptr(), out.data_ptr(), rows, k, _st(x)))
    return out


def rmsnorm_split3(x: Tensor, scale: Tensor, eps: float = 1e-6) -> Tensor:
    """RMSNorm(x) written as a split3 image (the A operand of the next bf16x3 Linear)."""
    x = L.dev_f32(x, "x")
    scale = L.dev_f32(scale, "scale")
    d = x.shape[-1]
    rows = x.numel() // d
    out = _image_like(rows, d, x.device, "rmsnorm_split3")
    L.check(L.lib().avd_rmsnorm_split3_f32(x.data_ptr(), scale.data_ptr(), out.data_ptr(), rows, d, eps, _st(x)))
    return out


def layernorm_act_split3(x: Tensor, weight: Tensor, bias: Tensor, eps: float = 1e-5, act: int = L.ACT_NONE) -> Tensor:
    """act(LayerNorm(x)) written as a split3 image (what the noise head's trunk hands its next bf16x3 Linear)."""
    x = L.dev_f32(x, "x")
    weight = L.dev_f32(weight, "weight")
    bias = L.dev_f32(bias, "bias")
    d = x.shape[-1]
    rows = x.numel() // d
    out = _image_like(rows, d, x.device, "layernorm_act_split3")
    L.check(L.lib().avd_layernorm_act_split3_f32(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), out.data_ptr(), rows, d, eps, act,
                                                 _st(x)))
    return out


def linear_bf16x3(x3: Tensor, rows: int, w3: Tensor, n: int, k: int, bias: Optional[Tensor] = None,
                  residual: Optional[Tensor] = None, act: int = L.ACT_NONE, out_split3: bool = False, terms: int = 6) -> Tensor:
    """act(x @ W.T + bias) + residual with both operands given as split3 images; fp32 [rows, n] result, or its split3
    image when out_split3 (bias + GELU only).  terms: 6 default, 9 strict (nothing dropped), 1 plain bf16 operands."""
    b = None if bias is None else L.dev_f32(bias, "bias")
    r = None if residual is None else L.dev_f32(residual, "residual")
    if out_split3:
        out = torch.empty(L.lib().avd_split3_bytes(rows, n), dtype=torch.uint8, device=x3.device)
        c, c3 = None, out.data_ptr()
    else:
        out = torch.empty(rows, n, dtype=torch.float32, device=x3.device)
        c, c3 = out.data_ptr(), None
    L.check(L.lib().avd_gemm_bf16x3_f32(x3.data_ptr(), w3.data_ptr(), L.ptr(b), L.ptr(r), c, c3, rows, n, k, act, terms, _st(x3)))
    return out


# ---- "f16x2": two scaled fp16 planes per operand, three product terms (include/avdiff_hip.h) ----
def f16x2_scale(bound: float) -> float:
    """Largest power of two s with s * bound <= 2^15 (fp16 tops out at 65504), for a bound on |x| over the image.
    The bound is widened by 1 % first so that fp32 rounding of the values it covers cannot cross it."""
    import math
    bound = float(bound) * 1.01
    if not math.isfinite(bound):
        raise L.AvdError("f16x2: the bound on the operand's magnitude is not finite")
    if bound <= 0.0:
        return 1.0
    e = 15 - math.ceil(math.log2(bound))
    return float(2.0 ** max(-100, min(100, e)))


def weight_bounds(tensors) -> list:
    """[(max|w|, max row 2-norm), ...] for a list of fp32 device tensors (vectors count as one row), computed by the library
    (``avd_weight_bounds_f32``); one device-to-host copy for the whole list."""
    tensors = [L.dev_f32(t.detach(), "weight") for t in tensors]
    if not tensors:
        return []
    out = torch.empty(len(tensors), 2, dtype=torch.float32, device=tensors[0].device)
    for i, t in enumerate(tensors):
        cols = t.shape[-1]
        rows = t.numel() // cols
        L.check(L.lib().avd_weight_bounds_f32(t.data_ptr(), rows, cols, out[i].data_ptr(), _st(t)))
    return [(float(a), float(b)) for a, b in out.cpu().tolist()]


def split_f16x2(x: Tensor, scale: Optional[float] = None, out: Optional[Tensor] = None):
    """fp32 [rows, K] -> (f16x2 image, scale).  scale None: derived from max|x| (one device sync)."""
    x = L.dev_f32(x, "x")
    k = x.shape[-1]
    rows = x.numel() // k
    nbytes = L.lib().avd_split3_bytes(rows, k)
    if nbytes < 0:
        raise L.AvdError(f"split_f16x2: K={k} must be a multiple of 16")
    if scale is None:
        scale = f16x2_scale(weight_bounds([x.reshape(rows, k)])[0][0])
    if out is None or out.numel() != nbytes or out.device != x.device:
        out = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    L.check(L.lib().avd_split_f16x2_f32(x.data_ptr(), out.data_ptr(), rows, k, scale, _st(x)))
    return out, scale


def rmsnorm_split_f16x2(x: Tensor, gamma: Tensor, eps: float = 1e-6, scale: Optional[float] = None):
    """RMSNorm(x) written as an f16x2 image; the default scale uses |y_i| <= sqrt(d) max|gamma|."""
    x = L.dev_f32(x, "x")
    gamma = L.dev_f32(gamma, "scale")
    d = x.shape[-1]
    rows = x.numel() // d
    if scale is None:
        scale = f16x2_scale(weight_bounds([gamma])[0][0] * d ** 0.5)
    scale = _image_scale(scale, "rmsnorm_split_f16x2")
    out = _image_like(rows, d, x.device, "rmsnorm_split_f16x2")
    L.check(L.lib().avd_rmsnorm_split_f16x2_f32(x.data_ptr(), gamma.data_ptr(), out.data_ptr(), rows, d, eps, scale, _st(x)))
    return out, scale


def layernorm_act_split_f16x2(x: Tensor, weight: Tensor, bias: Tensor, eps: float = 1e-5, act: int = L.ACT_NONE,
                              scale: Optional[float] = None):
    """act(LayerNorm(x)) written as an f16x2 image; the default scale uses the noise head's bound
    |y_i| <= sqrt(d) max|gamma| + max|beta| (every activation here satisfies |act(y)| <= |y|)."""
    x = L.dev_f32(x, "x")
    weight = L.dev_f32(weight, "weight")
    bias = L.dev_f32(bias, "bias")
    d = x.shape[-1]
    rows = x.numel() // d
    if scale is None:
        (gmax, _), (bmax, _) = weight_bounds([weight, bias])
        scale = f16x2_scale(gmax * d ** 0.5 + bmax)
    scale = _image_scale(scale, "layernorm_act_split_f16x2")
    out = _image_like(rows, d, x.device, "layernorm_act_split_f16x2")
    L.check(L.lib().avd_layernorm_act_split_f16x2_f32(x.data_ptr(), weight.data_ptr(), bias.data_ptr(), out.data_ptr(), rows, d, eps,
                                                      act, scale, _st(x)))
    return out, scale


def linear_f16x2(x2: Tensor, rows: int, w2: Tensor, n: int, k: int, ab_scale: float, bias: Optional[Tensor] = None,
                 residual: Optional[Tensor] = None, act: int = L.ACT_NONE, out_scale: Optional[float] = None) -> Tensor:
    """act(x @ W.T + bias) + residual with both operands given as f16x2 images of scales s_x, s_w (ab_scale = s_x * s_w);
    fp32 [rows, n] result, or — out_scale given — its f16x2 image at that scale (bias + GELU only)."""
    b = None if bias is None else L.dev_f32(bias, "bias")
    r = None if residual is None else L.dev_f32(residual, "residual")
    if out_scale is not None:
        out = torch.empty(L.lib().avd_split3_bytes(rows, n), dtype=torch.uint8, device=x2.device)
        c, c2 = None, out.data_ptr()
    else:
        out = torch.empty(rows, n, dtype=torch.float32, device=x2.device)
        c, c2 = out.data_ptr(), None
    L.check(L.lib().avd_gemm_f16x2_f32(x2.data_ptr(), w2.data_ptr(), L.ptr(b), L.ptr(r), c, c2, rows, n, k, act, ab_scale,
                                       1.0 if out_scale is None else out_scale, _st(x2)))
    return out
