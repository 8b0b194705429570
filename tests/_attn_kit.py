"""What the attention tests share: the two operand-image decoders, the q|k|v image built through an identity in_proj (bf16x3 and
f16x2), softmax(q k^T / 8) v in fp64, the fp8 kernel's two references, and one cached case per input (operands, references, the
fp32-MFMA kernel's error, both images).  Nothing here touches the GPU at import time."""
import math
from functools import lru_cache
from types import SimpleNamespace

import numpy as np
import torch

QSCALE = 0.125 * 1.4426950408889634          # softmax scale * log2 e, folded into q by the in_proj epilogue


# ------------------------------------------------------------------------------------------------- image decoders
def _image_offsets(rows: int, K: int) -> np.ndarray:
    """byte offset of plane 0 of element (r, k) in a split3 / f16x2 image (include/avdiff_hip.h, csrc/gemm_bf16x3.hip)"""
    r = np.arange(rows)[:, None]
    k = np.arange(K)[None, :]
    f = ((r & 127) >> 4) & 1
    half = (k >> 3) & 1
    return ((r >> 7) * (K // 16) + (k >> 4)) * (128 * 96) + (r & 127) * 32 + ((half ^ f) * 16) + (k & 7) * 2


def split3_decode(img: np.ndarray, rows: int, K: int) -> np.ndarray:
    """Independent reading of the split3 image layout (include/avdiff_hip.h, csrc/gemm_bf16x3.hip): -> planes [3, rows, K]."""
    base = _image_offsets(rows, K)
    u16 = img.view(np.uint16)
    planes = []
    for p in range(3):
        bits = u16[(base + p * 4096) // 2].astype(np.uint32) << 16
        planes.append(bits.view(np.float32))
    return np.stack(planes)


def h2_decode(img: np.ndarray, rows: int, K: int) -> np.ndarray:
    """Independent reading of the f16x2 image (split3 geometry, planes 0 and 1 hold fp16): -> [2, rows, K] float64."""
    base = _image_offsets(rows, K)
    f16 = img.view(np.float16)
    return np.stack([f16[(base + p * 4096) // 2].astype(np.float64) for p in range(2)])


# ------------------------------------------------------------------------------------------------- references
def _heads(qkv, B, N, H):
    full = qkv.double().view(B, N, 3, H, 64)
    return (full[:, :, i].transpose(1, 2) for i in range(3))                  # q, k, v: [B, H, N, 64]


def attn_ref(qkv, B, N, H):
    """softmax(q k^T / 8) v in fp64 from the packed [B*N, 3d] operands -> [B, N, d]"""
    q, k, v = _heads(qkv, B, N, H)
    return (torch.softmax(q @ k.transpose(-1, -2) / 8.0, dim=-1) @ v).transpose(1, 2).reshape(B, N, H * 64)


def attn_ref_e4m3(qkv, B, N, H):
    """fp64 on the operands the fp8 kernel multiplies: q (carrying scale * log2 e * 8), k, v rounded to e4m3, p rounded to e4m3
    relative to the row maximum at scale 256 (the second reference of test_attention_fp8_reported_error)"""
    q, k, v = _heads(qkv, B, N, H)
    f8 = lambda t: t.float().to(torch.float8_e4m3fn).double()
    s = (f8(q * (QSCALE * 8.0)) @ f8(k).transpose(-1, -2)) / 8.0 * math.log(2.0)
    p = torch.softmax(s, dim=-1)
    pmax = p.max(-1, keepdim=True).values
    pq = f8(p / pmax * 256.0) / 256.0 * pmax
    return (pq @ f8(v) / p.sum(-1, keepdim=True)).transpose(1, 2).reshape(B, N, H * 64)


# ------------------------------------------------------------------------------------------------- q|k|v images
@lru_cache(maxsize=None)
def _identity_images(dev, n):
    from multimodal_diffusion_amd import functional as Fn
    eye = torch.eye(n, device=dev)
    return Fn.split3(eye), Fn.split_f16x2(eye)


def qkv_image(dev, qkv, B, N, H, kind, fill=None):
    """(image, scale): the q|k|v operand image of the [B*N, 3d] tensor `qkv`, written by the in_proj epilogue of an identity
    projection with a zero bias — kind "bf16x3" (avd_gemm_bf16x3_qkv3_f32; scale 1.0) or "f16x2" (avd_gemm_f16x2_qkv_f32; scale from
    max|qkv|).  fill: the byte the buffer holds before the epilogue writes it (None: uninitialised)."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    lib = L.lib()
    d3 = 3 * H * 64
    nbytes = lib.avd_qkv3_bytes(B, N, H)
    img = torch.empty(nbytes, dtype=torch.uint8, device=dev) if fill is None else torch.full((nbytes,), fill, dtype=torch.uint8, device=dev)
    zb = torch.zeros(d3, device=dev)
    w3, (w2, sw) = _identity_images(dev, d3)
    x = qkv.to(dev)
    if kind == "bf16x3":
        x3 = Fn.split3(x)
        L.check(lib.avd_gemm_bf16x3_qkv3_f32(x3.data_ptr(), w3.data_ptr(), zb.data_ptr(), img.data_ptr(), B * N, N, H, d3, QSCALE, 6,
                                             L.stream_ptr(dev)))
        return img, 1.0
    assert kind == "f16x2", kind
    x2, sx = Fn.split_f16x2(x)
    sq = Fn.f16x2_scale(float(qkv.abs().max()))
    L.check(lib.avd_gemm_f16x2_qkv_f32(x2.data_ptr(), w2.data_ptr(), zb.data_ptr(), img.data_ptr(), B * N, N, H, d3, QSCALE, sx * sw, sq,
                                       L.stream_ptr(dev)))
    return img, sq


def run_attn(dev, img, scale, terms, B, N, H, nq, out=None, out_img=None):
    """the split-operand attention on a q|k|v image: terms 3 takes the f16x2 entry point (image and output image at `scale`)"""
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    o, oi = (None if t is None else t.data_ptr() for t in (out, out_img))
    if terms == 3:
        L.check(lib.avd_attn_fwd_qkv_f16x2_f32(img.data_ptr(), o, oi, B, N, H, nq, scale, scale, L.stream_ptr(dev)))
    else:
        L.check(lib.avd_attn_fwd_qkv3_f32(img.data_ptr(), o, oi, B, N, H, nq, terms, L.stream_ptr(dev)))


def run_attn_fp8(dev, img, scale, kind, ws, B, N, H, nq, out=None, out_img=None):
    """the fp8 attention on a q|k|v image of either kind; `ws` is its workspace"""
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    o, oi = (None if t is None else t.data_ptr() for t in (out, out_img))
    if kind == "f16x2":
        L.check(lib.avd_attn_fwd_fp8_f16x2_f32(img.data_ptr(), ws.data_ptr(), ws.numel(), o, oi, B, N, H, nq, scale, scale, L.stream_ptr(dev)))
    else:
        L.check(lib.avd_attn_fwd_fp8_f32(img.data_ptr(), ws.data_ptr(), ws.numel(), o, oi, B, N, H, nq, L.stream_ptr(dev)))


# ------------------------------------------------------------------------------------------------- cached cases
_CASES = {}


def attn_case(dev, key, make, B, N, H):
    """One input, computed once per module run and never modified: `make()` returns the [B*N, 3d] operands.  Holds qkv, the fp64
    reference `ref` [B, N, d], the fp32-MFMA kernel's output `y32` (Fn.attention) and both q|k|v images with their scales."""
    key = (str(dev), key, B, N, H)
    if key not in _CASES:
        from multimodal_diffusion_amd import functional as Fn
        qkv = make()
        assert qkv.shape == (B * N, 3 * H * 64)
        img3, _ = qkv_image(dev, qkv, B, N, H, "bf16x3")
        img2, sq = qkv_image(dev, qkv, B, N, H, "f16x2")
        _CASES[key] = SimpleNamespace(qkv=qkv, ref=attn_ref(qkv, B, N, H), y32=Fn.attention(qkv.view(B, N, -1).to(dev), H).cpu(),
                                      img={6: img3, 9: img3, 1: img3, 3: img2}, scale={6: 1.0, 9: 1.0, 1: 1.0, 3: sq})
    return _CASES[key]
