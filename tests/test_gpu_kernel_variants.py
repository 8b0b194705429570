"""GPU tests of the kernel variants that only a tune key selects (avd_tune_set, the AVD_* environment variables), against fp64.

A. every split-operand attention kernel x operand mode x output form at the edges of the key and query tiles;
B. inputs that stress the online softmax (a dominant key early, late and last; equal keys; wide scores) and the guarantee that the
   padding slots of the q|k|v image are never read (image prefilled with NaN bytes), on all three kernels and on the fp8 path;
C. the fp8 attention's f16x2 quantiser and its two image outputs, called directly;
D. the fp32 GEMM's LDS ring depth ("gemm_stages") on both tiles it applies to, and the super-tile shape of the split GEMMs' block map
   ("s3_sn", "s3_super4", "s3_super8").

Which attention kernel a case runs rests on reading attn3_launch (csrc/attn_bf16x3.hip), not on the profiler: the tag
`attn_bf16x3_kernel<terms>` is the same for all three.  attn3_launch takes attn_bf16x3_p16_kernel when "attn_m16" is 2 (or 1 with
terms 6 / 9); otherwise attn_bf16x3_pipe_kernel when "attn_pipe" is 2 (or 1 with terms 6 / 9); otherwise attn_bf16x3_kernel.  KERNELS
below holds the keys that force each of them for every `terms`.

Every bound is one the project already uses for the operation (named where it is used) or one measured against fp64, with the
measurement and its margin beside it."""
import math

import numpy as np
import pytest
import torch

from _attn_kit import (attn_case, attn_ref, attn_ref_e4m3, h2_decode, qkv_image, run_attn, run_attn_fp8, split3_decode)
from _kit import dev  # noqa: F401  (fixture)
from _tune import tuned
from conftest import rel_err
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

# the tune keys that make attn3_launch take each kernel whatever `terms` is
KERNELS = {"attn_bf16x3_kernel": {"attn_m16": 0, "attn_pipe": 0},
           "attn_bf16x3_pipe_kernel": {"attn_m16": 0, "attn_pipe": 2},
           "attn_bf16x3_p16_kernel": {"attn_m16": 2}}
TERMS = [6, 9, 1, 3]
# (B, N, H, n_query)
SHAPES = [(1, 5, 4, 5),          # shorter than a key tile and a query tile
          (2, 64, 4, 64),        # exactly one key tile
          (2, 37, 4, 37),        # the prompt length
          (2, 133, 4, 128),      # ragged keys; queries end on the 128-row block edge
          (1, 200, 4, 1),        # one query
          (1, 129, 8, 128),      # a one-key tail tile
          (1, 257, 4, 257)]      # three query blocks, a one-row last block, a one-key tail tile


def _shape_id(s):
    return "B%d-N%d-H%d-q%d" % s


def _check_error(terms, e, e32, absolute_cap=True):
    """the project's rules: test_attention_bf16x3 / test_attention_m16_shape (terms 6, 9, 1), test_attention_f16x2 (terms 3)"""
    if terms == 1:
        assert e < 2e-2, e
        return
    k = 3.0 if terms == 3 else 2.0
    if absolute_cap:
        assert e < k * 1e-6, (e, e32)
    assert e < k * e32 + 2e-7, (e, e32)


def _randn_case(dev, B, N, H, scale=1.5, seed=None):
    seed = 1000 * B + 7 * N + H if seed is None else seed
    make = lambda: torch.randn(B * N, 3 * H * 64, generator=torch.Generator().manual_seed(seed)) * scale
    return attn_case(dev, ("randn", scale, seed), make, B, N, H)


def _fp32_out(dev, c, kernel, terms, B, N, H, nq):
    """the fp32-output call of one kernel into a buffer prefilled with 7.0, on the host"""
    out = torch.full((B, N, H * 64), 7.0, device=dev)
    with tuned(**KERNELS[kernel]):
        run_attn(dev, c.img[terms], c.scale[terms], terms, B, N, H, nq, out=out)
    return out.cpu()


# ------------------------------------------------------------------------------------------------- A. kernel x mode x output form
@pytest.mark.parametrize("shape", SHAPES, ids=_shape_id)
@pytest.mark.parametrize("terms", TERMS, ids=lambda t: "terms%d" % t)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_attention_kernel_mode_edges(dev, kernel, terms, shape):
    """Each of the three split-operand attention kernels in each operand mode (six / nine / one bf16-plane terms, f16x2), fp32 and
    operand-image output: against fp64 next to the fp32-MFMA kernel's own error, rows past n_query untouched, image == fp32 output."""
    from multimodal_diffusion_amd import _lib as L
    B, N, H, nq = shape
    d = H * 64
    c = _randn_case(dev, B, N, H)
    out = _fp32_out(dev, c, kernel, terms, B, N, H, nq)
    e, e32 = rel_err(out[:, :nq], c.ref[:, :nq]), rel_err(c.y32[:, :nq], c.ref[:, :nq])
    print(f"{kernel} terms {terms} {_shape_id(shape)}: err {e:.3e} (fp32-MFMA {e32:.3e})")
    _check_error(terms, e, e32)
    assert torch.all(out[:, nq:] == 7.0)
    oimg = torch.zeros(L.lib().avd_split3_bytes(B * N, d), dtype=torch.uint8, device=dev)
    with tuned(**KERNELS[kernel]):
        run_attn(dev, c.img[terms], c.scale[terms], terms, B, N, H, nq, out_img=oimg)
    want = out.double().numpy()[:, :nq]
    if terms == 3:
        planes = h2_decode(oimg.cpu().numpy(), B * N, d).reshape(2, B, N, d)
        got = planes.sum(0) / c.scale[3]
        assert np.abs(got[:, :nq] - want).max() <= 2.0 ** -21 * np.abs(want).max()
    else:
        planes = split3_decode(oimg.cpu().numpy(), B * N, d).astype(np.float64).reshape(3, B, N, d)
        assert np.array_equal(planes.sum(0)[:, :nq], want)
    assert not planes[:, :, nq:].any()


# ------------------------------------------------------------------------------------------------- B. hard inputs
def _four_heads(make2):
    """The hard inputs are stated for two heads, [N, 3 * 128]; the in_proj epilogue that writes the q|k|v image needs 3 * heads * 64 to
    be a multiple of 256, so they run with four: make2(0) in heads 0 and 1, make2(1) (the same construction from another seed) in heads 2
    and 3 — the two-head input is computed unchanged, next to a second one."""
    a, b = make2(0), make2(1)
    return torch.cat([t[:, 128 * i:128 * i + 128] for i in range(3) for t in (a, b)], 1)


def _spiky(pos, second, N=200):
    """test_attention_spiky_scores's construction for both heads: query 3 scaled by 6, key `pos` aligned with it"""
    qkv = torch.randn(N, 3 * 128, generator=torch.Generator().manual_seed(5 + 100 * second))
    for h in range(2):
        qkv[3, 64 * h:64 * h + 64] *= 6.0
        qkv[pos, 128 + 64 * h:128 + 64 * h + 64] = qkv[3, 64 * h:64 * h + 64]
    return qkv


def _equal_keys(N, second):
    qkv = torch.randn(N, 3 * 128, generator=torch.Generator().manual_seed(11 + N + 100 * second)) * 1.5
    qkv[:, 128:256] = qkv[0, 128:256].clone()
    return qkv


@pytest.mark.parametrize("pos", [0, 170, 199], ids=lambda p: "key%d" % p)
@pytest.mark.parametrize("terms", [6, 3], ids=lambda t: "terms%d" % t)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_attention_dominant_key(dev, kernel, terms, pos):
    """One key dominates query 3's row — in the first tile, in a late full tile, as the last key of the ragged tail tile: the
    online-softmax rescale across tiles and the tail mask next to the largest score."""
    B, N, H = 1, 200, 4
    c = attn_case(dev, ("spiky", pos), lambda: _four_heads(lambda second: _spiky(pos, second)), B, N, H)
    p3 = torch.softmax((c.qkv[3, :64].double() @ c.qkv[:, 256:320].double().T) / 8.0, -1)
    assert p3[pos] > 0.99                                         # the input is what it claims to be
    out = _fp32_out(dev, c, kernel, terms, B, N, H, N)
    e, e32 = rel_err(out, c.ref), rel_err(c.y32, c.ref)
    print(f"{kernel} terms {terms} dominant key {pos}: err {e:.3e} (fp32-MFMA {e32:.3e})")
    _check_error(terms, e, e32)


@pytest.mark.parametrize("N", [200, 65])
@pytest.mark.parametrize("terms", [6, 3], ids=lambda t: "terms%d" % t)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_attention_equal_keys(dev, kernel, terms, N):
    """All keys of a head are the same: softmax is uniform and the output is the mean of v; a tail mask off by one key moves the
    divisor by 1 / N (5e-3 at N = 200, 1.5e-2 at N = 65: four orders above the tolerance)."""
    B, H = 1, 4
    c = attn_case(dev, ("equal", N), lambda: _four_heads(lambda second: _equal_keys(N, second)), B, N, H)
    mean_v = c.qkv[:, 2 * H * 64:].double().mean(0)
    assert rel_err(c.ref[0], mean_v.expand(N, -1)) < 1e-12
    out = _fp32_out(dev, c, kernel, terms, B, N, H, N)
    e, e32 = rel_err(out, c.ref), rel_err(c.y32, c.ref)
    print(f"{kernel} terms {terms} equal keys N {N}: err {e:.3e} (fp32-MFMA {e32:.3e})")
    _check_error(terms, e, e32)


@pytest.mark.parametrize("terms", [6, 3], ids=lambda t: "terms%d" % t)
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_attention_wide_scores(dev, kernel, terms):
    """qkv = randn * 4: scores of standard deviation ~16, most probabilities underflow in the exp2 domain, rows nearly one-hot.
    max|ref| is 17.2 and plain fp32 attention is itself 2.5e-6 off fp64 on the CPU (heads 0 and 1, seed 7), so the absolute 2e-6 cap
    of the N(0, 1.5^2) tests does not apply: the error is held to the fp32-MFMA kernel's on the same input (2x, f16x2 3x, + 2e-7), and
    that kernel to its own tolerance in test_attention (2e-5).
    Measured on an MI355X (relative to max|ref|; the fp32-MFMA kernel: e32 = 4.11e-6):
      attn_bf16x3_kernel        terms 6: 2.68e-6   terms 3: 3.19e-6
      attn_bf16x3_pipe_kernel   terms 6: 2.68e-6   terms 3: 3.19e-6
      attn_bf16x3_p16_kernel    terms 6: 2.60e-6   terms 3: 2.59e-6"""
    B, N, H = 1, 200, 4
    make2 = lambda second: torch.randn(N, 3 * 128, generator=torch.Generator().manual_seed(7 + 100 * second)) * 4.0
    c = attn_case(dev, "wide", lambda: _four_heads(make2), B, N, H)
    out = _fp32_out(dev, c, kernel, terms, B, N, H, N)
    e, e32 = rel_err(out, c.ref), rel_err(c.y32, c.ref)
    print(f"{kernel} terms {terms} wide scores: err {e:.3e} (fp32-MFMA {e32:.3e}), max|ref| {float(c.ref.abs().max()):.3g}")
    assert e32 < 2e-5
    _check_error(terms, e, e32, absolute_cap=False)


@pytest.mark.parametrize("N", [133, 5])
@pytest.mark.parametrize("terms", [6, 3], ids=lambda t: {6: "bf16x3_image", 3: "f16x2_image"}[t])
@pytest.mark.parametrize("kernel", list(KERNELS))
def test_attention_poisoned_padding(dev, kernel, terms, N):
    """The kernels fetch rows past N from token N - 1 and mask the tail scores; they must never read a padding slot of the q|k|v image.
    With every slot the in_proj epilogue leaves alone holding 0xFF bytes (a NaN in every plane, bf16 and fp16 alike) the output is
    bit-identical to the run on a zero-prefilled image, and finite."""
    B, H = 2, 4
    kind = "f16x2" if terms == 3 else "bf16x3"
    qkv = torch.randn(B * N, 3 * H * 64, generator=torch.Generator().manual_seed(77 + N)) * 1.5
    outs = []
    for fill in (0x00, 0xFF):
        img, scale = qkv_image(dev, qkv, B, N, H, kind, fill=fill)
        out = torch.full((B, N, H * 64), 7.0, device=dev)
        with tuned(**KERNELS[kernel]):
            run_attn(dev, img, scale, terms, B, N, H, N, out=out)
        outs.append(out)
    assert torch.isfinite(outs[1]).all()
    assert torch.equal(outs[0], outs[1])
    assert rel_err(outs[0].cpu(), attn_ref(qkv, B, N, H)) < 3e-6          # and the clean run is the operation (not all 7.0)


@pytest.mark.parametrize("N", [133, 5])
@pytest.mark.parametrize("kind", ["bf16x3_image", "f16x2_image"])
def test_attention_fp8_poisoned_padding(dev, kind, N):
    """The same guarantee for the fp8 path: quant_fp8_kernel reads rows past N from token N - 1 and writes zeros for them; image and
    workspace prefilled with 0xFF (NaN in bf16, fp16 and e4m3)."""
    from multimodal_diffusion_amd import _lib as L
    B, H = 2, 4
    kind = kind[:-6]
    qkv = torch.randn(B * N, 3 * H * 64, generator=torch.Generator().manual_seed(78 + N)) * 1.5
    outs = []
    for fill in (0x00, 0xFF):
        img, scale = qkv_image(dev, qkv, B, N, H, kind, fill=fill)
        ws = torch.full((L.lib().avd_attn_fp8_workspace_bytes(B, N, H),), fill, dtype=torch.uint8, device=dev)
        out = torch.full((B, N, H * 64), 7.0, device=dev)
        run_attn_fp8(dev, img, scale, kind, ws, B, N, H, N, out=out)
        outs.append(out)
    assert torch.isfinite(outs[1]).all()
    assert torch.equal(outs[0], outs[1])
    assert rel_err(outs[0].cpu(), attn_ref(qkv, B, N, H)) < 0.15           # the clean run is the operation (a wrong map gives O(1))


# ------------------------------------------------------------------------------------------------- C. fp8 attention, directly
def _fp8_case(dev, B, N, H):
    """inputs and seeds of test_attention_fp8_reported_error, with its two references"""
    def make():
        return torch.randn(B * N, 3 * H * 64, generator=torch.Generator().manual_seed(B * 100 + N + H)) * 1.5
    c = attn_case(dev, "fp8", make, B, N, H)
    if not hasattr(c, "ref8"):
        c.ref8 = attn_ref_e4m3(c.qkv, B, N, H)
    return c


def _fp8_out(dev, c, kind, B, N, H, nq):
    from multimodal_diffusion_amd import _lib as L
    terms = 3 if kind == "f16x2" else 6
    ws = torch.empty(L.lib().avd_attn_fp8_workspace_bytes(B, N, H), dtype=torch.uint8, device=dev)
    out = torch.full((B, N, H * 64), 7.0, device=dev)
    run_attn_fp8(dev, c.img[terms], c.scale[terms], kind, ws, B, N, H, nq, out=out)
    return out.cpu(), ws


# bounds of test_attention_fp8_reported_error for the same inputs (1.3x resp. 2x of its measurements on the bf16x3 image); measured
# here through the f16x2 quantiser: err 8.23e-2 / 7.68e-2, err8 6.27e-3 / 1.13e-2 for N = 64 / 133 — what that test measured on the bf16x3
# image, so its bounds stand unchanged
@pytest.mark.parametrize("B,N,H,bound,bound8", [(1, 64, 4, 0.11, 1.3e-2), (2, 133, 4, 0.10, 2.3e-2)],
                         ids=["quant_fp8_f16x2-fp32_out-N64", "quant_fp8_f16x2-fp32_out-N133"])
def test_attention_fp8_f16x2_image_in(dev, B, N, H, bound, bound8):
    """avd_attn_fwd_fp8_f16x2_f32 with fp32 output: quant_fp8_kernel<true> reads the f16x2 image; everything after it is the
    arithmetic of the bf16x3-image call, so that call's bounds hold — against fp64 on the fp32 operands (err) and on the e4m3-rounded
    q, k, v and p (err8)."""
    c = _fp8_case(dev, B, N, H)
    out, _ = _fp8_out(dev, c, "f16x2", B, N, H, N)
    err, err8 = rel_err(out, c.ref), rel_err(out, c.ref8)
    print(f"fp8 attention, f16x2 image in, B={B} N={N} H={H}: rel err vs fp64 {err:.3e}, vs fp64 on the e4m3 operands {err8:.3e}")
    assert err < bound and err8 < bound8


@pytest.mark.parametrize("B,N,H", [(1, 64, 4), (2, 133, 4)], ids=["N64", "N133"])
@pytest.mark.parametrize("kind", ["attn_fp8_kernel_1-bf16x3_image_out", "attn_fp8_kernel_2-f16x2_image_out"])
def test_attention_fp8_image_outputs(dev, kind, B, N, H):
    """attn_fp8_kernel<1> (bf16x3 image) and <2> (f16x2 image): the image-output call holds the values of the fp32-output call of
    the same kernel on the same input — exactly in three bf16 planes, to 2^-21 of max|out| in two fp16 planes — and writes nothing at
    rows >= n_query."""
    from multimodal_diffusion_amd import _lib as L
    kind = "f16x2" if "f16x2" in kind else "bf16x3"
    terms = 3 if kind == "f16x2" else 6
    d, nq = H * 64, N - 5
    c = _fp8_case(dev, B, N, H)
    out, ws = _fp8_out(dev, c, kind, B, N, H, nq)
    assert torch.all(out[:, nq:] == 7.0)
    assert rel_err(out[:, :nq], c.ref[:, :nq]) < 0.15                      # the fp32 output is the operation
    oimg = torch.zeros(L.lib().avd_split3_bytes(B * N, d), dtype=torch.uint8, device=dev)
    run_attn_fp8(dev, c.img[terms], c.scale[terms], kind, ws, B, N, H, nq, out_img=oimg)
    want = out.double().numpy()[:, :nq]
    if kind == "f16x2":
        planes = h2_decode(oimg.cpu().numpy(), B * N, d).reshape(2, B, N, d)
        got = planes.sum(0) / c.scale[3]
        assert np.abs(got[:, :nq] - want).max() <= 2.0 ** -21 * np.abs(want).max()
    else:
        planes = split3_decode(oimg.cpu().numpy(), B * N, d).astype(np.float64).reshape(3, B, N, d)
        assert np.array_equal(planes.sum(0)[:, :nq], want)
    assert not planes[:, :, nq:].any()


# err8 bounds at 2x the measurement (the margin of test_attention_fp8_reported_error: the residue depends on where the running maximum
# moves); measured on an MI355X: N = 5 err 1.04e-1, err8 5.47e-5 (one tile: p is rounded against the final row maximum, as the reference
# does, and the residue is fp32 rounding); N = 200 with one query err 6.54e-2, err8 8.45e-3
@pytest.mark.parametrize("B,N,H,nq,bound8", [(1, 5, 4, 5, 1.1e-4), (1, 200, 4, 1, 1.7e-2)], ids=["B1-N5-H4-q5", "B1-N200-H4-q1"])
def test_attention_fp8_small_and_single_query(dev, B, N, H, nq, bound8):
    """Sizes of the bf16x3-image fp8 call that had no bound: fewer tokens than a tile, and one query."""
    c = _fp8_case(dev, B, N, H)
    out, _ = _fp8_out(dev, c, "bf16x3", B, N, H, nq)
    err, err8 = rel_err(out[:, :nq], c.ref[:, :nq]), rel_err(out[:, :nq], c.ref8[:, :nq])
    print(f"fp8 attention B={B} N={N} H={H} n_query={nq}: rel err vs fp64 {err:.3e}, vs fp64 on the e4m3 operands {err8:.3e}")
    assert err < 0.15                      # a wrong operand map gives O(1)
    assert err8 < bound8
    assert torch.all(out[:, nq:] == 7.0)


# ------------------------------------------------------------------------------------------------- D. GEMM keys
@pytest.mark.parametrize("M,N,K", [(130, 128, 64), (300, 512, 512), (1000, 192, 96)])        # K = 64 / 96: two / three K tiles
@pytest.mark.parametrize("mode", ["plain", "gelu", "res"])
@pytest.mark.parametrize("stages", [2, 3], ids=lambda s: "gemm_stages%d" % s)
@pytest.mark.parametrize("tile", [1, 2], ids=lambda t: "gemm_tile%d" % t)
def test_gemm_ring_depth(dev, tile, stages, mode, M, N, K):
    """The two- and three-stage LDS ring of the 128x64 and the 64x64 fp32 tile, forced: at test_gemm's tolerance against fp64, with
    fewer K tiles than stages, as many, and many more."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    g = torch.Generator().manual_seed(M * 7 + N + K)
    x = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    ref = R.linear(x.double(), w.double(), b.double())
    if mode == "gelu":
        ref = R.gelu_erf(ref)
    if mode == "res":
        ref = ref + r.double()
    with tuned(gemm_tile=tile, gemm_stages=stages):
        y = Fn.linear(x.to(dev), w.to(dev), b.to(dev), act=L.ACT_GELU if mode == "gelu" else L.ACT_NONE,
                      residual=r.to(dev) if mode == "res" else None)
    assert rel_err(y.cpu(), ref) < 2e-5


_S3_BASE = {}


def _s3_operands(dev, N):
    """x [2701, 48], W [N, 48], bias, residual on the device, the fp64 x W^T + b + r, and — per mode — the fp32 result and the GELU
    image with every tune key at its default"""
    if N not in _S3_BASE:
        M, K = 2701, 48
        g = torch.Generator().manual_seed(2701 + N)
        x = torch.randn(M, K, generator=g).to(dev)
        w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dev)
        b = torch.randn(N, generator=g).to(dev)
        r = torch.randn(M, N, generator=g).to(dev)
        ref = (x.double() @ w.double().T + b.double() + r.double()).cpu()
        _S3_BASE[N] = dict(x=x, w=w, b=b, r=r, ref=ref)
        for mode in ("bf16x3", "f16x2"):
            _S3_BASE[N][mode] = _s3_run(dev, _S3_BASE[N], mode, N)
    return _S3_BASE[N]


def _s3_run(dev, o, mode, N):
    """(fp32 x W^T + b + r, decoded planes of the image of gelu(x W^T + b)) on the host"""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    M, K = 2701, 48
    if mode == "f16x2":
        x2, sx = Fn.split_f16x2(o["x"])
        w2, sw = Fn.split_f16x2(o["w"])
        y = Fn.linear_f16x2(x2, M, w2, N, K, sx * sw, bias=o["b"], residual=o["r"])
        img = Fn.linear_f16x2(x2, M, w2, N, K, sx * sw, bias=o["b"], act=L.ACT_GELU, out_scale=64.0)
        return y.cpu(), h2_decode(img.cpu().numpy(), M, N)
    x3, w3 = Fn.split3(o["x"]), Fn.split3(o["w"])
    y = Fn.linear_bf16x3(x3, M, w3, N, K, bias=o["b"], residual=o["r"])
    img = Fn.linear_bf16x3(x3, M, w3, N, K, bias=o["b"], act=L.ACT_GELU, out_split3=True)
    return y.cpu(), split3_decode(img.cpu().numpy(), M, N)


# (s3_tile, N, s3_sn, super-tile key, value): the super-tile of 256-row x 128 / 256-column blocks that results, for 11 block rows
SUPERTILES = [(1, 512, 2, "s3_super4", 8),       # 4 x 2, super-rows of 4 + 4 + 3 block rows
              (1, 1536, 3, "s3_super4", 6),      # 2 x 3, ragged 1
              (1, 1536, 4, "s3_super4", 4),      # 1 x 4
              (0, 512, 1, "s3_super8", 3),       # 3 x 1, ragged 2
              (0, 1536, 2, "s3_super8", 1)]      # total < sn: sm clamps to 1


@pytest.mark.parametrize("mode", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("tile,N,sn,skey,total", SUPERTILES, ids=["s3_tile%d-N%d-s3_sn%d-%s_%d" % s for s in SUPERTILES])
def test_split_gemm_supertile_map(dev, tile, N, sn, skey, total, mode):
    """The block-to-tile map s3_block_of under super-tile shapes no default gives (ragged last super-row, one-row and one-column
    super-tiles, a total below the width).  Each output element's summation order does not depend on the map, so the fp32 result and the
    image are bit-identical to the default-key ones (rows < M: the image's rows past M are never written); and the fp32 result is
    within test_split_gemm_tile_configurations_agree's 3e-6 of fp64.  tests/test_host_cpu.py shows on the CPU that the map is a
    bijection onto the block grid for these settings, so a mismatch here is a kernel bug, not a bad key."""
    o = _s3_operands(dev, N)
    y0, planes0 = o[mode]
    with tuned(**{"s3_tile": tile, "s3_sn": sn, skey: total}):
        y, planes = _s3_run(dev, o, mode, N)
    assert torch.equal(y, y0)
    assert rel_err(y, o["ref"]) < 3e-6
    assert np.array_equal(planes, planes0)
