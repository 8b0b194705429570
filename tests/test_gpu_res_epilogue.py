"""The residual + image + sums-of-squares epilogue of the split-operand GEMMs (csrc/s3_common.h: s3_epilogue_res, out_proj / fc2 of the
bf16x3 core), stand-alone through avd_gemm_bf16x3_res_img_f32 and, with the fp32 stream alone, through avd_gemm_bf16x3_f32 with a
residual.  The epilogue loads a whole row-tile pair's residual ahead of the stores of the pair before it, where a wave's rows are all
inside M, and keeps the serial order where rows need a guard; the stream is updated in place (R == C), so what is checked first is that
this order shows nowhere: in place and out of place give the same bits.  N = 512; K = 32 is two k-tiles (the loop is tail steps only),
K = 512 has main steps as well."""
from functools import lru_cache
from types import SimpleNamespace

import math
import numpy as np
import pytest
import torch

from _attn_kit import split3_decode
from _kit import dev, engine, modules, ts, video_case  # noqa: F401  (dev is a fixture)
from _tune import tuned
from conftest import rel_err
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

N = 512
PAD = 64
# one block per CU kernels (128 x 128 wave tile with 6 / 7 / 8 row tiles, 8 waves with 7 / 8), then the four-wave blocks of 2 / 5 / 8 row tiles
KEYS = {f"tile0 rt{rt} w128={w}": dict(s3_tile=0, s3_rt=rt, s3_w128=w) for rt in (6, 7, 8) for w in (1, 0)}
KEYS.update({f"tile1 rt4={rt}": dict(s3_tile=1, s3_rt4=rt) for rt in (2, 5, 8)})
KEYS["auto"] = {}
ROWS = (1, 33, 225, 300)       # 225: one 224-row block and a block with a single live row
RULE_M = 24321                 # the smallest row count at which the rule itself takes the 128 x 128 wave tile at N = 512
CASES = [(k, M, K) for k in KEYS if k != "auto" for M in ROWS for K in (32, 512)] + [("auto", RULE_M, K) for K in (32, 512)]
IDS = [f"{k} M{M} K{K}" for k, M, K in CASES]


@lru_cache(maxsize=None)
def operands(M, K):
    """x [M, K], w [N, K], bias, residual [M, N] (the scales of test_gemm_bf16x3_fp32_accuracy) and the two operand images"""
    from multimodal_diffusion_amd import functional as Fn
    d = torch.device("cuda:0")
    g = torch.Generator().manual_seed(M + N + K)
    x = torch.randn(M, K, generator=g) * 3.0
    w = torch.randn(N, K, generator=g) / math.sqrt(K)
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g)
    return SimpleNamespace(M=M, K=K, x=x, w=w, b=b, r=r, x3=Fn.split3(x.to(d)), w3=Fn.split3(w.to(d)), bias=b.to(d))


def arena(c, fill):
    """R, C, the image of C and ss_out for M + PAD rows inside ONE tensor of `fill` bytes; R rows < M hold the residual"""
    from multimodal_diffusion_amd import _lib as L
    rows = c.M + PAD
    sizes = [rows * N * 4, rows * N * 4, L.lib().avd_split3_bytes(rows, N), rows * (N // 64) * 4]
    offs = np.cumsum([0] + [(s + 255) // 256 * 256 for s in sizes])
    buf = torch.full((int(offs[-1]),), fill, dtype=torch.uint8, device=c.x3.device)
    part = [buf[int(o):int(o) + s] for o, s in zip(offs, sizes)]
    a = SimpleNamespace(buf=buf, R=part[0].view(torch.float32).view(rows, N), C=part[1].view(torch.float32).view(rows, N), img=part[2],
                        ss=part[3].view(torch.float32).view(rows, N // 64))
    a.R[:c.M] = c.r.to(buf.device)
    return a


def run(c, keys, in_place, fill=0, image=True):
    """one launch -> (C [M + PAD, N], image planes [3, M + PAD, N], ss_out [M + PAD, N / 64]) on the host, the image and the sums as
    uint16 / int32 bit patterns where `fill` makes the untouched rows NaN"""
    from multimodal_diffusion_amd import _lib as L
    a = arena(c, fill)
    out = a.R if in_place else a.C
    st = L.stream_ptr(a.buf.device)
    with tuned(**keys):
        if image:
            L.check(L.lib().avd_gemm_bf16x3_res_img_f32(c.x3.data_ptr(), c.w3.data_ptr(), c.bias.data_ptr(), a.R.data_ptr(), out.data_ptr(),
                                                        a.img.data_ptr(), a.ss.data_ptr(), c.M, N, c.K, st))
        else:
            L.check(L.lib().avd_gemm_bf16x3_f32(c.x3.data_ptr(), c.w3.data_ptr(), c.bias.data_ptr(), a.R.data_ptr(), out.data_ptr(), None,
                                                c.M, N, c.K, L.ACT_NONE, 6, st))
    torch.cuda.synchronize()
    planes = split3_decode(a.img.cpu().numpy(), c.M + PAD, N) if image else None
    other = a.C if in_place else a.R           # the buffer the launch must not have written
    return SimpleNamespace(C=out.cpu(), planes=planes, ss=a.ss.cpu(), other=other.cpu())


def bits(t):
    return t.contiguous().view(torch.int32)


@lru_cache(maxsize=None)
def result(keys_id, M, K):
    """the out-of-place launch on zero-filled padding: shared by the tests below"""
    return run(operands(M, K), KEYS[keys_id], in_place=False)


@lru_cache(maxsize=None)
def reference(M, K):
    """fp64: x w^T + bias + residual"""
    c = operands(M, K)
    return R.linear(c.x.double(), c.w.double(), c.b.double()) + c.r.double()


# ---- 1. in place equals out of place
@pytest.mark.parametrize("keys_id,M,K", CASES, ids=IDS)
def test_in_place_equals_out_of_place(dev, keys_id, M, K):
    c = operands(M, K)
    sep = result(keys_id, M, K)
    inp = run(c, KEYS[keys_id], in_place=True)
    assert torch.isfinite(sep.C[:M]).all()
    assert torch.equal(bits(inp.C[:M]), bits(sep.C[:M]))
    assert np.array_equal(inp.planes[:, :M].view(np.uint32), sep.planes[:, :M].view(np.uint32))
    assert torch.equal(bits(inp.ss[:M]), bits(sep.ss[:M]))
    assert torch.equal(sep.other[:M], c.r)                       # out of place: the residual operand is read only
    # the fp32 stream alone (no image, no sums: the last layer's fc2)
    sep1, inp1 = run(c, KEYS[keys_id], in_place=False, image=False), run(c, KEYS[keys_id], in_place=True, image=False)
    assert torch.equal(bits(inp1.C[:M]), bits(sep.C[:M])) and torch.equal(bits(sep1.C[:M]), bits(sep.C[:M]))


# ---- 2. rows past M are neither used nor written
@pytest.mark.parametrize("keys_id,M,K", CASES, ids=IDS)
def test_rows_past_m_are_neither_used_nor_written(dev, keys_id, M, K):
    c = operands(M, K)
    zero = result(keys_id, M, K)
    for in_place in (False, True):
        nan = run(c, KEYS[keys_id], in_place=in_place, fill=0xFF)          # every fp32 and every bf16 past M is a NaN (all bits set)
        assert (bits(nan.C[M:]) == -1).all() and (bits(nan.ss[M:]) == -1).all() and (bits(nan.other[M:]) == -1).all()
        assert (nan.planes[:, M:].view(np.uint32) == 0xFFFF0000).all()
        assert torch.isfinite(nan.C[:M]).all() and torch.isfinite(nan.ss[:M]).all() and np.isfinite(nan.planes[:, :M]).all()
        assert torch.equal(bits(nan.C[:M]), bits(zero.C[:M])) and torch.equal(bits(nan.ss[:M]), bits(zero.ss[:M]))
        assert np.array_equal(nan.planes[:, :M].view(np.uint32), zero.planes[:, :M].view(np.uint32))
        if in_place:
            assert (bits(nan.other) == -1).all()                             # the buffer that is neither R nor C: untouched everywhere


# ---- 3. the image is the stream, the sums are its sums
@pytest.mark.parametrize("keys_id,M,K", CASES, ids=IDS)
def test_image_and_sums_are_the_stream(dev, keys_id, M, K):
    res = result(keys_id, M, K)
    C = res.C[:M].double()
    assert np.array_equal(res.planes[:, :M].astype(np.float64).sum(0), C.numpy())            # h + m + l == fp32 output, exactly
    chunks = C.view(M, N // 64, 64).pow(2).sum(-1)
    assert rel_err(res.ss[:M], chunks) < 1e-5           # the bound of test_gemm_rmsfold_epilogue_direct for the folded norm's sums


# ---- 4. against the reference
@pytest.mark.parametrize("keys_id,M", [(k, 300) for k in KEYS if k != "auto"] + [("auto", RULE_M)])
@pytest.mark.parametrize("K", [32, 512])
def test_against_fp64(dev, keys_id, M, K):
    """the bounds of test_gemm_bf16x3_fp32_accuracy: 2e-6 of the largest output, and no worse than 1.5 x the fp32 MFMA GEMM"""
    from multimodal_diffusion_amd import functional as Fn
    c, ref = operands(M, K), reference(M, K)
    y32 = Fn.linear(c.x.to(dev), c.w.to(dev), c.bias, residual=c.r.to(dev)).cpu()
    e3 = (result(keys_id, M, K).C[:M].double() - ref).abs().max().item()
    e32 = (y32.double() - ref).abs().max().item()
    assert e3 <= 2e-6 * ref.abs().max().item()
    assert e3 <= 1.5 * e32 + 1e-7, (e3, e32)


# ---- a wave gives the same bits through the batched order (all its rows inside M) and through the guarded serial order
@pytest.mark.parametrize("keys_id", [k for k in KEYS if k != "auto"])
@pytest.mark.parametrize("K", [32, 512])
def test_guarded_and_unguarded_waves_agree(dev, keys_id, K):
    """M = 300: rows 256 .. 299 (224 .. 299) lie in a wave that ends past M.  The same rows as the head of 512 rows lie in waves that
    are whole."""
    from multimodal_diffusion_amd import functional as Fn
    short, M2 = operands(300, K), 512
    g = torch.Generator().manual_seed(K)
    x = torch.cat([short.x, torch.randn(M2 - 300, K, generator=g) * 3.0])
    r = torch.cat([short.r, torch.randn(M2 - 300, N, generator=g)])
    whole = SimpleNamespace(M=M2, K=K, x=x, w=short.w, b=short.b, r=r, x3=Fn.split3(x.to(dev)), w3=short.w3, bias=short.bias)
    a, b = result(keys_id, 300, K), run(whole, KEYS[keys_id], in_place=True)
    assert torch.equal(bits(b.C[:300]), bits(a.C[:300])) and torch.equal(bits(b.ss[:300]), bits(a.ss[:300]))
    assert np.array_equal(b.planes[:, :300].view(np.uint32), a.planes[:, :300].view(np.uint32))


# ---- 5. the trimmed last block: residual rows through the two-segment row map (r_seg > 0, the only caller with rrow != m)
def test_trimmed_last_block_row_map(dev):
    """a 3-layer step with the null-dedup route on against the route off, as tests/test_gpu_null_dedup.py sets it up: the same latent"""
    from multimodal_diffusion_amd import _lib as L
    mods = modules(dev, R.synth_weights(seed=0, n_layers=3), 3)
    z, za, npr = video_case(dev, B=2, W=32)
    tn, tp = ts([981, 402], dev), ts([961, 382], dev)
    out = {}
    with tuned(s3_min_rows=0):
        eng = engine(mods, "video", tuple(z.shape), npr, guidance=3.5, matmul="bf16x3")
        eng.set_prompt(za)
        for on in (0, 1):
            prev = L.lib().avd_cfg_dedup_set(on)
            try:
                out[on] = eng.step(z, tn, tp).clone()
            finally:
                L.lib().avd_cfg_dedup_set(prev)
    assert torch.isfinite(out[0]).all()
    assert torch.equal(out[1], out[0]), float((out[1] - out[0]).abs().max())
