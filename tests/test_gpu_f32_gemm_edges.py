"""The fp32 GEMM (csrc/gemm_f32.hip: avd_gemm_bias_act_f32, avd_gemm_rmsfold_f32) at the edges of its dispatch, called through the C ABI
with leading dimensions, pointer offsets and activations that Fn.linear never passes.

A. the LDS-DMA kernel on every tile (gemm_tile 0 / 1 / 2) and ring depth (gemm_stages 2 / 3): one K tile (K = 32), ragged and exact
   column blocks on each block width, M one short of, at and one past each block height; lda / ldr / ldc larger than the rows, NaN in
   the padding of A and R, a sentinel in the padding of C; R aliased with C; rows of a run at M = 257 against a run at M = 37;
B. the register kernel, one case per reason gemm_f32_fold has to take it (the REG table);
C. the refusals the host makes before a launch, and M == 0;
D. the folded-RMSNorm epilogues (Fn.linear_rmsfold) at ss_in_cols 4, 8 (the generic loop), 16 (the four-load path) and 1, at tiny and
   ragged M, on every tile.

Which kernel ran is asserted from the profiler tags that launch_dma / launch_reg register (the kernel names with their template
arguments), so a case that moves to another route fails.

Two kinds of operands.  Integers from [-8, 8] with K <= 160: every product and partial sum is below 64 K + 16 < 2^24, exact in fp32
in any order, and the result must be bit-equal to the int64 reference (no tolerance: one wrong row, column, K chunk or stride is a
mismatch).  randn operands with W / sqrt(K) for the cases with an activation, against fp64 with conftest.rel_err < 2e-5, test_gemm's
bound for the same operation (test_gpu_parity.py); the folded pair uses test_gemm_rmsfold_epilogue_direct's 2e-5 and 1e-5.

Largest rel_err measured on the MI355X over this module's cases (printed by the tests as they run; bounds are not taken from these):
      LDS-DMA kernel, GELU                        3.2e-7
      LDS-DMA kernel, plain / residual (randn)    3.0e-7 / 2.6e-7
      register kernel, SiLU                       1.9e-7   (21,761 x 258 x 64: 3.2e-7)
      register kernel, GELU + residual            1.7e-7
      folded pair: x1 7.4e-7, ss_out 1.2e-7, y 1.1e-6, y from the one-column table 1.1e-6
The one large case, the <128, 128, 64, 64> register block at 21,761 x 258 (513 blocks: the instantiation needs >= 512), takes 0.1 s
per case on the MI355X; its int64 reference is one matmul on the CPU, built once for the module."""
import math
from functools import lru_cache
from types import SimpleNamespace

import pytest
import torch

from _kit import dev  # noqa: F401  (fixture)
from _tune import tuned
from conftest import rel_err
from oracle import ref_cpu as R

gpu = pytest.mark.gpu

SENT = -12345.5                       # no sum of integer operands gives it
TOL = 2e-5                            # test_gemm
NONE, GELU, SILU = 0, 1, 2            # AVD_ACT_* (include/avdiff_hip.h)

# gemm_f32_fold: (gemm_tile, gemm_stages) -> "BM, BN, WM, WN", "WPS, NST" of the launch_dma_epi it picks
DMA_CONFIGS = {(0, 0): ("128, 128, 64, 64", "2, 2"),
               (1, 2): ("128, 64, 64, 32", "2, 2"), (1, 3): ("128, 64, 64, 32", "2, 3"),
               (2, 2): ("64, 64, 32, 32", "4, 2"), (2, 3): ("64, 64, 32, 32", "3, 3")}
DMA_SHAPES = [(1, 36, 32), (33, 100, 32), (127, 64, 32), (65, 132, 64), (129, 192, 96), (128, 128, 128), (257, 260, 160)]
EPIS = ["plain", "nobias", "gelu", "res"]
EPI_ID = {"plain": 0, "nobias": 0, "gelu": 1, "res": 2}      # EPI_BIAS, EPI_GELU, EPI_RES

# the register kernel: (name, M, N, K, epilogue, block, how).  how: "ldcN" ldc = N; "c1" / "b1" / "r1" the C / bias / R pointer one float
# into its buffer; "t10" gemm_tile = 10.  Epilogues: EPIS plus "silu" and "gelu_res"; KTAIL is K % 32 != 0.
REG = [("ktail", 70, 64, 4, "plain", "64, 64, 32, 32", ""), ("ktail", 70, 64, 4, "res", "64, 64, 32, 32", ""),
       ("ktail", 70, 64, 28, "plain", "64, 64, 32, 32", ""), ("ktail", 70, 64, 28, "res", "64, 64, 32, 32", ""),
       ("ktail", 130, 96, 100, "plain", "64, 64, 32, 32", ""), ("ktail", 130, 96, 100, "res", "64, 64, 32, 32", ""),
       ("n_le_32", 300, 1, 64, "plain", "128, 32, 32, 32", ""), ("n_le_32", 300, 1, 64, "res", "128, 32, 32, 32", ""),
       ("n_le_32", 300, 7, 36, "plain", "128, 32, 32, 32", ""), ("n_le_32", 300, 7, 36, "res", "128, 32, 32, 32", ""),
       ("n_le_32", 129, 32, 32, "plain", "128, 32, 32, 32", ""), ("n_le_32", 129, 32, 32, "nobias", "128, 32, 32, 32", ""),
       ("n_mod_4", 65, 33, 64, "plain", "64, 64, 32, 32", "ldcN"), ("n_mod_4", 65, 33, 64, "res", "64, 64, 32, 32", "ldcN"),
       ("n_mod_4", 130, 50, 36, "plain", "64, 64, 32, 32", "ldcN"), ("n_mod_4", 130, 50, 36, "res", "64, 64, 32, 32", "ldcN"),
       ("n_mod_4", 64, 127, 32, "plain", "64, 64, 32, 32", "ldcN"), ("n_mod_4", 64, 127, 32, "nobias", "64, 64, 32, 32", "ldcN"),
       ("n_mod_4", 33, 130, 96, "plain", "64, 64, 32, 32", "ldcN"), ("n_mod_4", 33, 130, 96, "res", "64, 64, 32, 32", "ldcN"),
       ("silu", 130, 128, 64, "silu", "64, 64, 32, 32", ""),
       ("gelu_res", 130, 128, 64, "gelu_res", "64, 64, 32, 32", ""),
       ("align4", 130, 128, 64, "plain", "64, 64, 32, 32", "c1"), ("align4", 130, 128, 64, "plain", "64, 64, 32, 32", "b1"),
       ("align4", 130, 128, 64, "res", "64, 64, 32, 32", "r1"),
       ("tile10", 129, 192, 96, "plain", "64, 64, 32, 32", "t10"), ("tile10", 129, 192, 96, "res", "64, 64, 32, 32", "t10"),
       ("block128", 21761, 258, 36, "plain", "128, 128, 64, 64", ""), ("block128", 21761, 258, 36, "res", "128, 128, 64, 64", ""),
       ("block128", 21761, 258, 64, "silu", "128, 128, 64, 64", "")]

INT_EPIS = ("plain", "nobias", "res")
_WORST = {}


def dma_tag(cfg, epi):
    tile, nst = DMA_CONFIGS[cfg]
    return f"gemm_f32_dma_kernel<{tile}, {EPI_ID[epi]}, {nst}>"


def reg_tag(block, K):
    return f"gemm_f32_reg_kernel<{block}, {'true' if K % 32 else 'false'}, false>"


def int_cases():
    """every (M, N, K, epilogue) that runs on integer operands"""
    out = [(M, N, K, e) for (M, N, K) in DMA_SHAPES for e in INT_EPIS]
    out += [(M, N, K, e) for (_, M, N, K, e, _, _) in REG if e in INT_EPIS]
    return sorted(set(out))


# ------------------------------------------------------------------------------------------------- operands and references
def _reference(c, dt):
    y = c.A.to(dt) @ c.W.to(dt).t()
    if c.bias is not None:
        y = y + c.bias.to(dt)
    if c.act == GELU:
        y = R.gelu_erf(y)
    elif c.act == SILU:
        y = y * torch.sigmoid(y)
    return y if c.R is None else y + c.R.to(dt)


@lru_cache(maxsize=None)
def case(M, N, K, epi, kind):
    """Operands on the CPU (fp32) and their reference, built once and never modified.  kind "int": integers from [-8, 8], int64
    reference; the seed is the first from the shape's own for which the reference has a non-zero in every row and column (an all-zero
    row or column is possible by chance at M = 1 or N = 1).  kind "randn": test_gemm's operands, fp64 reference."""
    act = {"gelu": GELU, "gelu_res": GELU, "silu": SILU}.get(epi, NONE)
    has_bias, has_res = epi != "nobias", epi in ("res", "gelu_res")
    for seed in range(M * 7 + N + K, M * 7 + N + K + 64):
        g = torch.Generator().manual_seed(seed)
        if kind == "int":
            draw = lambda *s: torch.randint(-8, 9, s, generator=g).float()
            A, W, b, r = draw(M, K), draw(N, K), draw(N), draw(M, N)
        else:
            A, W, b, r = (torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / math.sqrt(K), torch.randn(N, generator=g),
                          torch.randn(M, N, generator=g))
        c = SimpleNamespace(M=M, N=N, K=K, epi=epi, act=act, A=A, W=W, bias=b if has_bias else None, R=r if has_res else None)
        c.ref = _reference(c, torch.int64 if kind == "int" else torch.float64)
        if kind != "int" or ((c.ref != 0).any(0).all() and (c.ref != 0).any(1).all()):
            return c
    raise AssertionError("no seed gives a reference without an all-zero row or column")


def test_integer_cases_are_exact_and_leave_no_zero_row_or_column():
    for (M, N, K, epi) in int_cases():
        assert 64 * K + 16 < 2 ** 24, (M, N, K)
        c = case(M, N, K, epi, "int")
        for t in (c.A, c.W, c.bias, c.R):
            assert t is None or (t.abs().max() <= 8 and torch.equal(t, t.round()))
        assert c.ref.dtype == torch.int64 and c.ref.abs().max() <= 64 * K + 16
        assert (c.ref != 0).any(0).all() and (c.ref != 0).any(1).all(), (M, N, K, epi)
        assert not (c.ref.double() == SENT).any()


def test_case_tables_reach_what_they_claim():
    """the dispatch of gemm_f32_fold, re-read: every DMA shape is DMA-eligible, every REG case is not (or is forced), and picks its block"""
    for (M, N, K) in DMA_SHAPES:
        assert K % 32 == 0 and N % 4 == 0 and N > 32
    assert {K // 32 for (_, _, K) in DMA_SHAPES} >= {1, 2, 3}                         # nk = 1: no ring; 2, 3: each ring's prologue
    assert {N % 128 for (_, N, _) in DMA_SHAPES} >= {0, 36, 100, 4, 64} and {N % 64 for (_, N, _) in DMA_SHAPES} >= {0, 36, 4}
    assert {M for (M, _, _) in DMA_SHAPES} >= {1, 127, 128, 129, 65, 257}
    for (name, M, N, K, epi, block, how) in REG:
        assert K % 4 == 0
        eligible = K % 32 == 0 and N % 4 == 0 and N > 32 and epi in EPIS and how in ("", "t10")
        assert not eligible or how == "t10", (name, M, N, K)
        mb = (M + 127) // 128
        want = "128, 32, 32, 32" if N <= 32 else "128, 128, 64, 64" if (N >= 128 and mb * ((N + 127) // 128) >= 512) else "64, 64, 32, 32"
        assert block == want, (name, M, N, K)
    assert {(K % 32 != 0) for (n, _, _, K, _, _, _) in REG if n == "block128"} == {True, False}


# ------------------------------------------------------------------------------------------------- the call
def _buf(dev, rows, ld, off, fill):
    """a [rows, ld] view `off` floats into a flat buffer that holds `fill` everywhere"""
    flat = torch.full((off + rows * ld,), fill, dtype=torch.float32, device=dev)
    return flat[off:].view(rows, ld)


def run(dev, c, *, M=None, lda=None, ldr=None, ldc=None, c_off=0, b_off=0, r_off=0, inplace=False, a_pad=float("nan"), r_pad=float("nan")):
    """avd_gemm_bias_act_f32 on the first M rows of the case, every operand in a padded buffer with two rows more than M.
    -> (C's whole [M + 2, ldc] buffer on the CPU, {profiler tag: launches})"""
    from multimodal_diffusion_amd import _lib as L
    M = c.M if M is None else M
    N, K = c.N, c.K
    lda, ldr, ldc = (K + 4 if lda is None else lda), (N + 8 if ldr is None else ldr), (N + 4 if ldc is None else ldc)
    A = _buf(dev, M + 2, lda, 0, a_pad)
    A[:M, :K] = c.A[:M].to(dev)
    W = c.W.to(dev)
    bias = None
    if c.bias is not None:
        bias = _buf(dev, 1, N, b_off, 0.0)
        bias[0] = c.bias.to(dev)
    Cb = _buf(dev, M + 2, ldc, c_off, SENT)
    Rb = None
    if c.R is not None:
        if inplace:
            Rb, ldr = Cb, ldc
        else:
            Rb = _buf(dev, M + 2, ldr, r_off, r_pad)
        Rb[:M, :N] = c.R[:M].to(dev)
    torch.cuda.synchronize()
    L.prof_enable(True)
    try:
        L.check(L.lib().avd_gemm_bias_act_f32(A.data_ptr(), lda, W.data_ptr(), L.ptr(bias), L.ptr(Rb), ldr, Cb.data_ptr(), ldc,
                                              M, N, K, c.act, L.stream_ptr(dev)))
        torch.cuda.synchronize()
    finally:
        L.prof_enable(False)
    return Cb.cpu(), {k: v[0] for k, v in L.prof_report().items() if v[0] > 0}


def check_padding(Cb, M, N):
    assert (Cb[:M, N:] == SENT).all() and (Cb[M:] == SENT).all(), "the kernel wrote outside C[:M, :N]"


def check_values(Cb, c, route, M=None):
    """bit-equal for an int64 reference, rel_err < TOL for an fp64 one"""
    M = c.M if M is None else M
    got, ref = Cb[:M, :c.N], c.ref[:M]
    if ref.dtype == torch.int64:
        assert torch.equal(got.double(), ref.double()), f"{int((got.double() != ref.double()).sum())} elements differ from the int64 reference"
        return
    err = rel_err(got, ref)
    _WORST[route] = max(_WORST.get(route, 0.0), err)
    print(f"[f32 gemm edges] {route} {c.M}x{c.N}x{c.K} err {err:.3e} (largest so far {_WORST[route]:.3e})")
    assert err < TOL, err


# ------------------------------------------------------------------------------------------------- A: the LDS-DMA kernel
@gpu
@pytest.mark.parametrize("shape", DMA_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("epi", EPIS)
@pytest.mark.parametrize("cfg", list(DMA_CONFIGS), ids=lambda c: f"tile{c[0]}-stages{c[1]}")
def test_dma_kernel(dev, cfg, epi, shape):
    """Every tile, ring depth and epilogue at every shape: values, strides, the memory around C, NaN in the padding of A and R."""
    c = case(*shape, epi, "randn" if epi == "gelu" else "int")
    with tuned(gemm_tile=cfg[0], gemm_stages=cfg[1]):
        Cb, tags = run(dev, c)
        assert tags == {dma_tag(cfg, epi): 1}, tags
        check_padding(Cb, c.M, c.N)
        check_values(Cb, c, "dma " + epi)
        if epi == "res":                # R and C the same buffer: composite.hip's gemm_f32(..., y, rd, y, rd, ...)
            Ci, tags = run(dev, c, inplace=True)
            assert tags == {dma_tag(cfg, epi): 1}, tags
            check_padding(Ci, c.M, c.N)
            assert torch.equal(Ci[:c.M, :c.N], Cb[:c.M, :c.N])
        # the padding of A and R is never read: other bytes there, same result
        Cz, _ = run(dev, c, a_pad=3.0, r_pad=-5.0)
        assert torch.equal(Cz, Cb)


@gpu
@pytest.mark.parametrize("epi", ["plain", "gelu", "res"])
@pytest.mark.parametrize("cfg", list(DMA_CONFIGS), ids=lambda c: f"tile{c[0]}-stages{c[1]}")
def test_dma_rows_do_not_depend_on_M(dev, cfg, epi):
    """An output element's arithmetic does not depend on M: rows [0, 37) of a run at M = 257 are the bits of a run at M = 37
    (randn operands, so a row that a clamp or a guard takes from a neighbour differs)."""
    c = case(257, 260, 160, epi, "randn")
    with tuned(gemm_tile=cfg[0], gemm_stages=cfg[1]):
        big, tags = run(dev, c)
        assert tags == {dma_tag(cfg, epi): 1}, tags
        small, tags = run(dev, c, M=37)
        assert tags == {dma_tag(cfg, epi): 1}, tags
    check_padding(big, 257, c.N)
    check_padding(small, 37, c.N)
    check_values(big, c, "dma " + epi + " (randn)")
    assert torch.equal(small[:37, :c.N], big[:37, :c.N])


# ------------------------------------------------------------------------------------------------- B: the register kernel
@gpu
@pytest.mark.parametrize("name,M,N,K,epi,block,how", REG, ids=[f"{r[0]}-{r[1]}x{r[2]}x{r[3]}-{r[4]}{'-' + r[6] if r[6] else ''}" for r in REG])
def test_reg_kernel(dev, name, M, N, K, epi, block, how):
    c = case(M, N, K, epi, "randn" if epi in ("silu", "gelu_res") else "int")
    kw = {"ldc": N} if how == "ldcN" else {"c_off": 1} if how == "c1" else {"b_off": 1} if how == "b1" else {"r_off": 1} if how == "r1" else {}
    with tuned(gemm_tile=10 if how == "t10" else -1):
        Cb, tags = run(dev, c, **kw)
    assert tags == {reg_tag(block, K): 1}, tags
    check_padding(Cb, M, N)
    check_values(Cb, c, "reg " + epi + (" block128" if name == "block128" else ""))
    if how == "t10":                    # the same operands on the LDS-DMA kernel the shape takes by default
        Cd, tags = run(dev, c)
        assert list(tags) == [dma_tag((2, 3), epi)], tags
        assert torch.equal(Cd, Cb)


@gpu
def test_reg_kernel_in_place(dev):
    """R aliased with C on the register kernel (ragged K, N % 4 != 0)"""
    for (M, N, K) in ((130, 96, 100), (65, 33, 64)):
        c = case(M, N, K, "res", "int")
        block = "64, 64, 32, 32"
        Ci, tags = run(dev, c, inplace=True)
        assert tags == {reg_tag(block, K): 1}, tags
        check_padding(Ci, M, N)
        check_values(Ci, c, "reg res")


# ------------------------------------------------------------------------------------------------- C: refusals
@gpu
def test_refusals(dev):
    """Host checks: nothing launches, each raises with the library's message (AVD_EINVAL -> ValueError, AVD_EUNSUPPORTED -> AvdError)."""
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    buf = lambda n: torch.zeros(n, device=dev)
    A, W, b, r = buf(64 * 80), buf(64 * 80), buf(64), buf(64 * 80)
    Cb = torch.full((64 * 80,), SENT, device=dev)
    st = L.stream_ptr(dev)

    def call(M=8, N=64, K=32, lda=None, ldr=None, ldc=None, act=NONE, a_off=0, w_off=0, res=False):
        L.check(lib.avd_gemm_bias_act_f32(A.data_ptr() + 4 * a_off, K if lda is None else lda, W.data_ptr() + 4 * w_off, b.data_ptr(),
                                          r.data_ptr() if res else None, N if ldr is None else ldr, Cb.data_ptr(), N if ldc is None else ldc,
                                          M, N, K, act, st))

    L.prof_enable(True)
    try:
        with pytest.raises(L.AvdError, match="K=34 must be a multiple of 4"):
            call(K=34, lda=36)
        with pytest.raises(L.AvdError, match="A row stride must be a multiple of 4 floats"):
            call(K=32, lda=34)
        with pytest.raises(L.AvdError, match="A/W must be 16-byte aligned"):
            call(a_off=1, lda=36)
        with pytest.raises(L.AvdError, match="A/W must be 16-byte aligned"):
            call(w_off=2)
        with pytest.raises(ValueError, match="leading dimension smaller than row length"):
            call(lda=28)
        with pytest.raises(ValueError, match="leading dimension smaller than row length"):
            call(ldc=60)
        with pytest.raises(ValueError, match="leading dimension smaller than row length"):
            call(ldr=60, res=True)
        call(ldr=0)                                                      # ldr is not looked at without a residual
        for act in (3, 4, 5, -1, 17):                                    # tanh, relu, leaky relu: other kernels' activations
            with pytest.raises(ValueError, match=f"bad act {act}"):
                call(act=act)
        with pytest.raises(ValueError, match="bad dims"):
            call(M=-1)
        torch.cuda.synchronize()
        Cb.fill_(SENT)
        torch.cuda.synchronize()
        n_before = sum(v[0] for v in L.prof_report().values())
        call(M=0)                                                        # success, nothing launched, nothing written
        torch.cuda.synchronize()
    finally:
        L.prof_enable(False)
    assert sum(v[0] for v in L.prof_report().values()) == n_before == 1      # the one call above that was legal
    assert (Cb == SENT).all()


# ------------------------------------------------------------------------------------------------- D: folded RMSNorm
FOLD_TAGS = {0: ("128, 128, 64, 64", "2, 2"), 1: ("128, 64, 64, 32", "2, 2"), 2: ("64, 64, 32, 32", "3, 3")}   # default stages, M <= 2048


@gpu
@pytest.mark.parametrize("d", [128, 256, 512])
@pytest.mark.parametrize("M", [1, 65, 300])
@pytest.mark.parametrize("tile", [0, 1, 2])
def test_rmsfold_pair(dev, tile, M, d):
    """test_gemm_rmsfold_epilogue_direct's construction at small M and at d = 128 / 256 / 512 (ss_in_cols 4 / 8 / 16) and the one-column
    table: a residual GEMM that emits ss_out, then the scale-carrying GELU GEMM that consumes it."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    hid = 2 * d
    g = torch.Generator().manual_seed(M + tile + d)
    a = torch.randn(M, d, generator=g)
    x0 = torch.randn(M, d, generator=g) * torch.exp(torch.randn(M, 1, generator=g))       # rows of very different norms
    x0[min(7, M - 1)] = 0.0                                                               # a zero residual row
    w0 = torch.randn(d, d, generator=g) / math.sqrt(d)
    b0 = torch.randn(d, generator=g) * 0.1
    scale = 1.0 + 0.1 * torch.randn(d, generator=g)
    w1 = torch.randn(hid, d, generator=g) / math.sqrt(d)
    b1 = torch.randn(hid, generator=g) * 0.1
    w1s = (w1 * scale[None, :]).to(dev)
    blk, nst = FOLD_TAGS[tile]
    with tuned(gemm_tile=tile):
        L.prof_enable(True)
        try:
            x1, ss = Fn.linear_rmsfold(a.to(dev), w0.to(dev), b0.to(dev), residual=x0.to(dev), want_ss=True)
            y, _ = Fn.linear_rmsfold(x1, w1s, b1.to(dev), act=L.ACT_GELU, ss_in=ss, eps=1e-6)
            ss1 = (x1 * x1).sum(-1, keepdim=True).contiguous()
            y1, _ = Fn.linear_rmsfold(x1, w1s, b1.to(dev), act=L.ACT_GELU, ss_in=ss1, eps=1e-6)
            torch.cuda.synchronize()
        finally:
            L.prof_enable(False)
    tags = {k: v[0] for k, v in L.prof_report().items() if v[0] > 0}
    assert tags == {f"gemm_f32_dma_kernel<{blk}, 2, {nst}>": 1, f"gemm_f32_dma_kernel<{blk}, 1, {nst}>": 2}, tags
    assert ss.shape == (M, d // 32)
    x1_ref = x0.double() + R.linear(a.double(), w0.double(), b0.double())
    chunks = x1.cpu().double().view(M, d // 32, 32).pow(2).sum(-1)
    h = R.rmsnorm(x1.cpu().double(), scale.double(), 1e-6)                                # on the device's own x1
    ref = R.gelu_erf(R.linear(h, w1.double(), b1.double()))
    errs = {"fold x1": (rel_err(x1.cpu(), x1_ref), 2e-5), "fold ss_out": (rel_err(ss.cpu(), chunks), 1e-5),
            "fold y": (rel_err(y.cpu(), ref), 2e-5), "fold y one-column": (rel_err(y1.cpu(), ref), 2e-5)}
    for k, (e, _) in errs.items():
        _WORST[k] = max(_WORST.get(k, 0.0), e)
        print(f"[f32 gemm edges] {k} M={M} d={d} tile {tile} err {e:.3e} (largest so far {_WORST[k]:.3e})")
    for k, (e, bound) in errs.items():
        assert e < bound, (k, e)


@gpu
def test_rmsfold_refusals(dev):
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    z = lambda *s: torch.zeros(*s, device=dev)
    msg = "RMSNorm folding needs the LDS-DMA path"
    with pytest.raises(L.AvdError, match=msg):
        Fn.linear_rmsfold(z(8, 64), z(192, 64), z(192), want_ss=True)                       # N % 128 != 0
    with pytest.raises(L.AvdError, match=msg):
        Fn.linear_rmsfold(z(8, 64), z(192, 64), z(192), ss_in=z(8, 2))
    with pytest.raises(L.AvdError, match=msg):
        Fn.linear_rmsfold(z(8, 36), z(128, 36), z(128), ss_in=z(8, 1))                      # K % 32 != 0 with ss_in
    with pytest.raises(L.AvdError, match=msg):
        Fn.linear_rmsfold(z(8, 36), z(128, 36), z(128), want_ss=True)
