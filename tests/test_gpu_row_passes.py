"""GPU tests of the one-wave-per-row normalisation passes, called directly, against fp64 (oracle.ref_cpu on the fp32 inputs).

A. rmsnorm_kernel<NV> and layernorm_act_kernel<NV> (csrc/rowops.hip) at every tier, full and ragged, with every activation;
B. the four-rows-per-block edge: rows 1, 3, 4, 5 written into a larger prefilled buffer, bit-identical to the rows of a 37-row run;
C. the in-place call y == x the kernels' comments promise (core_forward makes it for the final norm);
D. exact and degenerate rows: constant rows through the LayerNorm, all-zero and 1e-7-scaled rows through the RMSNorm;
E. the four operand-image producers rmsnorm_split3_kernel<NC, F16> and layernorm_act_split3_kernel<NC, F16, GELU>
   (csrc/gemm_bf16x3.hip) at every NC, full and ragged, with the image bytes they must leave alone;
F. the f16x2 images' default scales at the input that reaches their bound;
G. the refusals the host makes before a launch.

Which instantiation a case runs rests on reading the dispatch, not on the profiler.
  fp32 kernels: nv_for(d) = ceil(d / 256) (rowops.hip).  WIDTHS gives
      NV 1: 4, 68, 256   NV 2: 260, 512   NV 3: 516, 768   NV 4: 772, 1024   NV 5: 1028, 1280   NV 6: 1284, 1536
      NV 7: 1540, 1792   NV 8: 1796, 2044, 2048
  so every tier runs with its last tier full (a multiple of 256) and ragged (4 columns into it: one lane of 64 holds data; 2044: one
  lane idle).  test_every_tier_and_activation runs each of them through rmsnorm_kernel<NV> and, once per activation, through
  layernorm_act_kernel<NV> (the activation is a runtime argument).  512, 516, 768, 1024 and 1536 are in the list because without them no
  width falls in tier 3 and tiers 2, 4 and 6 never run full.
  image producers: switch ((d + 511) / 512) (gemm_bf16x3.hip).  IMAGE_WIDTHS gives
      NC 1: 16, 272, 512   NC 2: 528, 768, 1024   NC 3: 1040, 1536   NC 4: 1552, 2032, 2048
  F16 is h2_scale > 0 (the two ..._f16x2 entry points), GELU is act == AVD_ACT_GELU.  test_image_producers runs, at each width,
  rmsnorm_split3_kernel<NC, false> and <NC, true>, and layernorm_act_split3_kernel<NC, false / true, true> (GELU) and
  <NC, false / true, false> (LEAKY_RELU and NONE, the runtime-`act` route): all 8 + 16 instantiations.

Bounds.  REL_RMS = 1e-6 and REL_LN = 2e-6 by conftest.rel_err are test_rmsnorm_and_layernorm_widths' (test_gpu_parity.py).  rel_err
divides the tensor's largest error by the tensor's largest value, so one wrong row next to ordinary ones passes; row_err divides each
row's largest error by that row's largest reference value, with no floor, and takes the worst row.  Its bound is measured: on the
MI355X against fp64, at WIDTHS x 37 rows, next to the same metric of the oracle's own fp32 evaluation on the CPU (the yardstick:
R.rmsnorm / R.layernorm on the fp32 tensors, then the activation in fp32):

      row_err, worst over WIDTHS        kernel (MI355X)     oracle in fp32 (CPU)
      RMSNorm                           1.9e-7              1.9e-7
      LayerNorm, NONE                   2.0e-7              2.7e-7
      LayerNorm, GELU                   3.6e-7              6.8e-7
      LayerNorm, SILU                   3.7e-7              5.4e-7
      LayerNorm, RELU                   2.7e-7              6.6e-7
      LayerNorm, LEAKY_RELU             2.7e-7              6.6e-7

(the worst width is d = 4 for every LayerNorm figure, where a row's largest value can be small; from d = 68 up the kernel stays below
2.5e-7).  Over the image producers' cases (IMAGE_WIDTHS x {5, 300} rows) the three bf16 planes' sum measures 2.1e-7 (RMSNorm) and
2.9e-7 (LayerNorm, GELU); the 1e-7-scaled row of test_rmsnorm_zero_and_tiny_rows 8.4e-8 (fp32 kernel) and 1.0e-7 (image).  Every kernel
figure is below half of the project's constant for its operation (5e-7 of 1e-6, 1e-6 of 2e-6), so the per-row bounds are those constants:
ROW_RMS = 1e-6, ROW_LN = 2e-6.  The f16x2 images use at most 0.22 of their bound (below).

The f16x2 images add their own resolution to that bound, 2^-22 |ref| + 2^-25 / s per element (test_split_f16x2_image, test_gpu_f16x2.py).
The bf16x3 images add nothing: three bf16 planes hold an fp32 value exactly."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from _attn_kit import h2_decode, split3_decode
from _kit import dev  # noqa: F401  (fixture)
from conftest import rel_err
from oracle import ref_cpu as R

pytestmark = pytest.mark.gpu

WIDTHS = [4, 68, 256, 260, 512, 516, 768, 772, 1024, 1028, 1280, 1284, 1536, 1540, 1792, 1796, 2044, 2048]
IMAGE_WIDTHS = [16, 272, 512, 528, 768, 1024, 1040, 1536, 1552, 2032, 2048]
ACTS = ["NONE", "GELU", "SILU", "RELU", "LEAKY_RELU"]
IMAGE_ACTS = ["GELU", "LEAKY_RELU", "NONE"]          # the GELU = true template, then the runtime-`act` route twice

REL_RMS, REL_LN = 1e-6, 2e-6        # conftest.rel_err: test_rmsnorm_and_layernorm_widths
ROW_RMS, ROW_LN = 1e-6, 2e-6        # row_err: see the module docstring
RMS_EPS, LN_EPS = 1e-6, 1e-5        # the wrappers' and the oracle's defaults


# ------------------------------------------------------------------------------------------------- references and metrics
def act_ref(name, t):
    """the activation of a LayerNorm + act pass in the precision of t (SILU: x * sigmoid(x); LEAKY_RELU: slope 0.1)"""
    if name == "NONE":
        return t
    if name == "GELU":
        return R.gelu_erf(t)
    if name == "SILU":
        return t * torch.sigmoid(t)
    if name == "RELU":
        return t.clamp(min=0)
    assert name == "LEAKY_RELU", name
    return torch.where(t > 0, t, 0.1 * t)


def act_id(name):
    from multimodal_diffusion_amd import _lib as L
    return getattr(L, "ACT_" + name)


def row_err(y, ref):
    """max over rows of (max |y - ref| over the row / max |ref| over the row); no floor"""
    y = torch.as_tensor(y, dtype=torch.float64)
    ref = torch.as_tensor(ref, dtype=torch.float64)
    return float(((y - ref).abs().amax(-1) / ref.abs().amax(-1)).max())


@lru_cache(maxsize=None)
def inputs(rows, d):
    """(x, gain, bias) in the style of test_rmsnorm_and_layernorm_widths, seeded from the shape; shared and never modified"""
    g = torch.Generator().manual_seed(4099 * rows + d)
    return torch.randn(rows, d, generator=g) * 3 + 0.5, torch.randn(d, generator=g), torch.randn(d, generator=g)


@lru_cache(maxsize=None)
def rms_ref(rows, d):
    x, s, _ = inputs(rows, d)
    return R.rmsnorm(x.double(), s.double(), RMS_EPS)


@lru_cache(maxsize=None)
def ln_ref(rows, d, act):
    x, s, b = inputs(rows, d)
    return act_ref(act, R.layernorm(x.double(), s.double(), b.double(), LN_EPS))


def check(y, ref, rel, row, what):
    e, er = rel_err(y, ref), row_err(y, ref)
    print(f"ROWPASS {what}: rel_err {e:.3e} row_err {er:.3e}")
    assert e < rel, (what, e)
    assert er < row, (what, er)


def on(dev, *ts):
    return tuple(t.to(dev) for t in ts)


# ------------------------------------------------------------------------------------------------- A. tiers and activations
@pytest.mark.parametrize("d", WIDTHS)
def test_every_tier_and_activation(dev, d):
    """rmsnorm_kernel<NV> and layernorm_act_kernel<NV> at NV = ceil(d / 256) with the last tier full or ragged, every activation, in
    both metrics (bounds and measurements in the module docstring)."""
    from multimodal_diffusion_amd import functional as Fn
    x, s, b = on(dev, *inputs(37, d))
    check(Fn.rmsnorm(x, s).cpu(), rms_ref(37, d), REL_RMS, ROW_RMS, f"rmsnorm d={d}")
    for act in ACTS:
        y = Fn.layernorm_act(x, s, b, act=act_id(act)).cpu()
        check(y, ln_ref(37, d, act), REL_LN, ROW_LN, f"layernorm {act} d={d}")


# ------------------------------------------------------------------------------------------------- B. row edges
@pytest.mark.parametrize("d", [260, 2048])
@pytest.mark.parametrize("rows", [1, 3, 4, 5])
def test_row_edges(dev, rows, d):
    """A block holds four rows and a row is one wave's work: the first `rows` rows of a 37-row input come out bit-identical to the 37-row
    run's whatever the grid's edge, and nothing is written past them (the buffer holds rows + 3 rows of 7.0)."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    lib, st = L.lib(), L.stream_ptr(dev)
    x, s, b = on(dev, *inputs(37, d))
    out = torch.full((rows + 3, d), 7.0, device=dev)
    L.check(lib.avd_rmsnorm_f32(x.data_ptr(), s.data_ptr(), out.data_ptr(), rows, d, RMS_EPS, st))
    assert torch.equal(out[:rows], Fn.rmsnorm(x, s)[:rows])
    assert bool((out[rows:] == 7.0).all())
    for act in ACTS:
        out = torch.full((rows + 3, d), 7.0, device=dev)
        L.check(lib.avd_layernorm_act_f32(x.data_ptr(), s.data_ptr(), b.data_ptr(), out.data_ptr(), rows, d, LN_EPS, act_id(act), st))
        assert torch.equal(out[:rows], Fn.layernorm_act(x, s, b, act=act_id(act))[:rows]), act
        assert bool((out[rows:] == 7.0).all()), act


# ------------------------------------------------------------------------------------------------- C. in place
@pytest.mark.parametrize("d", [260, 1028, 2048])
def test_in_place(dev, d):
    """y == x: a wave holds its whole row in registers before it stores, so the in-place result is the out-of-place one bit for bit"""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    lib, st = L.lib(), L.stream_ptr(dev)
    x, s, b = on(dev, *inputs(5, d))
    y = x.clone()
    L.check(lib.avd_rmsnorm_f32(y.data_ptr(), s.data_ptr(), y.data_ptr(), 5, d, RMS_EPS, st))
    assert torch.equal(y, Fn.rmsnorm(x, s))
    for act in ("NONE", "GELU"):
        y = x.clone()
        L.check(lib.avd_layernorm_act_f32(y.data_ptr(), s.data_ptr(), b.data_ptr(), y.data_ptr(), 5, d, LN_EPS, act_id(act), st))
        assert torch.equal(y, Fn.layernorm_act(x, s, b, act=act_id(act))), act


# ------------------------------------------------------------------------------------------------- D. exact and degenerate rows
@pytest.mark.parametrize("d", [260, 512, 1028])
def test_layernorm_constant_rows(dev, d):
    """Rows of 0.5: the lanes' partial sums, their butterfly sum 0.5 d and the mean 0.5 are exact in fp32, every centred value is exactly
    0 and the normalised value is beta whatever rstd is.  NONE, RELU and LEAKY_RELU are then exact operations on beta: bit for bit.  GELU
    and SILU round: within the per-row bound of act(beta) in fp64.  At d % 16 == 0 the bf16x3 image producer must give the same sums."""
    from multimodal_diffusion_amd import functional as Fn
    _, s, b = inputs(5, d)
    x = torch.full((5, d), 0.5)
    assert torch.equal(R.layernorm(x.double(), s.double(), b.double(), LN_EPS), b.double().expand(5, d))      # the fp64 reference is beta
    xd, sd, bd = on(dev, x, s, b)
    for act in ACTS:
        y = Fn.layernorm_act(xd, sd, bd, act=act_id(act)).cpu()
        if act in ("GELU", "SILU"):
            assert row_err(y, act_ref(act, b.double()).expand(5, d)) < ROW_LN, act
        else:
            assert torch.equal(y, act_ref(act, b).expand(5, d)), act
        if d % 16 == 0:
            img = Fn.layernorm_act_split3(xd, sd, bd, act=act_id(act)).cpu().numpy()
            assert np.array_equal(split3_decode(img, 5, d).astype(np.float64).sum(0), y.double().numpy()), act


@pytest.mark.parametrize("d", [260, 2044])
def test_rmsnorm_zero_and_tiny_rows(dev, d):
    """An all-zero row gives an all-zero row (0 / eps).  A row scaled by 1e-7 has an rms near 3e-7, below eps = 1e-6 outside the square
    root: its output is small against its neighbours', so only the per-row metric sees it, and it must hold the same bound."""
    from multimodal_diffusion_amd import functional as Fn
    x, s, _ = inputs(5, d)
    x = x.clone()
    x[1] = 0.0
    x[3] *= 1e-7
    ref = R.rmsnorm(x.double(), s.double(), RMS_EPS)
    assert 0.1 < float(ref[3].abs().max() / ref[0].abs().max()) < 0.5          # eps matters in row 3 and the row is not lost
    y = Fn.rmsnorm(*on(dev, x, s)).cpu()
    assert bool((y[1] == 0).all())
    keep = [0, 2, 3, 4]
    check(y[keep], ref[keep], REL_RMS, ROW_RMS, f"rmsnorm tiny row d={d}")
    # the image producers take d % 16 == 0 only: the same rows cut to the next such width below (256, 2032)
    d16 = d // 16 * 16
    x16, s16 = x[:, :d16].contiguous(), s[:d16].contiguous()
    ref = R.rmsnorm(x16.double(), s16.double(), RMS_EPS)
    y = split3_decode(Fn.rmsnorm_split3(*on(dev, x16, s16)).cpu().numpy(), 5, d16).astype(np.float64).sum(0)
    assert (y[1] == 0).all()
    check(y[keep], ref[keep], REL_RMS, ROW_RMS, f"rmsnorm_split3 tiny row d={d16}")


# ------------------------------------------------------------------------------------------------- E. image producers
def pattern(nbytes, dev):
    """a byte pattern of period 251 (no power of two): a store that lands in the wrong place changes it"""
    return (torch.arange(nbytes, device=dev) * 37 + 11).remainder(251).to(torch.uint8)


def image_parts(img, rows, d):
    """(image as [row tile, k / 16, plane, row in tile, 32 B], mask of the image rows >= `rows`): the geometry include/avdiff_hip.h
    and csrc/gemm_bf16x3.hip document, T[ceil(rows / 128)][K / 16][3 planes][128 rows][32 B]"""
    tiles = img.numel() // (d // 16 * 3 * 128 * 32)
    assert tiles * (d // 16) * 3 * 128 * 32 == img.numel() and tiles * 128 >= rows
    a = img.view(tiles, d // 16, 3, 128, 32)
    r = torch.arange(tiles, device=img.device)[:, None] * 128 + torch.arange(128, device=img.device)[None, :]
    return a, (r >= rows)[:, None, None, :, None].expand_as(a)


def check_untouched(run, fn_img, rows, d, planes, dev, what):
    """`run(image)` is the direct library call of the producer whose wrapper returned `fn_img`.  Into a patterned image it must leave
    every byte of the image rows >= rows, and of the planes >= `planes`, as it was; the bytes it does write are the wrapper's."""
    from multimodal_diffusion_amd import _lib as L
    img = pattern(fn_img.numel(), dev)
    before = img.clone()
    L.check(run(img))
    a, past = image_parts(img, rows, d)
    p, _ = image_parts(before, rows, d)
    f, _ = image_parts(fn_img, rows, d)
    assert torch.equal(a[past], p[past]), what + ": image rows past the last row were written"
    assert torch.equal(a[:, :, planes:], p[:, :, planes:]), what + ": an unused plane was written"
    assert torch.equal(a[:, :, :planes][~past[:, :, :planes]], f[:, :, :planes][~past[:, :, :planes]]), what


def check_bf16x3(img, rows, d, ref, y32, rel, row, what):
    """the three planes sum (exactly, in fp64) to a value within the fp32 kernels' bounds of the fp64 reference, and within 1e-6 by
    rel_err of the fp32 kernel's output (test_rmsnorm_split3's second check)"""
    y = torch.from_numpy(split3_decode(img.cpu().numpy(), rows, d).astype(np.float64).sum(0))
    check(y, ref, rel, row, what)
    assert rel_err(y, y32.cpu()) < 1e-6, what


def check_f16x2(img, s, rows, d, ref, row, what):
    """(h + l) / s within the per-row bound plus the image's resolution 2^-22 |ref| + 2^-25 / s of the fp64 reference, element by element
    (this implies the rel_err form of the bound, whose divisor is at least the row's); every plane value finite, |h| <= 2^15"""
    pl = h2_decode(img.cpu().numpy(), rows, d)
    assert np.isfinite(pl).all() and np.abs(pl[0]).max() <= 2.0 ** 15, what
    refn = ref.numpy()
    err = np.abs(pl.sum(0) / s - refn)
    lim = row * np.abs(refn).max(-1, keepdims=True) + 2.0 ** -22 * np.abs(refn) + 2.0 ** -25 / s
    print(f"ROWPASS {what}: worst err / bound {float((err / lim).max()):.3f} scale {s}")
    assert (err <= lim).all(), (what, float((err / lim).max()))


@pytest.mark.parametrize("rows", [5, 300])
@pytest.mark.parametrize("d", IMAGE_WIDTHS)
def test_image_producers(dev, d, rows):
    """The four producers at NC = ceil(d / 512) with the last chunk full or ragged (module docstring), against fp64 and against the fp32
    kernels, and the bytes they must not write: every kernel returns at `row >= rows` before its first store and the f16x2 stores go to
    planes 0 and 1 only (store_split8_h2, avd_common.h), so image rows past `rows` and an f16x2 image's third plane keep their bytes."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    lib, st = L.lib(), L.stream_ptr(dev)
    x, s, b = on(dev, *inputs(rows, d))
    xp, sp, bp = x.data_ptr(), s.data_ptr(), b.data_ptr()

    ref, what = rms_ref(rows, d), f"rmsnorm_split3 d={d} rows={rows}"
    img = Fn.rmsnorm_split3(x, s)
    check_bf16x3(img, rows, d, ref, Fn.rmsnorm(x, s), REL_RMS, ROW_RMS, what)
    check_untouched(lambda o: lib.avd_rmsnorm_split3_f32(xp, sp, o.data_ptr(), rows, d, RMS_EPS, st), img, rows, d, 3, dev, what)
    what = f"rmsnorm_split_f16x2 d={d} rows={rows}"
    img, sc = Fn.rmsnorm_split_f16x2(x, s)
    check_f16x2(img, sc, rows, d, ref, ROW_RMS, what)
    check_untouched(lambda o: lib.avd_rmsnorm_split_f16x2_f32(xp, sp, o.data_ptr(), rows, d, RMS_EPS, sc, st), img, rows, d, 2, dev, what)

    for act in IMAGE_ACTS:
        a = act_id(act)
        ref, what = ln_ref(rows, d, act), f"layernorm_act_split3 {act} d={d} rows={rows}"
        img = Fn.layernorm_act_split3(x, s, b, act=a)
        check_bf16x3(img, rows, d, ref, Fn.layernorm_act(x, s, b, act=a), REL_LN, ROW_LN, what)
        check_untouched(lambda o: lib.avd_layernorm_act_split3_f32(xp, sp, bp, o.data_ptr(), rows, d, LN_EPS, a, st), img, rows, d, 3,
                        dev, what)
        what = f"layernorm_act_split_f16x2 {act} d={d} rows={rows}"
        img, sc = Fn.layernorm_act_split_f16x2(x, s, b, act=a)
        check_f16x2(img, sc, rows, d, ref, ROW_LN, what)
        check_untouched(lambda o: lib.avd_layernorm_act_split_f16x2_f32(xp, sp, bp, o.data_ptr(), rows, d, LN_EPS, a, sc, st), img, rows,
                        d, 2, dev, what)


# ------------------------------------------------------------------------------------------------- F. the scale rule at its bound
def peaked(d, sign):
    """(x, gain, bias, k): five rows of which row 2 holds 1e4 * sign in column k and zeros elsewhere; |gain| and |bias| are largest in
    column k (1.9 and 1.5 against at most 1.5 and 1.0).  sign +1: the large element, gain_k and bias_k are all positive, so the LayerNorm's
    two terms add.  sign -1: the large element and bias_k are negative and gain_k stays positive, so they add at the negative end (with
    all three negative, gain_k times the normalised element would be positive again and bias_k would cancel against it)."""
    x, s, b = inputs(5, d)
    x, s, b = x.clone(), s.clamp(-1.5, 1.5), b.clamp(-1.0, 1.0)
    k = (3 * d) // 7
    x[2] = 0.0
    x[2, k] = 1e4 * sign
    s[k], b[k] = 1.9, 1.5 * sign
    return x, s, b, k


@pytest.mark.parametrize("sign", [1.0, -1.0])
@pytest.mark.parametrize("d", [512, 1040, 2048])
def test_f16x2_scale_rule_at_its_bound(dev, d, sign):
    """The default scales come from |y_i| <= sqrt(d) max|gamma| (RMSNorm) and sqrt(d) max|gamma| + max|beta| (LayerNorm, the head's rule
    in noise_heads.py::_f16x2_scales).  A one-hot row reaches the first (gamma_k sqrt(d) to rounding) and approaches the second
    (sqrt(d - 1) gamma_k + beta_k, the two terms adding because the signs agree).  The case is at the bound when the scaled value lies in
    the top binade the rule allows, (2^14, 2^15]: a scale with one bit less headroom would then overflow |h| <= 2^15."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    x, s, b, k = peaked(d, sign)
    xd, sd, bd = on(dev, x, s, b)

    ref = R.rmsnorm(x.double(), s.double(), RMS_EPS)
    assert abs(float(ref[2, k]) * sign / (1.9 * d ** 0.5) - 1.0) < 1e-6
    img, sc = Fn.rmsnorm_split_f16x2(xd, sd)
    assert 2.0 ** 14 < sc * float(ref.abs().max()) <= 2.0 ** 15
    check_f16x2(img, sc, 5, d, ref, ROW_RMS, f"rmsnorm_split_f16x2 one-hot d={d} sign={sign:+.0f}")

    ref = R.layernorm(x.double(), s.double(), b.double(), LN_EPS)
    assert abs(float(ref[2, k]) * sign / (1.9 * (d - 1) ** 0.5 + 1.5) - 1.0) < 1e-6
    img, sc = Fn.layernorm_act_split_f16x2(xd, sd, bd, act=L.ACT_NONE)
    assert 2.0 ** 14 < sc * float(ref.abs().max()) <= 2.0 ** 15
    check_f16x2(img, sc, 5, d, ref, ROW_LN, f"layernorm_act_split_f16x2 one-hot d={d} sign={sign:+.0f}")


# ------------------------------------------------------------------------------------------------- G. refusals on the host
def refused(rc, out, before):
    """a non-zero return code, and the output as it was: nothing ran"""
    torch.cuda.synchronize()
    return rc != 0 and torch.equal(out, before)


@pytest.mark.parametrize("d", [66, 2052])
def test_fp32_kernels_refuse_widths(dev, d):
    """d % 4 != 0 and d > 2048: both entry points check the width (AVD_REQUIRE in rmsnorm_f32 / layernorm_act_f32, rowops.hip) before
    the `rows == 0` return and the launch"""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    lib, st = L.lib(), L.stream_ptr(dev)
    x, s, b = torch.ones(4, d, device=dev), torch.ones(d, device=dev), torch.ones(d, device=dev)
    with pytest.raises(L.AvdError):
        Fn.rmsnorm(x, s)
    with pytest.raises(L.AvdError):
        Fn.layernorm_act(x, s, b)
    out = torch.full((4, d), 7.0, device=dev)
    before = out.clone()
    assert refused(lib.avd_rmsnorm_f32(x.data_ptr(), s.data_ptr(), out.data_ptr(), 4, d, RMS_EPS, st), out, before)
    assert refused(lib.avd_layernorm_act_f32(x.data_ptr(), s.data_ptr(), b.data_ptr(), out.data_ptr(), 4, d, LN_EPS, 0, st), out, before)


@pytest.mark.parametrize("d,scale", [(24, None), (2064, None), (512, 0.0), (512, -4.0)])
def test_image_producers_refuse(dev, d, scale):
    """d % 16 != 0 and d > 2048 (AVD_REQUIRE at the top of rmsnorm_split3_f32 / layernorm_act_split3_f32, gemm_bf16x3.hip) on all four
    producers, a zero or negative scale on the two f16x2 ones (the first line of their extern "C" entries): every refusal precedes the
    launch macro in its function.  The wrappers raise AvdError; the library returns an error code and writes nothing."""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    lib, st = L.lib(), L.stream_ptr(dev)
    x, s, b = torch.ones(4, d, device=dev), torch.ones(d, device=dev), torch.ones(d, device=dev)
    xp, sp, bp = x.data_ptr(), s.data_ptr(), b.data_ptr()
    out = pattern(256 * 2064 * 6, dev)
    before, o = out.clone(), out.data_ptr()
    if scale is None:
        with pytest.raises(L.AvdError):
            Fn.rmsnorm_split3(x, s)
        with pytest.raises(L.AvdError):
            Fn.layernorm_act_split3(x, s, b)
        assert refused(lib.avd_rmsnorm_split3_f32(xp, sp, o, 4, d, RMS_EPS, st), out, before)
        assert refused(lib.avd_layernorm_act_split3_f32(xp, sp, bp, o, 4, d, LN_EPS, L.ACT_GELU, st), out, before)
    with pytest.raises(L.AvdError):
        Fn.rmsnorm_split_f16x2(x, s, scale=scale)
    with pytest.raises(L.AvdError):
        Fn.layernorm_act_split_f16x2(x, s, b, scale=scale)
    sc = 64.0 if scale is None else scale
    assert refused(lib.avd_rmsnorm_split_f16x2_f32(xp, sp, o, 4, d, RMS_EPS, sc, st), out, before)
    assert refused(lib.avd_layernorm_act_split_f16x2_f32(xp, sp, bp, o, 4, d, LN_EPS, L.ACT_GELU, sc, st), out, before)
