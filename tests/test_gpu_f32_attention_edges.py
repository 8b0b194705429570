"""The fp32 attention (csrc/attn_f32.hip: avd_attn_fwd_f32, avd_attn_fwd_split3_f32) under a key_padding_mask on both of its kernels,
with fewer queries than keys, and with its split3-image output on the 4-wave kernel.

attn_launch runs attn_f32_kernel<4> exactly when ceil(n_query / 64) is even and attn_f32_kernel<2> otherwise; which one ran is
asserted from the profiler tags it registers.  SHAPES, as (N, n_query):
      (43, 43)      2-wave, one ragged tile          (64, 64)      2-wave, no tail          (128, 128)   4-wave, no tail
      (133, 133)    2-wave, three tiles              (200, 200)    4-wave                   (257, 257)   2-wave, a one-key tail
      (200, 40), (200, 130)   2-wave with fewer queries than keys        (200, 100)   4-wave with fewer queries than keys
One call holds one sample per mask of MASKS that applies to N (all eight for N > 64), H = 2 heads with different operands.

Bounds.  conftest.rel_err < 2e-5 against masked softmax in fp64 (-inf on the masked keys, as oracle.ref_cpu.self_attention), the
bound of test_attention and test_attention_key_padding_mask.  Where one key is visible its weight is exactly 1 (exp2(0) = 1, every
other exp2 is 0, 1 / l = 1), so every query row must equal that key's v row bit for bit.  A sample whose keys are all masked attends
uniformly (include/avdiff_hip.h): each row is the mean of the sample's v over its N keys, same 2e-5.

Largest rel_err measured on the MI355X (printed by the tests as they run; bounds are not taken from these):
      masked softmax, attn_f32_kernel<2>    2.4e-7          masked softmax, attn_f32_kernel<4>    1.5e-7
      all keys masked, against the mean     8.5e-8
Before the filler keys of a ragged last tile got a score below the masked keys' (ATT_PAD < ATT_NEG), an all-masked sample gave
(sum_j v_j + pad * v_{N-1}) / (N + pad), pad = 64 ceil(N / 64) - N.  Measured on these operands with the kernel as it was: rel_err
1.03 at N = 43, 0.85 at N = 133, 0.53 at N = 200 against the mean (and below 5e-7 against that formula); 8.4e-8 and 7.4e-8 at
N = 64 and 128, where there is no filler."""
from functools import lru_cache

import numpy as np
import pytest
import torch

from _attn_kit import split3_decode
from _kit import dev  # noqa: F401  (fixture)
from conftest import rel_err

gpu = pytest.mark.gpu

H, D = 2, 128
TOL = 2e-5                            # test_attention, test_attention_key_padding_mask
SHAPES = [(43, 43), (64, 64), (128, 128), (133, 133), (200, 200), (257, 257), (200, 40), (200, 130), (200, 100)]
SPLIT_SHAPES = [(128, 128), (200, 200), (200, 130), (200, 100)]
ALL_MASKED_N = [64, 128, 43, 133, 200]
MASKS = ["none", "first_tile", "last_tile", "only_key_0", "only_last_key", "only_key_64", "every_other", "random_45"]
SINGLE = {"only_key_0": lambda N: 0, "only_last_key": lambda N: N - 1, "only_key_64": lambda N: 64}
_WORST = {}


def last_tile_start(N):
    return 64 * ((N - 1) // 64)


def mask(name, N):
    """[N] bool, True = this key is padding"""
    m = torch.zeros(N, dtype=torch.bool)
    if name == "first_tile":
        m[:64] = True
    elif name == "last_tile":
        m[last_tile_start(N):] = True
    elif name in SINGLE:
        m[:] = True
        m[SINGLE[name](N)] = False
    elif name == "every_other":
        m[1::2] = True
    elif name == "random_45":
        m[torch.randperm(N, generator=torch.Generator().manual_seed(45 + N))[:round(0.45 * N)]] = True
    else:
        assert name == "none", name
    return m


def visible(name, N):
    """the number of keys the mask leaves"""
    return {"none": N, "first_tile": N - 64, "last_tile": last_tile_start(N), "every_other": (N + 1) // 2,
            "random_45": N - round(0.45 * N)}.get(name, 1)


def masks_for(N):
    return [m for m in MASKS if N > 64 or m not in ("first_tile", "last_tile", "only_key_64")]


def kernel_tag(n_query, split=False):
    nw = 4 if ((n_query + 63) // 64) % 2 == 0 else 2
    return f"attn_f32_kernel<{nw}, true>" if split else f"attn_f32_kernel<{nw}>"


def test_masks_leave_what_they_advertise():
    for N in sorted({n for n, _ in SHAPES} | set(ALL_MASKED_N)):
        names = masks_for(N)
        assert len(names) == (8 if N > 64 else 5)
        for name in names:
            m = mask(name, N)
            assert int((~m).sum()) == visible(name, N) >= 1, (name, N)
        if N > 64:
            first, last = mask("first_tile", N), mask("last_tile", N)
            assert first[:64].all() and not first[64:].any()
            s = last_tile_start(N)
            assert s % 64 == 0 and 0 < N - s <= 64 and last[s:].all() and not last[:s].any()
            assert not mask("only_key_64", N)[64] and mask("only_key_64", N).sum() == N - 1
        assert not mask("only_key_0", N)[0] and not mask("only_last_key", N)[N - 1]


def test_shapes_reach_both_kernels():
    tags = {(nq == N, N % 64 != 0, kernel_tag(nq)) for N, nq in SHAPES}
    for full in (True, False):
        assert {t for f, _, t in tags if f == full} == {"attn_f32_kernel<2>", "attn_f32_kernel<4>"}
    assert {r for _, r, _ in tags} == {True, False}
    assert [kernel_tag(nq) for N, nq in SHAPES] == [f"attn_f32_kernel<{w}>" for w in (2, 2, 4, 2, 4, 2, 2, 2, 4)]
    assert {kernel_tag(nq, True) for _, nq in SPLIT_SHAPES} == {"attn_f32_kernel<2, true>", "attn_f32_kernel<4, true>"}


# ------------------------------------------------------------------------------------------------- operands, reference, the call
@lru_cache(maxsize=None)
def operands(B, N):
    """qkv [B, N, 3 D] on the CPU, seeded from the shape; shared and never modified"""
    return torch.randn(B, N, 3 * D, generator=torch.Generator().manual_seed(1000 * B + N))


@lru_cache(maxsize=None)
def masked_case(N):
    """(qkv, kpm [B, N], fp64 reference [B, N, D]): one sample per mask that applies to N"""
    names = masks_for(N)
    B = len(names)
    qkv = operands(B, N)
    kpm = torch.stack([mask(n, N) for n in names])
    q, k, v = (qkv.double().view(B, N, 3, H, 64)[:, :, i].transpose(1, 2) for i in range(3))
    s = (q @ k.transpose(-1, -2) / 8.0).masked_fill(kpm[:, None, None, :], float("-inf"))
    return qkv, kpm, (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(B, N, D)


def attend(dev, qkv, kpm, n_query, fill=None, expect=None):
    """avd_attn_fwd_f32 into a buffer prefilled with `fill` -> the [B, N, D] output on the CPU; asserts the kernel that ran"""
    from multimodal_diffusion_amd import _lib as L
    B, N, _ = qkv.shape
    q = qkv.to(dev)
    m = None if kpm is None else kpm.to(dev).to(torch.uint8).contiguous()
    out = torch.empty(B, N, D, device=dev) if fill is None else torch.full((B, N, D), fill, device=dev)
    torch.cuda.synchronize()
    L.prof_enable(True)
    try:
        L.check(L.lib().avd_attn_fwd_f32(q.data_ptr(), out.data_ptr(), B, N, H, 64, 0.125, n_query, L.ptr(m), L.stream_ptr(dev)))
        torch.cuda.synchronize()
    finally:
        L.prof_enable(False)
    tags = {k: v[0] for k, v in L.prof_report().items() if v[0] > 0}
    assert tags == {kernel_tag(n_query) if expect is None else expect: 1}, tags
    return out.cpu()


def record(route, err):
    _WORST[route] = max(_WORST.get(route, 0.0), err)
    print(f"[f32 attention edges] {route} err {err:.3e} (largest so far {_WORST[route]:.3e})")


# ------------------------------------------------------------------------------------------------- masks on both kernels
@gpu
@pytest.mark.parametrize("N,nq", SHAPES, ids=[f"N{n}-q{q}" for n, q in SHAPES])
def test_masked_attention(dev, N, nq):
    qkv, kpm, ref = masked_case(N)
    names = masks_for(N)
    full = attend(dev, qkv, kpm, N)
    err = rel_err(full, ref)
    record(f"masked {kernel_tag(N)}", err)
    assert err < TOL, err
    # no key masked: the bits of the call without a mask
    assert torch.equal(full[names.index("none")], attend(dev, qkv, None, N)[names.index("none")])
    # one visible key: its v row, exactly, in every query row and head
    for name, key in SINGLE.items():
        if name in names:
            b = names.index(name)
            assert torch.equal(full[b], qkv[b, key(N), 2 * D:].expand(N, D)), name
    if nq < N:
        part = attend(dev, qkv, kpm, nq, fill=7.0)
        assert (part[:, nq:] == 7.0).all()
        assert torch.equal(part[:, :nq], full[:, :nq])


# ------------------------------------------------------------------------------------------------- split3 image output
@gpu
@pytest.mark.parametrize("N,nq", SPLIT_SHAPES, ids=[f"N{n}-q{q}" for n, q in SPLIT_SHAPES])
def test_split3_output(dev, N, nq):
    """the three planes of the image sum exactly to the fp32 output on rows < n_query; the zero-prefilled image holds nothing else"""
    from multimodal_diffusion_amd import functional as Fn, _lib as L
    B = 3
    qkv = operands(B, N).to(dev)
    y = Fn.attention(qkv, H, n_query=nq).cpu().double().numpy()
    img = torch.zeros(L.lib().avd_split3_bytes(B * N, D), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    L.prof_enable(True)
    try:
        L.check(L.lib().avd_attn_fwd_split3_f32(qkv.data_ptr(), img.data_ptr(), B, N, H, 64, 0.125, nq, L.stream_ptr(dev)))
        torch.cuda.synchronize()
    finally:
        L.prof_enable(False)
    tags = {k: v[0] for k, v in L.prof_report().items() if v[0] > 0}
    assert tags == {kernel_tag(nq, True): 1}, tags
    planes = split3_decode(img.cpu().numpy(), B * N, D).astype(np.float64).reshape(3, B, N, D)
    assert np.array_equal(planes.sum(0)[:, :nq], y[:, :nq])
    assert y[:, :nq].any() and not planes[:, :, nq:].any()


# ------------------------------------------------------------------------------------------------- a sample with every key masked
@gpu
@pytest.mark.parametrize("N", ALL_MASKED_N)
def test_all_keys_masked_attends_uniformly(dev, N):
    """include/avdiff_hip.h, above avd_attn_fwd_f32: a sample whose keys are all padded attends uniformly — the mean of its v rows,
    on a ragged N too (the filler keys of the last tile weigh nothing) — and the other samples of the call do not notice."""
    B = 3
    qkv = operands(B, N)
    kpm = torch.zeros(B, N, dtype=torch.bool)
    kpm[1] = True
    out = attend(dev, qkv, kpm, N)
    mean = qkv[1, :, 2 * D:].double().mean(0)
    err = rel_err(out[1], mean.expand(N, D))
    record("all keys masked", err)
    assert err < TOL, err
    plain = attend(dev, qkv, None, N)
    assert torch.equal(out[0], plain[0]) and torch.equal(out[2], plain[2])
