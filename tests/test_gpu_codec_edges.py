"""The AudioCodec's two entry points (csrc/codec_f32.hip: avd_conv1d_act_f32, avd_avgpool_frames_f32) called directly at the shapes where
their kernels change path, and the AudioCodec at geometries other than the shipped one (hop 320, hidden 64, k 7 / 9, 150 frames), each
against plain torch in fp64 on the CPU (conv1d, avgpool) or the fp64 oracle (oracle/ref_cpu.py: codec_encode, codec_decode).

Bounds, both asserted, on conftest.rel_err: err < TOL (1e-4), and err <= 8 e32 + 1e-6, e32 = rel_err of the same reference evaluated in
fp32 on the CPU against its fp64 result (both sides add the same Cin x k fp32 products per output in different orders).  The matrix-pipe
conv1d must return the bits of the vector kernel (an fp32 FMA chain in the same (channel, tap) order)."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from _kit import dev  # noqa: F401  (fixture)
from _tune import tuned
from conftest import rel_err
from oracle import ref_cpu as R
from test_gpu_parity import TOL

pytestmark = pytest.mark.gpu

M, FLOOR = 8.0, 1e-6
ACTS = {"none": lambda v: v, "gelu": R.gelu_erf, "tanh": torch.tanh}


def _within(got, fn):
    """fn(dtype) -> the reference in that precision; -> (ok, err, e32)"""
    ref = fn(torch.float64)
    e32 = rel_err(fn(torch.float32), ref)
    err = rel_err(got.cpu(), ref)
    print(f"[codec edges] err {err:.3e} e32 {e32:.3e} ratio {err / max(e32, 1e-30):.2f}")
    return err < TOL and err <= M * e32 + FLOOR, err, e32


def _conv_case(dev, B, Cin, Cout, Lin, up, k, act, bias, seed=0):
    """-> (conv on the device, x on the device, the reference as a function of the dtype)"""
    g = torch.Generator().manual_seed(1000 * Cin + 10 * Cout + k + seed)
    conv = nn.Conv1d(Cin, Cout, k, padding=k // 2, bias=bias)
    with torch.no_grad():
        conv.weight.copy_((torch.rand(conv.weight.shape, generator=g) * 2 - 1) / (Cin * k) ** 0.5)
        if bias:
            conv.bias.copy_(0.1 * torch.randn(Cout, generator=g))
    x = torch.randn(B, Cin, Lin, generator=g)
    w, b = conv.weight.detach().clone(), (conv.bias.detach().clone() if bias else None)

    def ref(dt):
        return ACTS[act](F.conv1d(x.to(dt).repeat_interleave(up, -1), w.to(dt), None if b is None else b.to(dt), padding=k // 2))

    return conv.to(dev), x.to(dev), ref


def _act_id(act):
    from multimodal_diffusion_amd import _lib as L
    return {"none": L.ACT_NONE, "gelu": L.ACT_GELU, "tanh": L.ACT_TANH}[act]


def _launches(call):
    """{conv1d tag: launches} of one call"""
    from multimodal_diffusion_amd import _lib as L
    L.prof_enable(True)
    try:
        call()
        torch.cuda.synchronize()
    finally:
        L.prof_enable(False)
    return {k: v[0] for k, v in L.prof_report().items() if k.startswith("conv1d") and v[0] > 0}


# ------------------------------------------------------------------------------------------------- C: conv1d, the vector kernel
# (B, Cin, Cout, Lin, up, k, act, bias).  Cin: 1, 5 (< one 16-channel staging pass), 16, 17, 40 (a ragged last pass); Cout: 1, 8, 16, 17, 70
# (a thread owns 16: ragged channel blocks) and 64 with k = 3 (off the matrix pipe); k: 1, 3, 5, 15; Lin x up: 1, 7 (shorter than the
# kernel), 255 / 256 / 257 (the 256-position tile), 600, and 320 / 640 by the x 320 upsample; up: 1, 3, 320
VECTOR = [
    (1, 1, 1, 1, 1, 1, "none", True),
    (1, 1, 8, 7, 1, 15, "gelu", True),
    (3, 5, 16, 255, 1, 3, "tanh", True),
    (1, 16, 17, 256, 1, 5, "gelu", True),
    (3, 17, 70, 257, 1, 3, "none", True),
    (1, 40, 1, 600, 1, 15, "tanh", True),
    (1, 5, 8, 85, 3, 5, "gelu", True),
    (3, 16, 16, 200, 3, 1, "none", True),
    (1, 17, 17, 2, 320, 15, "gelu", True),
    (1, 40, 70, 1, 320, 3, "tanh", True),
    (3, 1, 64, 256, 1, 3, "gelu", True),
    (1, 16, 64, 257, 1, 3, "none", False),
    (3, 40, 8, 7, 1, 5, "tanh", True),
    (1, 5, 70, 1, 1, 3, "gelu", True),
    (1, 1, 16, 600, 1, 1, "tanh", True),
    (3, 17, 1, 255, 1, 15, "none", True),
    (1, 40, 16, 257, 1, 1, "gelu", True),
    (1, 16, 8, 256, 1, 15, "tanh", True),
    (3, 5, 17, 600, 1, 5, "none", True),
    (1, 1, 70, 257, 1, 15, "gelu", False),
    (1, 17, 16, 7, 1, 3, "gelu", True),
    (1, 40, 17, 85, 3, 15, "none", True),
    (3, 16, 1, 1, 1, 5, "tanh", True),
    (1, 5, 1, 256, 1, 1, "gelu", True),
    (1, 1, 17, 2, 320, 5, "tanh", True),
    (3, 40, 64, 200, 3, 3, "gelu", True),
    (1, 17, 8, 7, 1, 15, "none", True),
    (1, 16, 70, 1, 1, 15, "tanh", True),
]


def test_vector_cases_cover_every_value():
    cols = list(zip(*VECTOR))
    assert set(cols[0]) == {1, 3} and set(cols[1]) == {1, 5, 16, 17, 40} and set(cols[2]) == {1, 8, 16, 17, 64, 70}
    assert set(cols[4]) == {1, 3, 320} and set(cols[5]) == {1, 3, 5, 15} and set(cols[6]) == set(ACTS) and set(cols[7]) == {True, False}
    assert {c[3] * c[4] for c in VECTOR} >= {1, 7, 255, 256, 257, 600}
    assert all(c[5] == 3 for c in VECTOR if c[2] == 64)


@pytest.mark.parametrize("case", VECTOR, ids=["-".join(str(v) for v in c) for c in VECTOR])
def test_conv1d_vector_kernel(dev, case):
    from multimodal_diffusion_amd.audio_codec import _conv1d
    B, Cin, Cout, Lin, up, k, act, bias = case
    conv, x, ref = _conv_case(dev, *case)
    ran = _launches(lambda: _conv1d(x, conv, _act_id(act), upsample=up))
    assert ran == {"conv1d_ncl_kernel": 1}, ran
    out = _conv1d(x, conv, _act_id(act), upsample=up)
    assert out.shape == (B, Cout, Lin * up)
    ok, err, e32 = _within(out, ref)
    assert ok, (err, e32)


# ------------------------------------------------------------------------------------------------- C: conv1d, the matrix-pipe kernel
# (Cin, k, Lin, up, act), Cout = 64, B = 3.  Cin 16 / 32 / 48: one to three 16-channel passes, whose weight staging starts at c0 > 0;
# Lin x up: 5, 256, 257, 700
MFMA = [
    (16, 7, 5, 1, "gelu"),
    (32, 9, 256, 1, "tanh"),
    (48, 7, 257, 1, "none"),
    (64, 9, 700, 1, "gelu"),
    (16, 9, 64, 4, "none"),
    (48, 9, 175, 4, "gelu"),
    (32, 7, 700, 1, "none"),
    (64, 7, 64, 4, "tanh"),
    (16, 7, 257, 1, "tanh"),
    (48, 9, 5, 1, "gelu"),
    (32, 9, 257, 1, "gelu"),
    (64, 7, 5, 1, "none"),
]


@pytest.mark.parametrize("case", MFMA, ids=["-".join(str(v) for v in c) for c in MFMA])
def test_conv1d_matrix_pipe_kernel(dev, case):
    from multimodal_diffusion_amd.audio_codec import _conv1d
    Cin, k, Lin, up, act = case
    conv, x, ref = _conv_case(dev, 3, Cin, 64, Lin, up, k, act, True)
    ran = _launches(lambda: _conv1d(x, conv, _act_id(act), upsample=up))
    assert ran == {"conv1d_mfma_kernel": 1}, ran
    out = _conv1d(x, conv, _act_id(act), upsample=up)
    ok, err, e32 = _within(out, ref)
    assert ok, (err, e32)
    with tuned(codec_mfma=0):
        ran = _launches(lambda: _conv1d(x, conv, _act_id(act), upsample=up))
        vec = _conv1d(x, conv, _act_id(act), upsample=up)
    assert ran == {"conv1d_ncl_kernel": 1}, ran
    assert torch.equal(out, vec), float((out - vec).abs().max())


@pytest.mark.parametrize("Cin,Cout,k", [(24, 64, 7), (16, 64, 5), (16, 32, 7)], ids=["Cin24", "k5", "Cout32"])
def test_conv1d_shapes_the_matrix_pipe_does_not_take(dev, Cin, Cout, k):
    from multimodal_diffusion_amd.audio_codec import _conv1d
    conv, x, ref = _conv_case(dev, 3, Cin, Cout, 257, 1, k, "gelu", True)
    ran = _launches(lambda: _conv1d(x, conv, _act_id("gelu")))
    assert ran == {"conv1d_ncl_kernel": 1}, ran
    ok, err, e32 = _within(_conv1d(x, conv, _act_id("gelu")), ref)
    assert ok, (err, e32)


@pytest.mark.parametrize("k", [4, 17])
def test_conv1d_refuses_even_and_long_kernels(dev, k):
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd.audio_codec import _conv1d
    g = torch.Generator().manual_seed(k)
    x, w, b = (torch.randn(s, generator=g).to(dev) for s in ((2, 16, 40), (64, 16, k), (64,)))
    out = torch.full((2, 64, 40), 7.0, device=dev)
    with pytest.raises(L.AvdError, match=rf"conv1d: odd kernel size 1\.\.15 supported \(got {k}\)"):
        L.check(L.lib().avd_conv1d_act_f32(x.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), 2, 16, 64, 40, 1, k, L.ACT_GELU,
                                           L.stream_ptr(dev)))
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    conv = nn.Conv1d(16, 64, k, padding=k // 2).to(dev)
    with pytest.raises(L.AvdError, match=rf"\(got {k}\)"):
        _conv1d(x, conv, L.ACT_GELU)


# ------------------------------------------------------------------------------------------------- C: avgpool_frames
# (rows, L, Fa, hop): exact; padded (the zeros count in the mean); cropped; whole frames past the end; hop 1; more than one block of 256
POOL = [(5, 12, 4, 3), (5, 10, 4, 3), (5, 13, 4, 3), (3, 4, 6, 3), (4, 9, 9, 1), (7, 1000, 50, 20)]


def _pool_ref(x, Fa, hop):
    def ref(dt):
        h, total = x.to(dt), Fa * hop
        h = F.pad(h, (0, total - h.shape[-1])) if total > h.shape[-1] else h[..., :total]
        return h.view(h.shape[0], Fa, hop).mean(-1)
    return ref


@pytest.mark.parametrize("rows,Ln,Fa,hop", POOL)
def test_avgpool_frames(dev, rows, Ln, Fa, hop):
    from multimodal_diffusion_amd import _lib as L
    x = torch.randn(rows, Ln, generator=torch.Generator().manual_seed(Ln)) + 0.5
    xd = x.to(dev)
    out = torch.full((rows, Fa), 7.0, device=dev)
    L.check(L.lib().avd_avgpool_frames_f32(xd.data_ptr(), out.data_ptr(), rows, Ln, Fa, hop, L.stream_ptr(dev)))
    ok, err, e32 = _within(out, _pool_ref(x, Fa, hop))
    assert ok, (err, e32)


@pytest.mark.parametrize("Ln,fpc", [(12, None), (10, None), (13, 4), (9, 9)], ids=["exact", "padded", "hop-bumped", "hop1"])
def test_avgpool_frames_through_the_module(dev, Ln, fpc):
    """AudioCodec._avgpool_frames: frames_per_clip None = ceil(L / hop) frames of the configured hop (3); a target frame count = the
    exact-pool hop (13 samples in 4 frames: round(13 / 4) = 3 does not cover them, so 4)"""
    from multimodal_diffusion_amd.audio_codec import AudioCodec, AudioCodecConfig
    codec = AudioCodec(AudioCodecConfig(hop_samples=3, hidden=8, frames_per_clip=fpc))
    x = torch.randn(2, 5, Ln, generator=torch.Generator().manual_seed(Ln)) + 0.5
    out = codec._avgpool_frames(x.to(dev), target_Fa=fpc)
    Fa, hop = (-(-Ln // 3), 3) if fpc is None else (fpc, R._exact_pool(Ln, fpc)[0])
    assert out.shape == (2, 5, Fa)
    ok, err, e32 = _within(out.reshape(10, Fa), _pool_ref(x.reshape(10, Ln), Fa, hop))
    assert ok, (err, e32)


# ------------------------------------------------------------------------------------------------- D: AudioCodec at other geometries
# (hop_samples, hidden, smooth_kernel, frames_per_clip, wav length, frames)
GEOMETRIES = [
    (320, 64, 7, None, 3300, 11),        # frames_per_clip None: 11 frames of 320, the last one padded
    (160, 32, 5, 20, 3333, 20),          # exact-pool hop 167 (20 x 167 = 3,340 >= 3,333)
    (7, 64, 9, 37, 260, 37),             # round(260 / 37) = 7 covers 259 samples only: the hop bumps to 8
    (33, 48, 15, 10, 300, 10),
]


@pytest.mark.parametrize("lat_ch", [3, 8])
@pytest.mark.parametrize("geo", GEOMETRIES, ids=[f"hop{g[0]}-hidden{g[1]}-k{g[2]}-frames{g[3]}" for g in GEOMETRIES])
def test_audio_codec_geometry(dev, geo, lat_ch):
    from multimodal_diffusion_amd.audio_codec import AudioCodec, AudioCodecConfig
    hop, hidden, k, fpc, n, Fa = geo
    torch.manual_seed(hop + lat_ch)
    codec = AudioCodec(AudioCodecConfig(lat_ch=lat_ch, hop_samples=hop, hidden=hidden, smooth_kernel=k, frames_per_clip=fpc)).eval()
    g = torch.Generator().manual_seed(n + lat_ch)
    with torch.no_grad():
        for name, p in codec.named_parameters():
            if name.endswith("bias"):                       # the module zeroes them at construction
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
    W = {name: p.detach().clone() for name, p in codec.state_dict().items()}
    codec = codec.to(dev)
    wav = 0.5 * torch.randn(2, 1, n, generator=g)
    zin = torch.randn(2, lat_ch, Fa, generator=g)

    z = codec.encode(wav.to(dev))
    assert z.shape == (2, lat_ch, Fa)
    ok, err, e32 = _within(z, lambda dt: R.codec_encode(wav.to(dt), {a: b.to(dt) for a, b in W.items()}, frames_per_clip=fpc, hop=hop))
    assert ok, ("encode", err, e32)

    out = codec.decode(zin.to(dev))
    assert out.shape == (2, 1, Fa * hop) and float(out.abs().max()) <= 1.0
    ok, err, e32 = _within(out, lambda dt: R.codec_decode(zin.to(dt), {a: b.to(dt) for a, b in W.items()}, hop=hop))
    assert ok, ("decode", err, e32)
