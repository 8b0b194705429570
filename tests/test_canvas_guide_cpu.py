"""CPU-only checks of the canvas-keyed latent guide (include/avdiff_hip.h, "canvas-keyed known noise"; no GPU, no kernel launches):
the header declares the new entries, _lib binds them and the pinned ABI stays; the C entries refuse bad arguments before any HIP call;
the numpy mirror against _guide_ref.q_f64 on a hand-gathered case; canvas_frame_mask; and the refusals of functional.latent_guide and
stream_generate that need no device."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

import _canvas_guide_ref as CG
import _consensus_ref as W
import _guide_ref as G
from _kit import STREAM_HALF_SECOND, pipeline_cfg
from conftest import ROOT

SEED = 0xDEADBEEF12345678


def test_header_declares_lib_binds_and_abi_stays():
    from multimodal_diffusion_amd import _lib as L
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    for name in ("avd_latent_guide_canvas_f32", "avd_denoise_step_canvas_guided_f32"):
        assert name in declared and name in L.SIGNATURES
        assert hasattr(L.lib(), name)
    assert "canvas-keyed known noise" in header and "canvas-keyed known noise is not implemented" not in header
    assert L.ABI_VERSION == 7 and L.lib().avd_abi_version() == 7
    assert [f[0] for f in L.LatentGuide._fields_] == ["known", "mask", "mask_batch_stride", "key"] and C.sizeof(L.LatentGuide) == 40


def _step_desc(L, eta, B=3):
    s = L.StepDesc()
    e = s.embed
    e.target_kind, e.target_first, e.B, e.d, e.tdim = 0, 1, B, 512, 256
    e.C, e.T, e.H, e.W, e.p0, e.p1, e.p2, e.Nt, e.Np = 8, 4, 16, 16, 2, 4, 4, 32, 10
    s.T_train, s.guidance, s.eta = 1000, 3.0, eta
    return s


def test_argument_errors_without_gpu():
    """every refusal comes back before a HIP call: the pointers below are small integers nobody may dereference"""
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    known, z, out = 1 << 20, 2 << 20, 3 << 20                                   # apart: the overlap checks pass
    g = L.LatentGuide(known, None, 0, L.NoiseKey(1, 0))
    f = lib.avd_latent_guide_canvas_f32
    dims = (4, 8, 6, 2, 16)                                                     # N, outer, L, hop, inner
    assert f(None, 16, 16, 1000, z, out, *dims, None) == L.EINVAL
    assert b"null guide" in lib.avd_last_error()
    assert f(C.byref(g), 16, 16, 1000, z, out, 4, 8, 6, 0, 16, None) == L.EINVAL
    assert b"hop" in lib.avd_last_error()
    assert f(C.byref(g), 16, 16, 1000, z, out, 4, 8, 6, -3, 16, None) == L.EINVAL
    assert f(C.byref(g), 16, 16, 1000, z, out, 0, 8, 6, 2, 16, None) == L.EINVAL
    assert f(C.byref(g), None, 16, 1000, z, out, *dims, None) == L.EINVAL       # tau
    assert f(C.byref(g), 16, 16, 1000, z, known, *dims, None) == L.EINVAL       # out over known
    assert b"overlap" in lib.avd_last_error()
    # the range: (sample_offset + N - 1)*hop + L <= 2^32
    top = L.LatentGuide(known, None, 0, L.NoiseKey(1, 2 ** 32 - 1))
    assert f(C.byref(top), 16, 16, 1000, z, out, 1, 8, 6, 2, 16, None) == L.EINVAL     # (2^32 - 1)*2 + 6
    assert b"2^32" in lib.avd_last_error()
    assert f(C.byref(top), 16, 16, 1000, z, out, 1, 8, 2, 1, 16, None) == L.EINVAL     # (2^32 - 1) + 2 = 2^32 + 1
    assert f(C.byref(top), 16, 16, 1000, z, out, 2, 8, 1, 1, 16, None) == L.EINVAL     # window index 2^32
    neg = L.LatentGuide(known, None, 0, L.NoiseKey(1, -1))
    assert f(C.byref(neg), 16, 16, 1000, z, out, *dims, None) == L.EINVAL
    assert f(C.byref(g), 16, 16, 1000, z, out, 4, 1 << 20, 6, 2, 1 << 14, None) == L.EINVAL      # outer*inner = 2^34
    assert b"2^34" in lib.avd_last_error()
    bad_stride = L.LatentGuide(known, 4 << 20, 7, L.NoiseKey(1, 0))
    assert f(C.byref(bad_stride), 16, 16, 1000, z, out, *dims, None) == L.EINVAL
    assert b"mask_batch_stride" in lib.avd_last_error()

    step = lib.avd_denoise_step_canvas_guided_f32
    zs, Xp, zo = 5 << 20, 6 << 20, 7 << 20
    tail = (zs, Xp, 16, 16, zo, 16, 1 << 20, None)

    def call(s, guide, hop, k, ctl=None, cond_only=0, t_last=None, hist=None):
        return step(None if s is None else C.byref(s), None if guide is None else C.byref(guide), hop, None if k is None else C.byref(k),
                    None if ctl is None else C.byref(ctl), cond_only, t_last, hist, *tail)

    assert call(None, g, 2, None) == L.EINVAL
    assert call(_step_desc(L, 0.0), None, 2, None) == L.EINVAL
    assert b"guide" in lib.avd_last_error()
    assert call(_step_desc(L, 0.0), g, 0, None) == L.EINVAL
    assert b"hop" in lib.avd_last_error()
    assert call(_step_desc(L, 0.0), top, 2, None) == L.EINVAL
    assert b"2^32" in lib.avd_last_error()
    assert call(_step_desc(L, 0.0), top, 2, None, cond_only=1) == L.EINVAL      # the cond-only form as well
    # a canvas guide at eta > 0 without a key: there is no per-sample or unseeded noise under it
    assert call(_step_desc(L, 0.5), g, 2, None) == L.EINVAL
    assert b"noise key" in lib.avd_last_error()
    assert call(_step_desc(L, 0.5), g, 2, None, t_last=16, hist=8 << 20) == L.EINVAL
    assert b"noise key" in lib.avd_last_error()
    # the step's own canvas key is range-checked with the same hop
    assert call(_step_desc(L, 0.5), g, 2, L.NoiseKey(1, 2 ** 32 - 1)) == L.EINVAL
    assert b"2^32" in lib.avd_last_error()
    ctl = L.CfgControl(16, None, None, 0)
    assert call(_step_desc(L, 0.0), g, 2, None, ctl=ctl, cond_only=1) == L.EINVAL
    assert b"cond-only" in lib.avd_last_error()
    assert call(_step_desc(L, 0.0), g, 2, None, t_last=16) == L.EINVAL          # t_last without x0_hist
    assert b"go together" in lib.avd_last_error()
    over = L.LatentGuide(zo, None, 0, L.NoiseKey(1, 0))                         # known over z_out
    assert call(_step_desc(L, 0.0), over, 2, None) == L.EINVAL
    assert b"overlap" in lib.avd_last_error()


def test_mirror_is_the_gather_and_agrees_on_overlaps():
    for shape, hop, off in (((3, 8, 4, 4, 8), 1, 0), ((3, 2, 4, 2, 3), 2, 5), ((3, 8, 40), 4, 2), ((4, 8, 30), 31, 0)):
        outer, L_, inner = W.dims(shape)
        n = CG.canvas_known_normals(SEED, shape, hop, off)
        assert n.shape == shape and np.isfinite(n).all() and W.overlaps_agree(n, hop)
        # by hand: element (o, l, i) of window b is element o*inner + i of sample (off + b)*hop + l of the per-sample guide stream
        rng = np.random.default_rng(1)
        for _ in range(20):
            b, o, l, i = (int(rng.integers(0, s)) for s in (shape[0], outer, L_, inner))
            p = (off + b) * hop + l
            assert n.reshape(shape[0], outer, L_, inner)[b, o, l, i] == G.known_normals(SEED, p, 1, outer * inner)[0, o * inner + i]
        # windows [lo, N) with window_offset + lo are that slice
        assert np.array_equal(CG.canvas_known_normals(SEED, (shape[0] - 1,) + shape[1:], hop, off + 1), n[1:])
        # not the per-sample keying, and a stream of its own (no timestep, its own tag)
        assert not np.array_equal(n, G.known_normals(SEED, off, shape[0], outer * L_ * inner).reshape(shape))


def test_mirror_q_against_guide_ref_hand_gathered():
    """q of the canvas keying = _guide_ref.q_f64 of the canvas read as P samples of outer*inner elements, gathered into windows"""
    abar = np.linspace(0.999, 0.01, 1000)
    shape, hop, off = (3, 2, 5, 2, 3), 2, 3
    outer, L_, inner = W.dims(shape)
    P = (shape[0] - 1) * hop + L_
    rng = np.random.default_rng(2)
    canvas = rng.standard_normal((outer, P, 2, 3))
    known = W.windows_from_canvas(canvas, L_, hop)
    tau = 412
    rows = canvas.transpose(1, 0, 2, 3).reshape(P, outer * inner)                    # sample p = canvas position p
    q_rows = G.q_f64(rows, [tau] * P, abar, SEED, sample_offset=off * hop)
    want = q_rows.reshape(P, outer, 2, 3).transpose(1, 0, 2, 3)
    got = CG.q_f64(known, [tau] * 3, abar, SEED, hop, window_offset=off)
    assert np.array_equal(got, W.windows_from_canvas(want, L_, hop))
    assert W.overlaps_agree(got, hop)
    # tau < 0: the known windows themselves
    assert np.array_equal(CG.q_f64(known, [-1] * 3, abar, SEED, hop), known)
    # the noise term passes through the consensus mean; the per-sample keying does not
    w = rng.uniform(0.25, 2.0, L_)
    assert np.allclose(W.consensus_f64(got, hop, w), got, rtol=1e-12, atol=1e-12)
    per = G.q_f64(known, [tau] * 3, abar, SEED, sample_offset=off)
    assert not np.allclose(W.consensus_f64(per, hop, w), per)


def test_canvas_frame_mask():
    from multimodal_diffusion_amd import sampler as S
    from multimodal_diffusion_amd.stream_infer import windows_from_canvas
    import multimodal_diffusion_amd as A
    assert A.canvas_frame_mask is S.canvas_frame_mask
    m = S.canvas_frame_mask((8, 5, 4, 4), 0, 2)
    assert m.dtype == torch.float32 and tuple(m.shape) == (8, 5, 4, 4)
    assert bool((m[:, :2] == 1).all()) and bool((m[:, 2:] == 0).all())
    a = S.canvas_frame_mask((8, 375), 100, 200)
    assert a.sum() == 800 and bool((a[:, 100:200] == 1).all())
    # cut into windows, every window holds its own part of the canvas mask
    mw = windows_from_canvas(m, 2, 1)
    assert tuple(mw.shape) == (4, 8, 2, 4, 4) and mw[0].min() == 1 and mw[1, :, 0].min() == 1 and mw[1, :, 1].max() == 0 and mw[2].max() == 0
    assert torch.equal(S.canvas_frame_mask((8, 5, 4, 4), 0, 0), torch.zeros(8, 5, 4, 4))
    for bad in ((8, 5, 4), (2, 8, 5, 4, 4), (8,)):
        with pytest.raises(ValueError, match="canvas"):
            S.canvas_frame_mask(bad, 0, 1)
    for lo, hi in ((-1, 2), (3, 2), (0, 6)):
        with pytest.raises(ValueError):
            S.canvas_frame_mask((8, 5, 4, 4), lo, hi)


def test_latent_guide_python_checks_need_no_device():
    from multimodal_diffusion_amd import functional as Fn
    sig = inspect.signature(Fn.latent_guide).parameters
    assert sig["canvas_hop"].default is None and sig["window_offset"].default == 0
    known, tau, abar = torch.zeros(3, 8, 4, 4, 4), torch.zeros(3, dtype=torch.long), torch.linspace(0.99, 0.01, 10)
    for bad_hop in (0, -1, 1.5, True):
        with pytest.raises(ValueError, match="hop"):
            Fn.latent_guide(known, tau, abar, canvas_hop=bad_hop)
    with pytest.raises(ValueError, match="window_offset"):
        Fn.latent_guide(known, tau, abar, window_offset=2)                       # without the keying
    with pytest.raises(ValueError, match="sample_offset"):
        Fn.latent_guide(known, tau, abar, canvas_hop=2, sample_offset=2)
    with pytest.raises(ValueError):
        Fn.latent_guide(known, tau, abar, canvas_hop=2, window_offset=-1)
    with pytest.raises(ValueError, match="2\\*\\*32"):
        Fn.latent_guide(known, tau, abar, canvas_hop=2, window_offset=2 ** 32 - 2)
    with pytest.raises(ValueError):
        Fn.latent_guide(torch.zeros(3, 8, 4, 4), tau, abar, canvas_hop=2)        # not a window batch


def test_engine_keywords():
    import multimodal_diffusion_amd as A
    sig = inspect.signature(A.DenoiseEngine.set_known).parameters
    assert sig["keying"].default == "sample" and sig["hop"].default is None and sig["guide_seed"].default == 0
    assert A.DenoiseEngine.GUIDE_KEYINGS == ("sample", "canvas")


def test_stream_generate_refusals_need_no_device():
    """raised before anything is encoded: no module and no device is touched"""
    from multimodal_diffusion_amd import stream_infer as S
    from multimodal_diffusion_amd.sampler import canvas_frame_mask
    sig = inspect.signature(S.stream_generate).parameters
    assert all(sig[k].default is None for k in ("init_video", "init_audio", "mask", "guide_seed")) and sig["strength"].default == 1.0
    wav = np.zeros(18000, dtype=np.float32)                                     # 4 windows of 0.5 s
    vid = np.zeros((20, 32, 32, 3), dtype=np.uint8)                             # 4 windows of 0.5 s
    mods = dict(vid_vae=None, aud_codec=None, adapt_v=None, adapt_a=None, core=None, head=None, tstep_dim=256, device=torch.device("cpu"))
    a2v = dict(mods, prompt_modality="audio", prompt_video=None, prompt_audio=wav)
    v2a = dict(mods, prompt_modality="video", prompt_video=vid, prompt_audio=None)
    cfg = pipeline_cfg(clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND)
    canvas = (8, 5, 4, 4)
    mask = canvas_frame_mask(canvas, 0, 2)
    # an init clip of the wrong modality
    with pytest.raises(ValueError, match="init_audio"):
        S.stream_generate(cfg=cfg, init_audio=wav, **a2v)
    with pytest.raises(ValueError, match="init_video"):
        S.stream_generate(cfg=cfg, init_video=vid, **v2a)
    with pytest.raises(ValueError, match="not both"):
        S.stream_generate(cfg=cfg, init_video=vid, init_audio=wav, **a2v)
    # a mask or a strength without an init clip
    with pytest.raises(ValueError, match="init clip"):
        S.stream_generate(cfg=cfg, mask=mask, **a2v)
    with pytest.raises(ValueError, match="init clip"):
        S.stream_generate(cfg=cfg, strength=0.5, **a2v)
    with pytest.raises(ValueError, match="strength"):
        S.stream_generate(cfg=cfg, init_video=vid, strength=1.5, **a2v)
    # the init clip's own form
    with pytest.raises(ValueError, match="uint8"):
        S.stream_generate(cfg=cfg, init_video=vid.astype(np.float32), **a2v)
    with pytest.raises(ValueError, match="waveform"):
        S.stream_generate(cfg=cfg, init_audio=wav.astype(np.int16), **v2a)
    # a window count mismatch: 12 frames are 2 windows, the prompt gives 4
    with pytest.raises(ValueError, match="2 windows.*4"):
        S.stream_generate(cfg=cfg, init_video=vid[:12], **a2v)
    with pytest.raises(ValueError, match="windows"):
        S.stream_generate(cfg=cfg, init_audio=wav[:9000], **v2a)
    # a mask that does not broadcast to the canvas [8, 5, 4, 4], or leaves [0, 1]
    for bad in (torch.ones(8, 4, 4, 4), torch.ones(4, 8, 2, 4, 4), torch.ones(3)):
        with pytest.raises(ValueError, match="broadcast"):
            S.stream_generate(cfg=cfg, init_video=vid, mask=bad, **a2v)
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        S.stream_generate(cfg=cfg, init_video=vid, mask=2.0 * mask, **a2v)
    with pytest.raises(ValueError, match="broadcast"):
        S.stream_generate(cfg=cfg, init_audio=wav, mask=torch.ones(8, 374), **v2a)      # the audio canvas is [8, 375]
    # sharding an init clip is out of scope, and says so
    with pytest.raises(ValueError, match="second broadcast"):
        S.stream_generate(cfg=cfg, init_video=vid, shard=True, **a2v)
    # under consensus the same refusals hold (the canvas is the consensus canvas)
    with pytest.raises(ValueError, match="broadcast"):
        S.stream_generate(cfg=cfg, init_video=vid, mask=torch.ones(8, 4, 4, 4), consensus="uniform", **a2v)
