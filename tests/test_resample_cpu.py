"""CPU-only checks of RePaint resampling (include/avdiff_hip.h, "renoise"; no GPU, no kernel launches): the header declares the two
entries, _lib binds them and the pinned ABI stays; the C entries refuse bad arguments before any HIP call; resample_schedule and
step_segments; the float64 reference (identity case, jump, canvas keying commutes with cutting a canvas into windows); and the
refusals of functional.renoise, sample_one_direction and stream_generate that need no device."""
import ctypes as C
import inspect
import re

import numpy as np
import pytest
import torch

import _consensus_ref as W
import _guide_ref as G
import _noise_ref as NR
import _renoise_ref as RR
from _kit import ABAR, STREAM_HALF_SECOND, pipeline_cfg
from conftest import ROOT

SEED, GSEED = 0xDEADBEEF12345678, 0x1234567ABCDEF01


def test_header_declares_lib_binds_and_abi_stays():
    from multimodal_diffusion_amd import _lib as L
    header = (ROOT / "include" / "avdiff_hip.h").read_text()
    declared = set(re.findall(r"\b(avd_[a-z0-9_]+)\s*\(", header))
    for name in ("avd_renoise_f32", "avd_renoise_canvas_f32"):
        assert name in declared and name in L.SIGNATURES and hasattr(L.lib(), name)
    assert "0x52504E31" in header and "---- renoise" in header
    assert L.ABI_VERSION == 7 and L.lib().avd_abi_version() == 7
    assert declared == set(L.SIGNATURES)


def test_argument_errors_without_gpu():
    """every refusal comes back before a HIP call: the pointers below are small integers nobody may dereference"""
    from multimodal_diffusion_amd import _lib as L
    lib = L.lib()
    known, z, out = 1 << 20, 2 << 20, 3 << 20
    key = L.NoiseKey(1, 0)
    f = lib.avd_renoise_f32
    assert f(None, 0, None, 16, 16, 16, 1000, z, out, 2, 64, None) == L.EINVAL
    assert b"noise key" in lib.avd_last_error()
    assert f(C.byref(key), 0, None, None, 16, 16, 1000, z, out, 2, 64, None) == L.EINVAL          # t_from
    assert f(C.byref(key), 0, None, 16, 16, 16, 1000, None, out, 2, 64, None) == L.EINVAL          # z
    assert f(C.byref(key), 0, None, 16, 16, 16, 0, z, out, 2, 64, None) == L.EINVAL                # T_train
    assert f(C.byref(key), 0, None, 16, 16, 16, 1000, z, out, 0, 64, None) == L.EINVAL
    assert f(C.byref(key), 0, None, 16, 16, 16, 1000, z, out, 2, 0, None) == L.EINVAL
    assert f(C.byref(key), 0, None, 16, 16, 16, 1000, z, z + 16, 2, 64, None) == L.EINVAL          # partial overlap
    assert b"overlap" in lib.avd_last_error()
    assert f(C.byref(L.NoiseKey(1, 2 ** 32 - 1)), 0, None, 16, 16, 16, 1000, z, out, 2, 64, None) == L.EINVAL
    assert b"2^32" in lib.avd_last_error()
    over = L.LatentGuide(out, None, 0, L.NoiseKey(1, 0))                                           # known over out
    assert f(C.byref(key), 0, C.byref(over), 16, 16, 16, 1000, z, out, 2, 64, None) == L.EINVAL
    assert b"overlap" in lib.avd_last_error()
    bad_stride = L.LatentGuide(known, 4 << 20, 7, L.NoiseKey(1, 0))
    assert f(C.byref(key), 0, C.byref(bad_stride), 16, 16, 16, 1000, z, out, 2, 64, None) == L.EINVAL
    assert b"mask_batch_stride" in lib.avd_last_error()

    fc = lib.avd_renoise_canvas_f32
    dims = (4, 8, 6, 2, 16)                                                                        # N, outer, L, hop, inner
    assert fc(None, 0, None, 16, 16, 16, 1000, z, out, *dims, None) == L.EINVAL
    assert fc(C.byref(key), 0, None, 16, 16, 16, 1000, z, out, 4, 8, 6, 0, 16, None) == L.EINVAL
    assert b"hop" in lib.avd_last_error()
    assert fc(C.byref(L.NoiseKey(1, 2 ** 32 - 1)), 0, None, 16, 16, 16, 1000, z, out, 1, 8, 6, 2, 16, None) == L.EINVAL
    assert b"2^32" in lib.avd_last_error()
    assert fc(C.byref(key), 0, None, 16, 16, 16, 1000, z, out, 4, 1 << 20, 6, 2, 1 << 14, None) == L.EINVAL
    assert b"2^34" in lib.avd_last_error()
    assert fc(C.byref(key), 0, None, 16, None, 16, 1000, z, out, *dims, None) == L.EINVAL         # t_to
    # the guide's key and the renoise key must carry the same window offset
    g2 = L.LatentGuide(known, None, 0, L.NoiseKey(7, 2))
    assert fc(C.byref(key), 0, C.byref(g2), 16, 16, 16, 1000, z, out, *dims, None) == L.EINVAL
    assert b"same sample_offset" in lib.avd_last_error()
    assert fc(C.byref(key), 0, C.byref(over), 16, 16, 16, 1000, z, out, *dims, None) == L.EINVAL
    assert b"overlap" in lib.avd_last_error()


# ------------------------------------------------------------------------------------------------- schedules
def _counts(n, jump, resamples):
    """(denoising steps, jumps) from the block rule: every block but the one that ends in -1 runs `resamples` times"""
    steps = jumps = 0
    for a in range(0, n, jump):
        b = min(a + jump, n)
        reps = resamples if b < n else 1
        steps += reps * (b - a)
        jumps += reps - 1
    return steps, jumps


def test_resample_schedule():
    from multimodal_diffusion_amd import schedule_utils as su
    s = su.make_sampling_schedule(1000, 4)
    s0, s1, s2, s3, s4 = s.tolist()
    assert s4 == -1
    out = su.resample_schedule(s, 2, 2)
    assert out.dtype == torch.long and out.tolist() == [s0, s1, s2, s0, s1, s2, s3, s4]
    assert su.resample_schedule(s, 1, 3).tolist() == [s0, s1, s0, s1, s0, s1, s2, s1, s2, s1, s2, s3, s2, s3, s2, s3, s4]
    assert su.resample_schedule(s, 3, 2).tolist() == [s0, s1, s2, s3, s0, s1, s2, s3, s4]
    assert su.resample_schedule(s, 4, 5).tolist() == s.tolist() and su.resample_schedule(s, 9, 2).tolist() == s.tolist()
    for n in (1, 2, 5, 6, 7, 50):
        sched = su.make_sampling_schedule(1000, n)
        for jump in (1, 2, 3, 10):
            assert torch.equal(su.resample_schedule(sched, jump, 1), sched)                        # resamples == 1: the identity
            for resamples in (2, 3):
                r = su.resample_schedule(sched, jump, resamples).tolist()
                pairs = list(zip(r[:-1], r[1:]))
                steps, jumps = _counts(n, jump, resamples)
                assert sum(b < a for a, b in pairs) == steps and sum(b > a for a, b in pairs) == jumps
                assert len(r) == steps + jumps + 1 and r[0] == sched[0] and r[-1] == -1 and r.count(-1) == 1
                assert all(a >= 0 for a, b in pairs if b > a)                                      # a jump never starts at -1
                assert all(a != b for a, b in pairs) and set(r) == set(sched.tolist())
                for a, b in pairs:                                                                 # a jump goes back `<= jump` entries
                    if b > a:
                        ia, ib = sched.tolist().index(a), sched.tolist().index(b)
                        assert 1 <= ia - ib <= jump and ib % jump == 0
    # truncated first, then expanded: the tail of the schedule, from its own block boundaries
    tail = su.truncate_schedule(su.make_sampling_schedule(1000, 6), 0.5)
    assert su.resample_schedule(tail, 2, 2).tolist() == [tail[0], tail[1], tail[2], tail[0], tail[1], tail[2], tail[3]]
    assert su.resample_schedule(torch.tensor([-1]), 2, 2).tolist() == [-1]                        # strength 0: no steps
    for bad in (dict(jump=0, resamples=2), dict(jump=2, resamples=0), dict(jump=1.5, resamples=2), dict(jump=True, resamples=2),
                dict(jump=2, resamples="2")):
        with pytest.raises(ValueError):
            su.resample_schedule(s, **bad)
    with pytest.raises(ValueError, match="-1"):
        su.resample_schedule(torch.tensor([900, 500, 100]), 2, 2)
    with pytest.raises(ValueError, match="decreasing"):
        su.resample_schedule(out, 2, 2)                                                            # already resampled
    with pytest.raises(ValueError, match="decreasing"):
        su.resample_schedule(torch.tensor([900, 900, -1]), 2, 2)
    assert su.check_resample(None) is None and su.check_resample((2, 3)) == (2, 3) and su.check_resample([4, 1]) == (4, 1)
    assert su.check_resample({"jump": 10, "resamples": 2}) == (10, 2)
    assert su.resample_from_config({}) is None and su.resample_from_config({"resample": {"jump": 2, "resamples": 2}}) == (2, 2)
    for bad in ((2,), (2, 2, 2), "22", {"jump": 2}, {"jump": 2, "resamples": 2, "x": 1}, (0, 2), (2, 2.0)):
        with pytest.raises(ValueError):
            su.check_resample(bad)


def test_step_segments():
    from multimodal_diffusion_amd import schedule_utils as su
    s = su.make_sampling_schedule(1000, 4)                                                         # 999, 749, 499, 249, -1
    assert s.tolist() == [999, 749, 499, 249, -1]
    # without jumps: guidance_segments with the kinds spelled out
    for iv in (None, (300, 800), (0, 100), (999, 999)):
        assert su.step_segments(s, iv) == [(a, b, "cfg" if c else "cond") for a, b, c in su.guidance_segments(s, iv)]
    r = su.resample_schedule(s, 2, 2)                                                              # 999 749 499 | 999 749 499 249 -1
    assert su.step_segments(r, None) == [(0, 2, "cfg"), (2, 3, "renoise"), (3, 7, "cfg")]
    assert su.step_segments(r, (300, 800)) == [(0, 1, "cond"), (1, 2, "cfg"), (2, 3, "renoise"), (3, 4, "cond"), (4, 6, "cfg"),
                                               (6, 7, "cond")]
    # a renoise is a renoise whatever the interval says about its t_now
    assert su.step_segments(r, (499, 499))[1:3] == [(2, 3, "renoise"), (3, 5, "cond")]
    segs = su.step_segments(su.resample_schedule(s, 1, 2), None)
    assert [k for _, _, k in segs] == ["cfg", "renoise", "cfg", "renoise", "cfg", "renoise", "cfg"]
    assert [i for a, b, _ in segs for i in range(a, b)] == list(range(10))                         # a partition, in order
    assert su.step_segments(torch.tensor([100, 300, 500]), None) == [(0, 2, "renoise")]
    with pytest.raises(ValueError, match="both 749"):
        su.step_segments(torch.tensor([999, 749, 749, -1]), None)
    assert su.has_jumps(r) and not su.has_jumps(s) and not su.has_jumps(torch.tensor([-1]))
    # a resampling schedule is known by its time travel, a jump back to a timestep already passed; a climb to a new timestep is not
    # one (the DDIM engine steps through it as it always has, the multistep solver refuses it)
    assert not su.has_jumps(torch.tensor([990, 900, 360, 700, 650, -1])) and su.has_jumps(torch.tensor([990, 900, 360, 900, 360, -1]))
    assert su.has_jumps(su.resample_schedule(s, 1, 2)) and su.has_jumps(su.resample_schedule(s, 3, 3))
    assert inspect.signature(su.guidance_segments).parameters.keys() == {"sched", "interval"}      # stays as it is


# ------------------------------------------------------------------------------------------------- the reference
def test_reference_stream_and_cases():
    abar = ABAR.numpy()
    # the renoise stream is the seeded stream with its own domain word and the visit in the timestep's place
    n = RR.renoise_normals(SEED, 3, 2, 37, visit=5)
    assert n.shape == (2, 37) and np.array_equal(n, G.known_normals(SEED, 3, 2, 37, tag=0x52504E31, t=5))
    assert not np.array_equal(n, NR.normals(SEED, 3, [5, 5], 37))                                  # DDIM's stream at t = visit
    assert not np.array_equal(n, G.known_normals(SEED, 3, 2, 37)) and not np.array_equal(n, RR.renoise_normals(SEED, 3, 2, 37, 6))
    big = RR.renoise_normals(SEED, 0, 4, 4096, 0)
    assert abs(big.mean()) < 0.05 and abs(big.std() - 1.0) < 0.05
    z = np.random.default_rng(0).standard_normal((4, 37))
    t_from, t_to = [100, -1, 500, 300], [600, 200, 500, 100]
    out = RR.renoise_f64(z, t_from, t_to, abar, SEED, 5)
    same, A, S = RR.coef(abar, t_from, t_to)
    assert same.tolist() == [False, False, True, True] and np.array_equal(out[2:], z[2:])          # t_to <= t_from: z itself
    a = G.abar_at(abar, [600, 200])
    assert np.allclose(A[:2] ** 2, [a[0] / G.abar_at(abar, [100])[0], a[1]]) and np.allclose(A ** 2 + S ** 2, 1.0)
    assert np.allclose(out[:2], A[:2, None] * z[:2] + S[:2, None] * RR.renoise_normals(SEED, 0, 2, 37, 5))
    # composing q(t) with the jump t -> t' has the variance of q(t'): A'^2 (1 - a_t) + S'^2 = 1 - a_t'
    af, at = G.abar_at(abar, [100])[0], G.abar_at(abar, [600])[0]
    assert np.isclose(A[0] ** 2 * (1 - af) + S[0] ** 2, 1 - at)
    # a_f == 0 is the identity case (no division)
    zero = abar.copy()
    zero[-1] = 0.0
    assert RR.coef(zero, [999], [999])[0].all() and RR.coef(zero, [999], [500])[0].all()
    # with a guide: q(t_to) where the mask is 1, the unguided jump where it is 0
    known = np.random.default_rng(1).standard_normal((4, 37))
    m = (np.arange(37) % 3 == 0).astype(np.float64)
    g = RR.renoise_f64(z, t_from, t_to, abar, SEED, 5, known=known, mask=m, guide_seed=GSEED)
    q = G.q_f64(known, t_to, abar, GSEED)
    assert np.array_equal(g[:, m == 1], q[:, m == 1]) and np.array_equal(g[:, m == 0], out[:, m == 0])


@pytest.mark.parametrize("shape,hop,off", [((3, 8, 4, 4, 4), 2, 0), ((3, 2, 4, 2, 3), 1, 5), ((3, 8, 40), 4, 2), ((4, 8, 30), 31, 0)])
def test_reference_canvas_renoise_commutes_with_the_windows(shape, hop, off):
    """canvas-keyed renoise of windows_from_canvas(canvas) = windows_from_canvas of the renoised canvas, where the canvas is renoised
    as P samples of outer*inner elements by the per-sample reference at [p, e']"""
    abar = ABAR.numpy()
    N = shape[0]
    outer, L_, inner = W.dims(shape)
    P = (N - 1) * hop + L_
    rng = np.random.default_rng(2)
    canvas = rng.standard_normal((outer, P) + tuple(shape[3:]))
    known_c = rng.standard_normal(canvas.shape)
    mask_c = (rng.random(canvas.shape) < 0.5).astype(np.float64)
    t_from, t_to, visit = 249, 749, 3

    def rows(c):                                              # [outer, P, *rest] -> [P, outer*inner]: position p as a sample
        return np.moveaxis(c.reshape(outer, P, inner), 1, 0).reshape(P, outer * inner)

    def back(r):
        return np.moveaxis(r.reshape(P, outer, inner), 0, 1).reshape(canvas.shape)

    for guided in (False, True):
        kw = dict(known=rows(known_c), mask=rows(mask_c), guide_seed=GSEED) if guided else {}
        ref_c = back(RR.renoise_f64(rows(canvas), [t_from] * P, [t_to] * P, abar, SEED, visit, sample_offset=off * hop, **kw))
        kww = dict(known=W.windows_from_canvas(known_c, L_, hop), mask=W.windows_from_canvas(mask_c, L_, hop),
                   guide_seed=GSEED) if guided else {}
        got = RR.renoise_canvas_f64(W.windows_from_canvas(canvas, L_, hop), [t_from] * N, [t_to] * N, abar, SEED, visit, hop, off, **kww)
        assert got.shape == shape and np.array_equal(got, W.windows_from_canvas(ref_c, L_, hop))
        assert W.overlaps_agree(got, hop)
    per = RR.renoise_f64(W.windows_from_canvas(canvas, L_, hop), [t_from] * N, [t_to] * N, abar, SEED, visit, sample_offset=off)
    if hop < L_:
        assert not W.overlaps_agree(per, hop)                 # keyed per sample the windows part


# ------------------------------------------------------------------------------------------------- refusals that need no device
def test_functional_renoise_refusals_need_no_device():
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn
    sig = inspect.signature(Fn.renoise).parameters
    assert list(sig)[:6] == ["z", "t_from", "t_to", "alpha_bar", "seed", "visit"]
    assert sig["sample_offset"].default == 0 and all(sig[k].default is None for k in ("guide", "canvas_hop", "out"))
    z, t = torch.zeros(2, 8, 4, 4, 4), torch.tensor([1, 2])
    with pytest.raises(L.AvdError, match="no CPU fallback"):
        Fn.renoise(z, t, t, ABAR, SEED, 0)
    for bad in (-1, 2 ** 32, 1.0, True):
        with pytest.raises(ValueError, match="visit"):
            Fn.check_visit(bad)
    assert Fn.check_visit(2 ** 32 - 1) == 2 ** 32 - 1


def test_engine_keywords():
    import multimodal_diffusion_amd as A
    sig = inspect.signature(A.DenoiseEngine.renoise).parameters
    assert list(sig) == ["self", "z", "t_from", "t_to", "visit", "out"] and sig["out"].default is None
    assert inspect.signature(A.sample_one_direction).parameters["resample"].default is None
    from multimodal_diffusion_amd import stream_infer as S
    assert inspect.signature(S.stream_generate).parameters["resample"].default is None


def test_pipeline_refusals_need_no_device():
    """raised before anything is encoded: no module and no device is touched"""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import stream_infer as S
    from multimodal_diffusion_amd.sampler import canvas_frame_mask, frame_mask
    wav = np.zeros(18000, dtype=np.float32)
    vid = np.zeros((20, 32, 32, 3), dtype=np.uint8)
    mods = dict(vid_vae=None, aud_codec=None, adapt_v=None, adapt_a=None, core=None, head=None, tstep_dim=256, device=torch.device("cpu"))
    a2v = dict(mods, prompt_modality="audio", prompt_video=None, prompt_audio=wav)
    cfg = pipeline_cfg(clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND)
    cfg_rs = dict(cfg, sampling=dict(cfg["sampling"], resample={"jump": 2, "resamples": 2}))
    mask_c, mask_1 = canvas_frame_mask((8, 5, 4, 4), 0, 2), frame_mask((8, 2, 4, 4), 0, 1)
    for fn, mask, init in ((S.stream_generate, mask_c, vid), (A.sample_one_direction, mask_1, vid[:8])):
        with pytest.raises(ValueError, match="needs an init clip with a mask"):
            fn(cfg=cfg, resample=(2, 2), noise_seed=1, **a2v)
        with pytest.raises(ValueError, match="needs an init clip with a mask"):
            fn(cfg=cfg, resample=(2, 2), noise_seed=1, init_video=init, **a2v)                     # SDEdit without a mask
        with pytest.raises(ValueError, match="needs noise_seed"):
            fn(cfg=cfg, resample=(2, 2), init_video=init, mask=mask, **a2v)
        with pytest.raises(ValueError, match="needs noise_seed"):
            fn(cfg=cfg_rs, init_video=init, mask=mask, **a2v)                                      # from the config
        with pytest.raises(ValueError, match="needs noise_seed"):
            fn(cfg=cfg, resample=(2, 1), init_video=init, mask=mask, **a2v)                        # resamples == 1 asks the same
        for bad in ((0, 2), (2,), "2x2", (2, 1.5)):
            with pytest.raises(ValueError, match="resample"):
                fn(cfg=cfg, resample=bad, noise_seed=1, init_video=init, mask=mask, **a2v)
        with pytest.raises(ValueError, match="jump"):
            fn(cfg=dict(cfg, sampling=dict(cfg["sampling"], resample={"jump": 2})), noise_seed=1, init_video=init, mask=mask, **a2v)
    with pytest.raises(ValueError, match="second broadcast"):                                      # shard with an init clip stays refused
        S.stream_generate(cfg=cfg, resample=(2, 2), noise_seed=1, init_video=vid, mask=mask_c, shard=True, **a2v)
