"""The FIFO clip batch without a GPU (include/avdiff_hip.h, "FIFO clip batch"): the torch statement of ``functional.fifo_shift_clips``
against the one-queue reference ``_slot_ref.shift`` on slices, with the entering tails handed in; the refusals of the function, of
``fifo_denoise_clips`` and of ``stream_generate`` with a list of prompt clips; ``fifo_geometry(clips=)``."""
import inspect
from types import SimpleNamespace

import pytest
import torch

import _slot_ref as SR
from _kit import STREAM_HALF_SECOND, pipeline_cfg

CASES = [((4, 8, 4, 16, 16), 2, 2), ((6, 8, 40), 4, 3)]      # (shape, slot_len, K)
SEEDS = [7, 2 ** 64 - 1, 7]                                  # a seed above 2^63 and a duplicate


def _inputs(shape, slot_len, K, n_clip=3):
    g = torch.Generator().manual_seed(len(shape))
    z, hist, carry = (torch.randn(shape, generator=g) for _ in range(3))
    tails = torch.randn((K, shape[1], slot_len) + tuple(shape[3:]), generator=g)
    clips = torch.full((K, shape[1], n_clip * slot_len) + tuple(shape[3:]), 7.0)
    return z, hist, carry, tails, clips


@pytest.mark.parametrize("riders", [0, 1, 2])
@pytest.mark.parametrize("shape,slot_len,K", CASES)
def test_statement_equals_one_queue_shifts_on_slices(shape, slot_len, K, riders):
    from multimodal_diffusion_amd import functional as Fn
    z, hist, carry, tails, clips = _inputs(shape, slot_len, K)
    Bq, m = shape[0] // K, 1
    kw = {}
    if riders >= 1:
        kw["hist"] = hist
    if riders == 2:
        kw["carry"], kw["carry_out"] = carry, torch.empty_like(carry)
    res = Fn.fifo_shift_clips(z, K, 11, SEEDS[:K], 999, slot_len, clips, m, tails=tails, **kw)
    outs = (res,) if riders == 0 else res
    assert len(outs) == 1 + riders and (riders < 2 or outs[2] is kw["carry_out"])
    zero = torch.zeros_like(tails[0])
    for k in range(K):
        sl = slice(k * Bq, (k + 1) * Bq)
        want, popped = SR.shift(z[sl], tails[k], slot_len)
        assert torch.equal(outs[0][sl], want)
        # the head of queue k lands in slot m of canvas k, and nowhere else
        assert torch.equal(clips[k, :, m * slot_len:(m + 1) * slot_len], popped)
        assert bool((clips[k, :, :m * slot_len] == 7.0).all()) and bool((clips[k, :, (m + 1) * slot_len:] == 7.0).all())
        for src, got in zip((hist, carry), outs[1:]):
            assert torch.equal(got[sl], SR.shift(src[sl], zero, slot_len)[0])      # the riders: the same map, zeros entering
    # the functional carry at ctx = 0, shift = 1 is the riders' map on a slice
    if riders:
        assert torch.equal(outs[1][:Bq], Fn.fifo_carry(hist[:Bq].contiguous(), shape[2] // slot_len, slot_len))


@pytest.mark.parametrize("shape,slot_len,K", CASES)
def test_a_head_outside_the_clip_is_written_nowhere(shape, slot_len, K):
    from multimodal_diffusion_amd import functional as Fn
    z, _, _, tails, clips = _inputs(shape, slot_len, K)
    ref = Fn.fifo_shift_clips(z, K, 0, SEEDS[:K], 0, slot_len, clips.clone(), 0, tails=tails)
    for m in (-1, 3):                                                             # n_clip = 3
        out = Fn.fifo_shift_clips(z, K, 0, SEEDS[:K], 0, slot_len, clips, m, tails=tails)
        assert bool((clips == 7.0).all()) and torch.equal(out, ref)               # the queues still shift


def test_function_refusals():
    from multimodal_diffusion_amd import functional as Fn
    z, hist, _, tails, clips = _inputs((4, 8, 4, 16, 16), 2, 2)
    ok = dict(z=z, queues=2, c=0, seeds=[1, 2], t=999, slot_len=2, clips=clips, m=0, tails=tails)
    assert Fn.fifo_shift_clips(**ok).shape == z.shape
    with pytest.raises(ValueError, match=r"queues 3 .*divides the batch 4"):
        Fn.fifo_shift_clips(**dict(ok, queues=3))
    with pytest.raises(ValueError, match=r"queues 0"):
        Fn.fifo_shift_clips(**dict(ok, queues=0))
    with pytest.raises(ValueError, match=r"3 seeds for 2 queues"):
        Fn.fifo_shift_clips(**dict(ok, seeds=[1, 2, 3]))
    for bad in ([1, 2 ** 64], [1, -1], [1, True], [1, 2.0]):
        with pytest.raises(ValueError, match="noise seed must be an int in"):
            Fn.fifo_shift_clips(**dict(ok, seeds=bad))
    for bad in (clips[:1], clips[:, :, :5], clips[:, :4], clips[:, :, :, :8], clips.double(), clips[0]):
        with pytest.raises(ValueError, match=r"clips must be a contiguous float32 \[2, 8, n_clip \* 2"):
            Fn.fifo_shift_clips(**dict(ok, clips=bad))
    with pytest.raises(ValueError, match="hist_out goes with hist"):
        Fn.fifo_shift_clips(**dict(ok, hist_out=hist))
    with pytest.raises(ValueError, match="carry_out goes with carry"):
        Fn.fifo_shift_clips(**dict(ok, carry_out=hist))
    with pytest.raises(ValueError, match="hist must be a contiguous float32 tensor of z's shape"):
        Fn.fifo_shift_clips(**dict(ok, hist=hist[:2]))
    with pytest.raises(ValueError, match="divides the sliding length"):
        Fn.fifo_shift_clips(**dict(ok, slot_len=3))
    with pytest.raises(ValueError, match=r"2\*\*32"):
        Fn.fifo_shift_clips(**dict(ok, c=2 ** 31))
    with pytest.raises(ValueError, match="tails must be the entering slots"):
        Fn.fifo_shift_clips(**dict(ok, tails=tails[:1]))
    # the seeds as the launch takes them: the same 64 bits, signed
    assert Fn.clip_seeds([0, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1], 4).tolist() == [0, 2 ** 63 - 1, -2 ** 63, -1]


# ------------------------------------------------------------------------------------------------- fifo_denoise_clips
def _bare_engine(B=4, eta=0.0, clip=None):
    """an engine shell with the attributes the driver's refusals read: a video queue of S = 2 slots of 2 positions"""
    import multimodal_diffusion_amd as A
    eng = object.__new__(A.DenoiseEngine)
    eng.latent_shape, eng.device, eng.target, eng.tube, eng.chunk = (B, 8, 4, 16, 16), torch.device("cpu"), "video", (2, 4, 4), (4, 4)
    eng.eta, eng._clip, eng.solver, eng.embed = eta, clip, "ddim", SimpleNamespace(B=B, Np=10)
    return eng


def test_driver_refusals():
    import multimodal_diffusion_amd as A
    sched = torch.tensor([999, 749, 499, 249, -1])
    pcs = [torch.zeros(8, 150), torch.zeros(8, 150)]
    with pytest.raises(ValueError, match=r"eta == 0 \(the engine has eta = 0\.5\).*same step normals"):
        A.fifo_denoise_clips(_bare_engine(eta=0.5), pcs, 20, sched, 3, [1, 2])
    with pytest.raises(ValueError, match=r"fifo_denoise_clips takes no clip guide"):
        A.fifo_denoise_clips(_bare_engine(clip=(None, None, 0)), pcs, 20, sched, 3, [1, 2])
    # K = 2 in a batch of 4 with S = 2 is B_q * S = 4 = n; three steps, a batch of 6, or K = 3 do not fit
    with pytest.raises(ValueError, match=r"K = 2 clips .*B = 4 .*S = 2 .*n = 2 steps"):
        A.fifo_denoise_clips(_bare_engine(), pcs, 20, torch.tensor([999, 499, -1]), 3, [1, 2])
    with pytest.raises(ValueError, match=r"K = 2 clips .*B = 6 .*S = 2 .*n = 4 steps"):
        A.fifo_denoise_clips(_bare_engine(B=6), pcs, 20, sched, 3, [1, 2])
    with pytest.raises(ValueError, match=r"K = 3 clips .*B = 4"):
        A.fifo_denoise_clips(_bare_engine(), pcs + pcs[:1], 20, sched, 3, [1, 2, 3])
    with pytest.raises(ValueError, match="K = 0"):
        A.fifo_denoise_clips(_bare_engine(), [], 20, sched, 3, [])
    with pytest.raises(ValueError, match="one shape"):
        A.fifo_denoise_clips(_bare_engine(), [pcs[0], torch.zeros(8, 151)], 20, sched, 3, [1, 2])
    with pytest.raises(ValueError, match=r"1 seeds for 2 queues"):
        A.fifo_denoise_clips(_bare_engine(), pcs, 20, sched, 3, [1])
    with pytest.raises(ValueError, match="n_slots"):
        A.fifo_denoise_clips(_bare_engine(), pcs, 20, sched, 0, [1, 2])
    with pytest.raises(TypeError, match="DenoiseEngine"):
        A.fifo_denoise_clips(object(), pcs, 20, sched, 3, [1, 2])
    # the single-queue options are not arguments here, and fifo_denoise keeps them
    params = inspect.signature(A.fifo_denoise_clips).parameters
    assert not {"graph", "lookahead", "context", "init_canvas", "mask"} & set(params)
    assert list(params)[:6] == ["engine", "prompt_canvases", "prompt_hop", "sched", "n_slots", "noise_seeds"]
    assert {"graph", "lookahead", "context", "init_canvas"} <= set(inspect.signature(A.fifo_denoise).parameters)


# ------------------------------------------------------------------------------------------------- the pipeline
def _cfg(**sampling):
    return pipeline_cfg(clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND, sampling=sampling or None)


def _generate(cfg, **kw):
    """stream_generate(sampler="fifo") with two prompt clips and no modules: a refusal comes before anything is read"""
    from multimodal_diffusion_amd import stream_infer as S
    wav = torch.zeros(18000).numpy()
    args = dict(cfg=cfg, vid_vae=None, aud_codec=None, adapt_v=None, adapt_a=None, core=None, head=None, tstep_dim=256,
                prompt_modality="audio", prompt_video=None, prompt_audio=[wav, wav], device=torch.device("cpu"), sampler="fifo")
    return S.stream_generate(**dict(args, **kw))


def test_pipeline_refusals_of_a_clip_list():
    import numpy as np
    from multimodal_diffusion_amd import stream_infer as S
    vid = np.zeros((20, 32, 32, 3), dtype=np.uint8)
    with pytest.raises(ValueError, match="list of prompt clips takes no init clip or mask"):
        _generate(_cfg(), init_video=vid)
    with pytest.raises(ValueError, match="list of prompt clips takes no init clip or mask"):
        _generate(_cfg(), init_video=vid, mask=torch.ones(1))
    with pytest.raises(ValueError, match=r"list of prompt clips needs sampling.ddim_eta == 0 \(got 0\.5\)"):
        _generate(_cfg(ddim_eta=0.5), noise_seed=3)
    with pytest.raises(ValueError, match=r"fifo\['graph'\] True is refused"):
        _generate(_cfg(), fifo={"graph": True})
    with pytest.raises(ValueError, match=r"fifo\['lookahead'\] 1 is refused"):
        _generate(_cfg(), fifo={"lookahead": 1})
    with pytest.raises(ValueError, match="at least one clip"):
        _generate(_cfg(), prompt_audio=[])
    # the helper alone, on _fifo_options' result
    kw = dict(shard=False, consensus=None, noise_keying=None, resample=None, init_noise=None)
    opts = S._fifo_options(_cfg(), fifo=None, **kw)
    assert S._fifo_clips_refusals(_cfg(), opts, 2, False, False) is None
    assert S._fifo_clips_refusals(_cfg(), S._fifo_options(_cfg(), fifo={"graph": None}, **kw), 2, False, False) is None
    with pytest.raises(ValueError, match="lookahead"):
        S._fifo_clips_refusals(_cfg(), S._fifo_options(_cfg(), fifo={"lookahead": 2}, **kw), 2, False, False)
    with pytest.raises(ValueError, match="init clip or mask"):
        S._fifo_clips_refusals(_cfg(), opts, 2, False, True)


def test_geometry_reports_the_clip_batch():
    from multimodal_diffusion_amd.stream_infer import FifoGeometry, fifo_geometry
    cfg = pipeline_cfg(clip_seconds=1.0, sampler_steps=4, streaming={"window_seconds": 1.0, "hop_seconds": 0.5, "crossfade_seconds": 0.25})
    one = fifo_geometry(cfg, "audio", 4, 4)
    three = fifo_geometry(cfg, "audio", 4, 4, clips=3)
    assert (one.B, one.clips, three.B, three.clips) == (2, 1, 6, 3)
    assert isinstance(three, FifoGeometry) and three._replace(B=one.B) == one      # every other number is one clip's
    assert fifo_geometry(cfg, "audio", 4, 4, clips=1) == one and type(fifo_geometry(cfg, "audio", 4, 4, clips=1)) is FifoGeometry
    assert inspect.signature(fifo_geometry).parameters["clips"].default == 1
    for bad in (0, -1, True, 2.0):
        with pytest.raises(ValueError, match="clips must be an int >= 1"):
            fifo_geometry(cfg, "audio", 4, 4, clips=bad)
