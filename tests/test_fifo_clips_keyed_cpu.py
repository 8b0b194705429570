"""Clip batch keying without a GPU (include/avdiff_hip.h, "clip batch keying"): the torch statements of ``functional.slot_noise_clips``
and ``functional.clip_guide_slots_clips`` against the one-queue functions on slices (stand-ins that are pure functions of their
arguments take the one-queue functions' place: those launch on a device), the argument refusals of the functions, of
``fifo_denoise_clips`` and of the pipeline, and the new entries in the header, the binding and the library."""
import inspect
import re
from pathlib import Path
from types import SimpleNamespace

import pytest
import torch

from _kit import STREAM_HALF_SECOND, pipeline_cfg

ROOT = Path(__file__).resolve().parent.parent
NEW = ("avd_slot_noise_clips_f32", "avd_clip_guide_slots_clips_f32", "avd_cfg_unpatch_ddim_slots_clips_f32",
       "avd_cfg_untoken_ddim_audio_slots_clips_f32", "avd_denoise_step_slots_clips_f32")
CASES = [((4, 8, 4, 16, 16), 2, 2), ((6, 8, 8), 4, 3)]      # (shape, slot_len, K)
SEEDS = [7, 2 ** 64 - 1, 7]                                 # a seed above 2^63 and a duplicate


def test_entries_are_declared_bound_and_exported():
    from multimodal_diffusion_amd import _lib as L
    hdr = (ROOT / "include" / "avdiff_hip.h").read_text()
    lib = L.lib()
    for name in NEW:
        assert re.search(rf"\bint {name}\(", hdr) and name in L.SIGNATURES and hasattr(lib, name)
    assert lib.avd_abi_version() == L.ABI_VERSION == 7           # an addition: the ABI stays
    assert "} avd_clip_queues;" in hdr and "clip batch keying" in hdr
    assert [f[0] for f in L.ClipQueues._fields_] == ["K", "step_seeds", "guide_seeds"]
    # the existing entries keep their signatures
    for name in ("avd_slot_noise_f32", "avd_clip_guide_slots_f32", "avd_cfg_unpatch_ddim_slots_cfg_f32", "avd_denoise_step_slots_cfg_f32"):
        assert "ClipQueues" not in repr(L.SIGNATURES[name])


# ------------------------------------------------------------------------------------------------- the torch statements
def _noise_stub(seed, t_now, shape, slot_len, first=0, stride=None, cursor=None, out=None):
    """a pure function of the one-queue arguments, with the sample index in it: a slice handed in under a wrong seed, origin or stride
    cannot give the same values"""
    B, S = t_now.shape
    b = torch.arange(B).view((B,) + (1,) * (len(shape) - 1)).float()
    pos = (first + b * (S if stride is None else stride)) * slot_len + torch.arange(shape[2]).view((1, 1, -1) + (1,) * (len(shape) - 3))
    t = t_now.float().repeat_interleave(slot_len, 1).view((B, 1, -1) + (1,) * (len(shape) - 3))
    return ((seed % 1000) + pos * 3.0 + t / 7.0).expand(shape).clone()


def _guide_stub(known, tau, alpha_bar, z, mask=None, *, slot_len, seed, first=0, stride=None, cursor=None, everywhere=False, out=None):
    B, S = tau.shape
    lead = _noise_stub(seed, tau.clamp(min=0), tuple(z.shape), slot_len, first, stride)
    m = 1.0 if mask is None or everywhere else mask.mean()
    res = z + m * lead + known.sum()
    leave = (tau == -2 ** 63).repeat_interleave(slot_len, 1).view((B, 1, -1) + (1,) * (z.dim() - 3)).expand(z.shape)
    return torch.where(leave, z, res)


@pytest.mark.parametrize("shape,slot_len,K", CASES)
def test_slot_noise_statement_is_the_one_queue_function_on_slices(monkeypatch, shape, slot_len, K):
    from multimodal_diffusion_amd import functional as Fn
    monkeypatch.setattr(Fn, "slot_noise", _noise_stub)
    B, S = shape[0], shape[2] // slot_len
    Bq = B // K
    tn = torch.arange(B * S).view(B, S) * 10
    for first, stride in ((0, None), (-2, 3)):
        got = Fn.slot_noise_clips(SEEDS[:K], tn, shape, slot_len, first=first, stride=stride, out=torch.empty(shape))
        for k in range(K):
            q = slice(k * Bq, (k + 1) * Bq)
            assert torch.equal(got[q], _noise_stub(SEEDS[k], tn[q], (Bq,) + shape[1:], slot_len, first, stride))
        # the walk restarts in every queue: equal seeds and equal tables give equal queues
        same = Fn.slot_noise_clips([5] * K, tn[:Bq].repeat(K, 1), shape, slot_len, first=first, stride=stride, out=torch.empty(shape))
        assert all(torch.equal(same[:Bq], same[k * Bq:(k + 1) * Bq]) for k in range(K))
    with pytest.raises(ValueError, match="queues must divide the batch"):
        Fn.slot_noise_clips([1] * (B - 1), tn, shape, slot_len, out=torch.empty(shape))
    for bad in ([1, 2 ** 64][:K] + [1] * (K - 2), [1, -1] + [1] * (K - 2), [1, True] + [1] * (K - 2), [1, 2.0] + [1] * (K - 2)):
        with pytest.raises(ValueError, match="noise seed must be an int in"):
            Fn.slot_noise_clips(bad, tn, shape, slot_len, out=torch.empty(shape))
    with pytest.raises(ValueError, match="sequence of ints"):
        Fn.slot_noise_clips(3, tn, shape, slot_len, out=torch.empty(shape))
    with pytest.raises(ValueError, match="out must be a float32 tensor of shape"):
        Fn.slot_noise_clips(SEEDS[:K], tn, shape, slot_len, out=torch.empty(shape[:-1]))


@pytest.mark.parametrize("shape,slot_len,K", CASES)
def test_clip_guide_statement_is_the_one_queue_function_on_slices(monkeypatch, shape, slot_len, K):
    from multimodal_diffusion_amd import functional as Fn
    monkeypatch.setattr(Fn, "clip_guide_slots", _guide_stub)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)      # the statement keeps the slices where they are
    B, S = shape[0], shape[2] // slot_len
    Bq = B // K
    g = torch.Generator().manual_seed(K)
    z = torch.randn(shape, generator=g)
    known = torch.randn((K, shape[1], 11) + shape[3:], generator=g)
    masks = torch.rand(known.shape, generator=g)
    tau = torch.arange(B * S).view(B, S) * 10
    ab = torch.linspace(0.99, 0.01, 1000)
    for m, everywhere in ((masks, False), (None, False), (masks, True)):
        kw = dict(slot_len=slot_len, first=3, stride=None, everywhere=everywhere)
        got = Fn.clip_guide_slots_clips(known, tau, ab, z, m, seeds=SEEDS[:K], **kw)
        for k in range(K):
            q = slice(k * Bq, (k + 1) * Bq)
            assert torch.equal(got[q], _guide_stub(known[k], tau[q], ab, z[q], None if m is None else m[k], seed=SEEDS[k], **kw))
    # a list of canvases is the stacked tensor; the in-place call over the K tails touches nothing else
    tails = torch.full((B, S), Fn.SLOT_LEAVE, dtype=torch.long)
    tails[Bq - 1::Bq, S - 1] = 999
    ip = z.clone()
    assert Fn.clip_guide_slots_clips(list(known.unbind(0)), tails, ab, ip, masks, slot_len=slot_len, seeds=SEEDS[:K], out=ip) is ip
    touched = torch.zeros(B, shape[2], dtype=torch.bool)
    touched[Bq - 1::Bq, (S - 1) * slot_len:] = True
    assert torch.equal(ip.movedim(2, 1)[~touched], z.movedim(2, 1)[~touched]) and not torch.equal(ip.movedim(2, 1)[touched], z.movedim(2, 1)[touched])
    # refusals
    with pytest.raises(ValueError, match=rf"{K + 1} seeds for {K} queues"):
        Fn.clip_guide_slots_clips(known, tau, ab, z, seeds=SEEDS[:K] + [1], slot_len=slot_len)
    with pytest.raises(ValueError, match="one shape"):
        Fn.clip_guide_slots_clips([known[0], known[1][:, :5]], tau, ab, z, seeds=SEEDS[:2], slot_len=slot_len)
    with pytest.raises(ValueError, match="masks shape"):
        Fn.clip_guide_slots_clips(known, tau, ab, z, masks[:, :, :5], seeds=SEEDS[:K], slot_len=slot_len)
    with pytest.raises(ValueError, match="queues must divide the batch"):
        Fn.clip_guide_slots_clips(known, tau[:B - 1], ab, z[:B - 1], seeds=SEEDS[:K], slot_len=slot_len)
    with pytest.raises(ValueError, match="canvases' rank"):
        Fn.clip_guide_slots_clips(known, tau, ab, z[0], seeds=SEEDS[:K], slot_len=slot_len)


def test_seed_and_descriptor_helpers():
    from multimodal_diffusion_amd import functional as Fn
    assert Fn.queue_seeds([0, 2 ** 63, 2 ** 64 - 1]).tolist() == [0, -2 ** 63, -1]
    t = Fn.clip_seeds([1, 2], 2)
    assert Fn.queue_seeds(t, 2) is t
    for bad in (t.to(torch.int32), t.view(1, 2), torch.zeros(0, dtype=torch.int64)):
        with pytest.raises(ValueError, match="seeds tensor must be"):
            Fn.queue_seeds(bad)
    with pytest.raises(ValueError, match="seeds tensor must be"):
        Fn.queue_seeds(t, 3)
    for bad in (0, True, 3):
        with pytest.raises(ValueError, match="divides the batch 4"):
            Fn.clip_queues(bad, 4)
    with pytest.raises(ValueError, match="step_seeds must be"):
        Fn.clip_queues(2, 4, step_seeds=t)                       # a CPU tensor: the kernels read the seeds on the device
    cq = Fn.clip_queues(2, 4)
    assert (cq.K, cq.step_seeds, cq.guide_seeds) == (2, None, None)


# ------------------------------------------------------------------------------------------------- fifo_denoise_clips
def _bare_engine(B=4, eta=0.0, clip=None):
    """test_fifo_clips_cpu.py's engine shell: a video queue of S = 2 slots of 2 positions"""
    import multimodal_diffusion_amd as A
    eng = object.__new__(A.DenoiseEngine)
    eng.latent_shape, eng.device, eng.target, eng.tube, eng.chunk = (B, 8, 4, 16, 16), torch.device("cpu"), "video", (2, 4, 4), (4, 4)
    eng.eta, eng._clip, eng.solver, eng.embed = eta, clip, "ddim", SimpleNamespace(B=B, Np=10)
    return eng


def test_driver_arguments():
    import multimodal_diffusion_amd as A
    sched = torch.tensor([999, 749, 499, 249, -1])
    short = torch.tensor([999, 499, -1])      # the batch check comes behind every argument check: reaching it is passing them
    pcs = [torch.zeros(8, 150), torch.zeros(8, 150)]
    canv = [torch.zeros(8, 6, 16, 16), torch.zeros(8, 6, 16, 16)]
    past = r"K = 2 clips .*B = 4 .*S = 2 .*n = 2 steps"
    params = list(inspect.signature(A.fifo_denoise_clips).parameters)
    assert params[-5:] == ["step_seeds", "init_canvases", "masks", "guide_seeds", "guide_start"]
    # an eta > 0 engine: refused without step seeds, past the eta refusal with them
    with pytest.raises(ValueError, match=r"eta == 0 \(the engine has eta = 0\.5\).*same step normals.*step_seeds"):
        A.fifo_denoise_clips(_bare_engine(eta=0.5), pcs, 20, sched, 3, [1, 2])
    with pytest.raises(ValueError, match=past):
        A.fifo_denoise_clips(_bare_engine(eta=0.5), pcs, 20, short, 3, [1, 2], step_seeds=[1, 2])
    # step seeds on an eta == 0 engine are checked and otherwise ignored
    with pytest.raises(ValueError, match=past):
        A.fifo_denoise_clips(_bare_engine(), pcs, 20, short, 3, [1, 2], step_seeds=[1, 2])
    with pytest.raises(ValueError, match=r"1 seeds for 2 queues"):
        A.fifo_denoise_clips(_bare_engine(), pcs, 20, sched, 3, [1, 2], step_seeds=[1])
    for bad in ([1, 2 ** 64], [1, -1], [1, True], [1, 2.0]):
        with pytest.raises(ValueError, match="noise seed must be an int in"):
            A.fifo_denoise_clips(_bare_engine(eta=0.5), pcs, 20, sched, 3, [1, 2], step_seeds=bad)
    with pytest.raises(ValueError, match="sequence of 2 ints"):
        A.fifo_denoise_clips(_bare_engine(eta=0.5), pcs, 20, sched, 3, [1, 2], step_seeds=torch.tensor([1, 2]))
    # the guides
    with pytest.raises(ValueError, match=past):
        A.fifo_denoise_clips(_bare_engine(), pcs, 20, short, 3, [1, 2], init_canvases=canv, masks=[torch.ones(1)] * 2, guide_seeds=[3, 4],
                             guide_start="init")
    with pytest.raises(ValueError, match=past):
        A.fifo_denoise_clips(_bare_engine(), pcs, 20, short, 3, [1, 2], init_canvases=torch.stack(canv))      # guide_seeds: K zeros
    with pytest.raises(ValueError, match="one shape"):
        A.fifo_denoise_clips(_bare_engine(), pcs, 20, sched, 3, [1, 2], init_canvases=[canv[0], canv[1][:, :4]])
    with pytest.raises(ValueError, match="3 init canvases for 2 clips"):
        A.fifo_denoise_clips(_bare_engine(), pcs, 20, sched, 3, [1, 2], init_canvases=canv + canv[:1])
    with pytest.raises(ValueError, match="1 masks for 2 clips"):
        A.fifo_denoise_clips(_bare_engine(), pcs, 20, sched, 3, [1, 2], init_canvases=canv, masks=[torch.ones(1)])
    with pytest.raises(ValueError, match=r"3 seeds for 2 queues"):
        A.fifo_denoise_clips(_bare_engine(), pcs, 20, sched, 3, [1, 2], init_canvases=canv, guide_seeds=[1, 2, 3])
    for kw in (dict(masks=[torch.ones(1)] * 2), dict(guide_seeds=[1, 2]), dict(guide_start="init")):
        with pytest.raises(ValueError, match="belong to the clip guides: pass init_canvases"):
            A.fifo_denoise_clips(_bare_engine(), pcs, 20, sched, 3, [1, 2], **kw)
    with pytest.raises(ValueError, match="guide_start must be 'noise' or 'init'"):
        A.fifo_denoise_clips(_bare_engine(), pcs, 20, sched, 3, [1, 2], init_canvases=canv, guide_start="known")
    # the engine's own guides stay refused
    with pytest.raises(ValueError, match=r"fifo_denoise_clips takes no clip guide"):
        A.fifo_denoise_clips(_bare_engine(clip=(None, None, 0)), pcs, 20, sched, 3, [1, 2], init_canvases=canv)
    eng = _bare_engine()
    eng._clips = (None, None, None)
    with pytest.raises(ValueError, match="clear_clip_guides"):
        A.fifo_denoise_clips(eng, pcs, 20, sched, 3, [1, 2])


def test_engine_refusals_of_the_k_guide_state():
    eng = _bare_engine()
    assert eng._clips is None
    eng._clips = (torch.zeros(2, 8, 6, 16, 16), None, None)
    for what in ("step", "run", "fifo_open", "fifo_lookahead"):
        with pytest.raises(ValueError, match=f"{what} takes no clip guides"):
            eng._clips_refusal(what)
    eng.clear_clip_guides()
    assert eng._clips is None and eng._clips_refusal("step") is None
    # the sources call it where they call the one-canvas refusal
    src = inspect.getsource(type(eng))
    for what in ("step", "run", "fifo_open", "fifo_lookahead"):
        assert f'self._clips_refusal("{what}")' in src


# ------------------------------------------------------------------------------------------------- the pipeline
def test_pipeline_admits_a_noise_seed_list():
    from multimodal_diffusion_amd import stream_infer as S
    cfg = pipeline_cfg(clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND, sampling={"ddim_eta": 0.5})
    kw = dict(shard=False, consensus=None, noise_keying=None, resample=None, init_noise=None)
    opts = S._fifo_options(cfg, fifo=None, **kw)
    assert S._fifo_clips_refusals(cfg, opts, 2, False, False, [3, 4]) is None
    assert S._fifo_clips_refusals(cfg, opts, 2, False, False, (3, 3)) is None
    for seed in (3, None):
        with pytest.raises(ValueError, match=r"list of prompt clips needs sampling.ddim_eta == 0 \(got 0\.5\)"):
            S._fifo_clips_refusals(cfg, opts, 2, False, False, seed)
    with pytest.raises(ValueError, match=r"1 seeds for 2 queues"):
        S._fifo_clips_refusals(cfg, opts, 2, False, False, [3])
    with pytest.raises(ValueError, match="noise seed must be an int in"):
        S._fifo_clips_refusals(cfg, opts, 2, False, False, [3, -1])
    with pytest.raises(ValueError, match="init clip or mask"):
        S._fifo_clips_refusals(cfg, opts, 2, True, False, [3, 4])
    # at eta == 0 a list is checked the same way and changes nothing else
    cfg0 = pipeline_cfg(clip_seconds=0.5, sampler_steps=4, streaming=STREAM_HALF_SECOND)
    assert S._fifo_clips_refusals(cfg0, S._fifo_options(cfg0, fifo=None, **kw), 2, False, False, [3, 4]) is None
