"""The FIFO clip batch on the GPU (include/avdiff_hip.h, "FIFO clip batch"): the multi-queue shift kernel against the existing
one-queue entries on slices, ``fifo_denoise_clips`` against a loop written here from existing parts, the clips' independence, K = 1
against ``fifo_denoise``, the slot control with its momentum, and one pipeline call with two prompt clips.  Every comparison holds the
batch fixed and is bit for bit: equal bits across batch sizes are no contract (the GEMM dispatch may pick a kernel by row count)."""
import ctypes as C

import numpy as np
import pytest
import torch

from _kit import audio_prompt, components, dev, engine, model, pipeline  # noqa: F401  (dev, model are fixtures)

pytestmark = pytest.mark.gpu

GS = 3.5
SEEDS = [0x5EED0F1F0, 2 ** 64 - 3, 11]
SCHED4 = [999, 749, 499, 249, -1]


# ------------------------------------------------------------------------------------------------- the kernel
def _reference(z, K, c, seeds, t, slot_len, clips, m, hist, carry):
    """K one-queue shifts (with the history) and K carries on slices, plus the copies of the popped heads"""
    from multimodal_diffusion_amd import functional as Fn
    Bq, S = z.shape[0] // K, z.shape[2] // slot_len
    out, h_out, c_out = torch.empty_like(z), torch.empty_like(z), torch.empty_like(z)
    for k in range(K):
        sl = slice(k * Bq, (k + 1) * Bq)
        if hist is None:
            out[sl], popped = Fn.fifo_shift(z[sl], c, seeds[k], t, slot_len)
        else:
            out[sl], popped, h_out[sl] = Fn.fifo_shift(z[sl], c, seeds[k], t, slot_len, hist=hist[sl].contiguous())
        if carry is not None:
            c_out[sl] = Fn.fifo_carry(carry[sl], S, slot_len)
        if 0 <= m < clips.shape[2] // slot_len:
            clips[k, :, m * slot_len:(m + 1) * slot_len] = popped
    return out, h_out, c_out


@pytest.mark.parametrize("riders", [0, 1, 2])
# the last two are K queues of one window of one slot each (Bq = 1, S = 1): every queue's only slot is its head and its tail
@pytest.mark.parametrize("shape,slot_len,K", [((4, 8, 4, 16, 16), 2, 2), ((6, 8, 40), 4, 3), ((3, 8, 4, 16, 16), 1, 3),
                                              ((2, 1, 1, 2, 2), 1, 2), ((2, 2, 4), 4, 2)])
def test_kernel_equals_the_one_queue_entries_on_slices(dev, shape, slot_len, K, riders):
    from multimodal_diffusion_amd import _lib as L
    from multimodal_diffusion_amd import functional as Fn
    g = torch.Generator().manual_seed(len(shape) + K)
    z, hist, carry = (torch.randn(shape, generator=g).to(dev) for _ in range(3))
    hist, carry = (hist if riders >= 1 else None), (carry if riders == 2 else None)
    c, t, m, n_clip = 11, 999, 2, 4
    canvas = (K, shape[1], n_clip * slot_len) + tuple(shape[3:])
    want_clips = torch.full(canvas, 7.0, device=dev)
    want = _reference(z, K, c, SEEDS[:K], t, slot_len, want_clips, m, hist, carry)

    def run(z_, clips, m_=m, hist_=hist, carry_=carry):
        res = Fn.fifo_shift_clips(z_, K, c, SEEDS[:K], t, slot_len, clips, m_, hist=hist_, carry=carry_)
        return (res,) if riders == 0 else res

    clips = torch.full(canvas, 7.0, device=dev)
    got = run(z, clips)
    assert len(got) == 1 + riders
    for a, b in zip(got, (want[0],) + ((want[1],) if riders else ()) + ((want[2],) if riders == 2 else ())):
        assert torch.equal(a, b)
    assert torch.equal(clips, want_clips) and not bool((clips[:, :, m * slot_len:(m + 1) * slot_len] == 7.0).all())
    # the torch statement on CPU tensors, drawing its own tails, is the same map
    cpu_clips = torch.full(canvas, 7.0)
    cpu = Fn.fifo_shift_clips(z.cpu(), K, c, SEEDS[:K], t, slot_len, cpu_clips, m, hist=None if hist is None else hist.cpu(),
                              carry=None if carry is None else carry.cpu())
    assert all(torch.equal(a.cpu(), b) for a, b in zip(got, (cpu,) if riders == 0 else cpu)) and torch.equal(clips.cpu(), cpu_clips)
    # a head outside the clip is written nowhere; the queues still shift
    for bad in (-1, n_clip):
        clips2 = torch.full(canvas, 7.0, device=dev)
        assert torch.equal(run(z, clips2, bad)[0], want[0]) and bool((clips2 == 7.0).all())
    # a view misaligned by one float takes the one-element lanes: the same bits
    if len(shape) == 5:
        zu = torch.empty(z.numel() + 1, device=dev)[1:].view(shape).copy_(z)
        assert zu.data_ptr() % 16 != 0
        clips3 = torch.full(canvas, 7.0, device=dev)
        got3 = run(zu, clips3)
        assert all(torch.equal(a, b) for a, b in zip(got3, got)) and torch.equal(clips3, want_clips)
        if riders:                                          # a misaligned rider alone does the same
            hu = torch.empty(z.numel() + 1, device=dev)[1:].view(shape).copy_(hist)
            clips4 = torch.full(canvas, 7.0, device=dev)
            got4 = run(z, clips4, hist_=hu)
            assert all(torch.equal(a, b) for a, b in zip(got4, got)) and torch.equal(clips4, want_clips)
    # K = 1 on the first queue: the bits of avd_fifo_shift_f32 / _hist_f32
    Bq = shape[0] // K
    one = torch.full(canvas[:0] + (1,) + canvas[1:], 7.0, device=dev)
    res = Fn.fifo_shift_clips(z[:Bq], 1, c, SEEDS[:1], t, slot_len, one, m, hist=None if hist is None else hist[:Bq].contiguous())
    single = Fn.fifo_shift(z[:Bq], c, SEEDS[0], t, slot_len, hist=None if hist is None else hist[:Bq].contiguous())
    assert torch.equal(res if hist is None else res[0], single[0]) and torch.equal(one[0, :, m * slot_len:(m + 1) * slot_len], single[1])
    if hist is not None:
        assert torch.equal(res[1], single[2])
    # the library's own refusals (AVD_EINVAL -> ValueError): overlapping buffers, a null canvas
    sd = Fn.clip_seeds(SEEDS[:K], K, dev)
    S_, inner = shape[2] // slot_len, (shape[3] * shape[4] if len(shape) == 5 else 1)
    args = lambda zo, cl: (sd.data_ptr(), t, c, z.data_ptr(), zo, cl, n_clip, m, None, None, None, None, shape[0], K, shape[1], S_,  # noqa: E731
                           slot_len, inner, L.stream_ptr(dev))
    out = torch.empty_like(z)
    for bad in (args(z.data_ptr(), clips.data_ptr()), args(out.data_ptr(), out.data_ptr()), args(out.data_ptr(), None)):
        with pytest.raises(ValueError, match="fifo_shift"):
            L.check(L.lib().avd_fifo_shift_clips_f32(*bad))
    with pytest.raises(ValueError, match="queues must divide the batch"):
        L.check(L.lib().avd_fifo_shift_clips_f32(*(args(out.data_ptr(), clips.data_ptr())[:13] + (shape[0] + 1,) +
                                                   args(out.data_ptr(), clips.data_ptr())[14:])))


# ------------------------------------------------------------------------------------------------- the driver
def _setup(dev, mods, target, K, Bq, **kw):
    """(engine of batch K * Bq, K prompt canvases, prompt_hop): the small queues of test_gpu_fifo.py.  Video [B, 8, 4, 16, 16], tube
    2 x 4 x 4 (S = 2), audio prompts of 20 frames per target slot; audio [B, 8, 8], chunk 4 / 4 (S = 2), video prompts of 2 frames per
    slot"""
    g = torch.Generator().manual_seed(17)
    if target == "video":
        eng = engine(mods, "video", (K * Bq, 8, 4, 16, 16), 10, guidance=GS, **kw)
        return eng, [torch.randn(8, 150, generator=g).to(dev) for _ in range(K)], 20
    eng = engine(mods, "audio", (K * Bq, 8, 8), 8, guidance=GS, **kw)
    return eng, [torch.randn(8, 14, 8, 8, generator=g).to(dev) for _ in range(K)], 2


def _loop(eng, canvases_p, hop, sched, n_out, seeds, momentum=False):
    """fifo_denoise_clips restated from existing parts: fifo_plan's tables tiled, set_prompt of the concatenated
    fifo_prompt_windows, step_slots on the whole batch, K one-queue shifts (and K carries) on slices.  Returns (canvases, the slot
    momentum buffer or None)."""
    from multimodal_diffusion_amd import functional as Fn, schedule_utils as su
    from multimodal_diffusion_amd.stream_infer import fifo_prompt_len, fifo_prompt_windows
    K, B, S, sl = len(canvases_p), eng.embed.B, eng.slots, eng.slot_len
    Bq = B // K
    sched = torch.tensor(sched)
    multistep = eng.solver == "dpmpp_2m"
    tile = lambda t: t.repeat((1,) * (t.dim() - 2) + (K, 1))      # noqa: E731
    rn, rp, sn, sp = (tile(t) for t in su.fifo_plan(sched, S))
    rl, sl_last = (tile(t) for t in su.fifo_plan_last(sched, S)) if multistep else (None, None)
    n, s0, L_ = Bq * S, int(sched[0]), eng.latent_shape[2]
    Lp = fifo_prompt_len(eng, canvases_p[0])
    prompt = lambda m: torch.cat([fifo_prompt_windows(p, m, Bq, S, hop, Lp) for p in canvases_p], 0)      # noqa: E731
    z = torch.cat([Fn.canvas_noise(s, torch.full((Bq,), s0), (Bq,) + tuple(eng.latent_shape[1:]), L_) for s in seeds], 0)
    eng.set_prompt(prompt(0))
    for r in range(n - 1):
        z = eng.step_slots(z, rn[r], rp[r], t_last=rl[r] if multistep else None)
    done = []
    for m in range(n_out):
        eng.set_prompt(prompt(m))
        z = eng.step_slots(z, sn, sp, t_last=sl_last)
        nz, heads = torch.empty_like(z), []
        nh = torch.empty_like(z) if multistep else None
        for k in range(K):
            q = slice(k * Bq, (k + 1) * Bq)
            if multistep:
                nz[q], popped, nh[q] = Fn.fifo_shift(z[q], n + m, seeds[k], s0, sl, hist=eng.x0_hist[q].contiguous())
            else:
                nz[q], popped = Fn.fifo_shift(z[q], n + m, seeds[k], s0, sl)
            heads.append(popped)
            if momentum:
                eng.slot_momentum[q] = Fn.fifo_carry(eng.slot_momentum[q].contiguous(), S, sl)
        if multistep:
            eng.x0_hist.copy_(nh)
        z = nz
        done.append(torch.stack(heads, 0))
    mom = eng.slot_momentum.clone() if momentum else None
    return torch.cat(done, 2), mom


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("target,K,sched", [("video", 2, SCHED4), ("audio", 2, SCHED4), ("video", 3, [999, 499, -1])])
def test_driver_equals_the_loop_of_existing_parts(dev, model, target, K, sched, solver):
    import multimodal_diffusion_amd as A
    eng, pcs, hop = _setup(dev, model[1], target, K, (len(sched) - 1) // 2, solver=solver)
    out = A.fifo_denoise_clips(eng, pcs, hop, torch.tensor(sched), 3, SEEDS[:K])
    ref, _ = _loop(eng, pcs, hop, sched, 3, SEEDS[:K])
    assert out.shape == (K, 8, 3 * eng.slot_len) + tuple(eng.latent_shape[3:]) and torch.isfinite(out).all()
    assert torch.equal(out, ref), float((out - ref).abs().max())
    assert float(out.std()) > 0 and not torch.equal(out[0], out[1])
    # a stacked tensor of canvases is the list
    assert torch.equal(A.fifo_denoise_clips(eng, torch.stack(pcs), hop, torch.tensor(sched), 3, SEEDS[:K]), out)


@pytest.mark.parametrize("target", ["video", "audio"])
def test_a_clip_does_not_depend_on_its_neighbour(dev, model, target):
    import multimodal_diffusion_amd as A
    eng, pcs, hop = _setup(dev, model[1], target, 2, 2)
    sched = torch.tensor(SCHED4)
    a = A.fifo_denoise_clips(eng, pcs, hop, sched, 3, SEEDS[:2])
    b = A.fifo_denoise_clips(eng, [pcs[0], torch.flip(pcs[1], (1,)) * 0.5], hop, sched, 3, [SEEDS[0], 99])
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])
    # equal seeds and equal prompts are equal clips (correlated starts)
    c = A.fifo_denoise_clips(eng, [pcs[0], pcs[0]], hop, sched, 3, [SEEDS[0], SEEDS[0]])
    assert torch.equal(c[0], c[1]) and torch.equal(c[0], a[0])


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("target", ["video", "audio"])
def test_one_clip_is_fifo_denoise(dev, model, target, solver):
    import multimodal_diffusion_amd as A
    eng, pcs, hop = _setup(dev, model[1], target, 1, 2, solver=solver)
    sched = torch.tensor(SCHED4)
    want = A.fifo_denoise(eng, pcs[0], hop, sched, 3, SEEDS[0])
    got = A.fifo_denoise_clips(eng, pcs, hop, sched, 3, SEEDS[:1])
    assert got.shape == (1,) + tuple(want.shape) and torch.equal(got[0], want)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_slot_control_with_momentum_equals_the_loop_with_carries(dev, model, solver):
    import multimodal_diffusion_amd as A
    eng, pcs, hop = _setup(dev, model[1], "video", 2, 2, solver=solver)
    ctl = dict(rescale_by_level=None, guidance_by_level=lambda t: 1.0 + 3.0 * t / 999.0, apg={"norm_threshold": 2.0, "eta_parallel": 0.25},
               apg_momentum=-0.5)
    eng.set_slot_cfg(guidance=ctl["guidance_by_level"], apg=ctl["apg"], apg_momentum=ctl["apg_momentum"])
    eng.slot_momentum.zero_()
    ref, ref_mom = _loop(eng, pcs, hop, SCHED4, 3, SEEDS[:2], momentum=True)
    eng.slot_momentum.fill_(3.0)                            # the driver starts from zero whatever the buffer held
    out = A.fifo_denoise_clips(eng, pcs, hop, torch.tensor(SCHED4), 3, SEEDS[:2])
    assert torch.equal(out, ref), float((out - ref).abs().max())
    assert torch.equal(eng.slot_momentum, ref_mom) and float(ref_mom.abs().max()) > 0
    eng.clear_slot_cfg()
    # the control passed as arguments is the same control, set for the call and cleared after it
    again = A.fifo_denoise_clips(eng, pcs, hop, torch.tensor(SCHED4), 3, SEEDS[:2], **ctl)
    assert torch.equal(again, out) and eng.slot_momentum is None
    plain = A.fifo_denoise_clips(eng, pcs, hop, torch.tensor(SCHED4), 3, SEEDS[:2])
    assert not torch.equal(plain, out)
    # a rescale table rides the same way (its own statistics pass, no momentum)
    eng.set_slot_cfg(rescale=0.7)
    ref_r, _ = _loop(eng, pcs, hop, SCHED4, 2, SEEDS[:2])
    eng.clear_slot_cfg()
    got_r = A.fifo_denoise_clips(eng, pcs, hop, torch.tensor(SCHED4), 2, SEEDS[:2], rescale_by_level=0.7)
    assert torch.equal(got_r, ref_r) and not torch.equal(got_r, plain[:, :, :got_r.shape[2]])


def test_engine_refuses_a_clip_guide(dev, model):
    eng, pcs, hop = _setup(dev, model[1], "video", 2, 2)
    eng.set_clip_guide(torch.zeros(8, 8, 16, 16, device=dev))
    z = torch.zeros(eng.latent_shape, device=dev)
    with pytest.raises(ValueError, match="fifo_shift_clips takes no clip guide"):
        eng.fifo_shift_clips(z, 2, 4, 999, SEEDS[:2], torch.zeros(2, 8, 6, 16, 16, device=dev), 0)
    import multimodal_diffusion_amd as A
    with pytest.raises(ValueError, match="fifo_denoise_clips takes no clip guide"):
        A.fifo_denoise_clips(eng, pcs, hop, torch.tensor(SCHED4), 3, SEEDS[:2])


# ------------------------------------------------------------------------------------------------- the pipeline
STREAM_ONE_SECOND = {"window_seconds": 1.0, "hop_seconds": 0.5, "crossfade_seconds": 0.25}


def test_pipeline_with_two_prompt_clips(dev, model):
    """the reduced audio -> video pipeline of test_gpu_stream_fifo.py: 1.0 s windows every 0.5 s, S = 2 slots of 2, P = 10 positions
    in 5 slots; 36000 samples are 4 windows"""
    import multimodal_diffusion_amd as A
    from multimodal_diffusion_amd import _pipeline as P
    from multimodal_diffusion_amd import functional as Fn
    from multimodal_diffusion_amd import schedule_utils as su
    from multimodal_diffusion_amd import stream_infer as S
    mods = model[1]
    vae, codec, cfg = pipeline(dev, seed=8, clip_seconds=1.0, sampler_steps=4, streaming=STREAM_ONE_SECOND)
    wavs = [audio_prompt(36000)["prompt_audio"], audio_prompt(36000)["prompt_audio"][::-1].copy()]
    kw = dict(components(mods, vae, codec, dev), cfg=cfg, prompt_modality="audio", prompt_video=None, sampler="fifo", return_latents=True)
    res = S.stream_generate(prompt_audio=wavs, seed=[31, 77], **kw)
    single = S.stream_generate(prompt_audio=wavs[0], seed=31, **kw)
    assert isinstance(res, list) and len(res) == 2
    for r in res:
        assert set(r) == set(single) and r["fps"] == 16
        for key in ("video", "latents", "latent_canvas"):
            assert r[key].shape == single[key].shape and r[key].dtype == single[key].dtype
    # by hand: the two prompt canvases, one engine of batch K * B = 4, fifo_denoise_clips
    abar = su.alphas_cumprod_from_betas(su.make_beta_schedule(1000, kind="cosine", min_beta=1e-4, max_beta=0.02))[1]
    pcs = []
    for w in wavs:
        chunks = S.split_audio_into_windows(w, 16000, 1.0, 0.5)[0]
        pcs.append(S.canvas_from_windows(Fn.window_consensus(P.encode_audio(codec, chunks, dev).float().contiguous(), 75), 75))
    geo = S.fifo_geometry(cfg, "audio", 4, 4, clips=2)
    assert (geo.B, geo.clips, geo.S, geo.slot_len, geo.P, geo.n_slots, geo.prompt_hop) == (4, 2, 2, 2, 10, 5, 75)
    eng = engine(mods, "video", (4, 8, 4, 4, 4), 37, guidance=2.0, alpha_bar=abar, tube=(2, 4, 4), chunk=(4, 4))
    want = A.fifo_denoise_clips(eng, pcs, 75, su.make_sampling_schedule(1000, 4), 5, [31, 77])[:, :, :10]
    for k in range(2):
        assert np.array_equal(res[k]["latent_canvas"], want[k].cpu().numpy())
        assert np.array_equal(res[k]["latents"], S.windows_from_canvas(want[k].contiguous(), 4, 2).cpu().numpy())
    assert not np.array_equal(res[0]["video"], res[1]["video"])
    # one int seeds clip k with seed + k
    by_int = S.stream_generate(prompt_audio=wavs, seed=31, **kw)
    by_list = S.stream_generate(prompt_audio=wavs, seed=[31, 32], **kw)
    assert all(np.array_equal(a["latent_canvas"], b["latent_canvas"]) for a, b in zip(by_int, by_list))
    assert np.array_equal(by_int[0]["latent_canvas"], res[0]["latent_canvas"])
    with pytest.raises(ValueError, match="3 seeds for 2 prompt clips"):
        S.stream_generate(prompt_audio=wavs, seed=[1, 2, 3], **kw)
    with pytest.raises(ValueError, match="equal length"):
        S.stream_generate(prompt_audio=[wavs[0], wavs[1][:30000]], seed=31, **kw)
