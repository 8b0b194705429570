"""Sliding-window long-form generation — mirror of ``avdiff/models/infer/stream_infer.py``.

The reference splits the prompt into windows (3 s window / 1 s hop), calls ``sample_one_direction`` once per window
(B = 1, sequentially) and cross-fades the results on the host.  Windows are independent samples, so here they are one
batch: the prompt windows are encoded together, ``DenoiseEngine`` steps all windows at once (they are the natural
large-batch feed for the data-parallel path), the outputs are decoded together and stitched by a HIP kernel.
With ``shard=True`` under ``torch.distributed`` the windows are the units of the data-parallel layout: rank 0 encodes the
prompt windows, ONE broadcast hands them to every rank, each rank steps AND DECODES its contiguous share of the windows with no
further communication (the reference ends every window's call with its own decode, sample_clip.py:392 via stream_infer.py:182-188,
207-213), one gather brings the decoded windows — uint8 frames or waveforms — to rank 0, which only stitches.

``split_*`` are host-side slicing (as in the reference); the fade tables are built on the host with the reference's
fp32 numpy expressions and uploaded; ``crossfade_*`` keep the reference's numpy-in / numpy-out signatures.
File I/O and the CLI of the reference script are out of scope.

Extension, opt-in (``stream_generate(consensus=...)``): latent window consensus.  Independent windows make the stitched clip the
pixel average of up to window / hop unrelated samples.  With consensus the windows are views of ONE latent canvas: after every
denoising step each canvas position under several windows is replaced in all of them by their weighted mean (MultiDiffusion, Bar-Tal
et al. 2023; ``avd_window_consensus_f32``), so they stay one batch and finish as one coherent latent clip.  ``latent_hop``,
``windows_from_canvas`` and ``canvas_from_windows`` are its host-side geometry.

Extension (``fifo_denoise``): FIFO diagonal denoising, the other family of long-form samplers.  Instead of windows that share one
timestep, a queue of latent slots runs from nearly clean to pure noise, one model call moves every slot one level
(``DenoiseEngine.step_slots``), the head leaves finished and noise enters at the tail (``functional.fifo_shift``).  With
``lookahead=`` the samples are overlapping windows of the queue whose leading slots are held context (``functional.fifo_lookahead``), and
``context=`` continues an existing clip.  ``stream_generate(sampler="fifo")`` runs it from a config, a VAE, a codec and a prompt clip.
``fifo_denoise_clips`` runs K independent clips as K queues in lockstep in one engine (``functional.fifo_shift_clips``), which fills
the batch a short schedule leaves small; ``stream_generate(sampler="fifo")`` takes a list of prompt clips for it.
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _lib as L
from . import _pipeline as P
from . import dist as D
from . import functional as Fn
from . import schedule_utils as su
from .sampler import DenoiseEngine


def split_audio_into_windows(y: np.ndarray, sr: int, win_s: float, hop_s: float) -> Tuple[np.ndarray, int, int]:
    """[L] -> [N, win] (last window zero-padded), stream_infer.py:40-58."""
    n = len(y)
    win, hop = int(round(sr * win_s)), int(round(sr * hop_s))
    if n <= win:
        return y[None, :], win, hop
    starts = list(range(0, n, hop))
    out = []
    for s in starts:
        seg = y[s:min(n, s + win)]
        out.append(np.pad(seg, (0, win - len(seg))) if len(seg) < win else seg)
        if s + win >= n:
            break
    return np.stack(out, axis=0), win, hop


def split_frames_into_windows(frames: np.ndarray, fps: int, win_s: float, hop_s: float) -> Tuple[np.ndarray, int, int]:
    """[T,H,W,3] -> [N, win, H, W, 3] (last window padded by repeating its last frame), stream_infer.py:61-82."""
    n = frames.shape[0]
    win, hop = int(round(fps * win_s)), int(round(fps * hop_s))
    if n <= win:
        return frames[None, ...], win, hop
    out = []
    for s in range(0, n, hop):
        seg = frames[s:min(n, s + win)]
        if seg.shape[0] < win:
            seg = np.concatenate([seg, np.repeat(seg[-1:], win - seg.shape[0], axis=0)], axis=0)
        out.append(seg)
        if s + win >= n:
            break
    return np.stack(out, axis=0), win, hop


def audio_fade_window(L_: int, fade: int) -> np.ndarray:
    """Cosine fade-in / fade-out table (stream_infer.py:103-106); all ones for fade <= 0."""
    w = np.ones(L_, dtype=np.float32)
    if fade > 0:
        w[:fade] = 0.5 * (1 - np.cos(np.linspace(0, np.pi, fade, dtype=np.float32)))
        w[-fade:] = 0.5 * (1 + np.cos(np.linspace(0, np.pi, fade, dtype=np.float32)))
    return w


def video_fade_window(L_: int, fade: int) -> np.ndarray:
    """Triangular ramp table in frames (stream_infer.py:130-137)."""
    w = np.ones(L_, dtype=np.float32)
    if fade > 0:
        ramp = np.linspace(0, 1, fade, dtype=np.float32)
        w[:fade] *= ramp
        w[-fade:] *= ramp[::-1]
    return w


def crossfade_tensor(chunks: torch.Tensor, w: torch.Tensor, hop: int) -> torch.Tensor:
    """chunks [N, L, ...] (float32 or uint8, on the device), w [L] -> [(N-1)*hop + L, ...]."""
    if not chunks.is_cuda:
        raise L.AvdError("crossfade needs ROCm device tensors (no CPU fallback)")
    chunks = chunks.contiguous()
    N, L_ = chunks.shape[:2]
    inner = int(np.prod(chunks.shape[2:])) if chunks.dim() > 2 else 1
    w = w.to(chunks.device, torch.float32).contiguous()
    out = torch.empty((N - 1) * hop + L_, *chunks.shape[2:], device=chunks.device, dtype=chunks.dtype)
    fn = L.lib().avd_crossfade_u8 if chunks.dtype == torch.uint8 else L.lib().avd_crossfade_f32
    if chunks.dtype not in (torch.uint8, torch.float32):
        raise TypeError("crossfade takes float32 or uint8 chunks")
    L.check(fn(chunks.data_ptr(), w.data_ptr(), out.data_ptr(), N, L_, hop, inner, L.stream_ptr(chunks.device)))
    return out


def crossfade_audio(chunks: np.ndarray, sr: int, hop: int, win: int, fade_s: float, device="cuda") -> np.ndarray:
    """[N, L] float32 -> stitched [ (N-1)*hop + L ] (stream_infer.py:85-116)."""
    fade = int(round(sr * fade_s))
    w = torch.from_numpy(audio_fade_window(chunks.shape[1], fade))
    out = crossfade_tensor(torch.from_numpy(np.ascontiguousarray(chunks, dtype=np.float32)).to(device), w, hop)
    return out.cpu().numpy()


def crossfade_video(chunks: np.ndarray, hop: int, win: int, fade_f: int, device="cuda") -> np.ndarray:
    """[N, T, H, W, 3] uint8 -> stitched [T_total, H, W, 3] uint8 (stream_infer.py:119-143)."""
    w = torch.from_numpy(video_fade_window(chunks.shape[1], int(fade_f)))
    out = crossfade_tensor(torch.from_numpy(np.ascontiguousarray(chunks)).to(device), w, hop)
    return out.cpu().numpy()


def latent_hop(cfg: Dict, target: str) -> Tuple[int, int]:
    """(hop, L): the hop and the window length in latent positions of the target's sliding axis, from ``streaming.window_seconds`` /
    ``hop_seconds``.  Video (axis T): the window's and the hop's frames over ``t_down``; audio (axis F): ``frames_per_clip`` latent
    frames per window, hop = Fa * hop_s / win_s.  ValueError when the hop is not a whole number of latent positions (windows could not
    share canvas positions)."""
    st = cfg.get("streaming", {})
    win_s, hop_s = float(st.get("window_seconds", 3.0)), float(st.get("hop_seconds", 1.0))
    if target == "video":
        fps, t_down = int(cfg["video"]["fps"]), int(cfg["video"]["latent"]["t_down"])
        win_f, hop_f = int(round(fps * win_s)), int(round(fps * hop_s))
        if hop_f <= 0 or hop_f % t_down:
            raise ValueError(f"the hop of {hop_s} s is {hop_f} frames, not a positive multiple of the VAE's t_down = {t_down}: the windows "
                             "do not share latent frames")
        return hop_f // t_down, max(1, win_f // t_down)
    if target == "audio":
        Fa = int(cfg["audio"]["latent"]["frames_per_clip"])
        hop = Fa * hop_s / win_s
        if hop < 0.5 or abs(hop - round(hop)) > 1e-9 * hop:
            raise ValueError(f"the hop of {hop_s} s is {hop:g} of the window's {Fa} latent frames, not a positive whole number: the windows "
                             "do not share latent frames")
        return int(round(hop)), Fa
    raise ValueError("target must be 'video' or 'audio'")


def windows_from_canvas(canvas: torch.Tensor, L_: int, hop: int) -> torch.Tensor:
    """Latent canvas -> the batch of its windows: video [C, P, H, W] -> [N, C, L, H, W], audio [Ca, P] -> [N, Ca, L], with
    P = (N-1)*hop + L; window k is canvas positions k*hop .. k*hop + L - 1 (overlapping windows repeat canvas values)."""
    if canvas.dim() not in (2, 4):
        raise ValueError(f"a latent canvas is [C, P, H, W] (video) or [Ca, P] (audio), got shape {tuple(canvas.shape)}")
    P = canvas.shape[1]
    if L_ <= 0 or hop <= 0 or P < L_ or (P - L_) % hop:
        raise ValueError(f"a canvas of {P} positions is not (N-1)*{hop} + {L_} for any N >= 1")
    return torch.stack([canvas[:, k * hop:k * hop + L_] for k in range((P - L_) // hop + 1)], 0).contiguous()


def canvas_from_windows(windows: torch.Tensor, hop: int) -> torch.Tensor:
    """Inverse of ``windows_from_canvas`` for a batch whose windows agree wherever they overlap (what the consensus leaves): [N, C, L,
    H, W] -> [C, (N-1)*hop + L, H, W], [N, Ca, L] -> [Ca, (N-1)*hop + L].  Where windows disagree the later one wins."""
    if windows.dim() not in (3, 5):
        raise ValueError(f"a window batch is [N, C, L, H, W] (video) or [N, Ca, L] (audio), got shape {tuple(windows.shape)}")
    if hop <= 0:
        raise ValueError(f"hop must be > 0, got {hop}")
    N, L_ = windows.shape[0], windows.shape[2]
    canvas = windows.new_empty((windows.shape[1], (N - 1) * hop + L_) + tuple(windows.shape[3:]))
    for k in range(N):
        canvas[:, k * hop:k * hop + L_] = windows[k]
    return canvas


def fifo_prompt_windows(prompt_canvas: torch.Tensor, m: int, B: int, S: int, prompt_hop: int, prompt_len: int,
                        stride: Optional[int] = None, first: Optional[int] = None, prompt_den: int = 1,
                        prompt_interp: Optional[str] = None) -> torch.Tensor:
    """The prompt batch of ``fifo_denoise`` before the step of steady iteration ``m``: sample k is prompt positions (m + k*S) *
    prompt_hop .. + prompt_len - 1 of the canvas's sliding axis ([C, P, H, W] video prompt, [Ca, P] audio prompt), zeros beyond the
    canvas end.  Returns [B, C, prompt_len, H, W] / [B, Ca, prompt_len] on the canvas's device (any device: pure slicing).
    ``stride`` (None = S) and ``first`` (None = m; may be negative) generalise it to sample k at positions (first + k*stride) *
    prompt_hop ..: the overlapping windows of the lookahead queue (stride = S - ctx, first = m - ctx).  Positions before the canvas
    start are zeros like those past its end.
    ``prompt_den`` / ``prompt_interp`` (defaults 1 / None: everything above, call for call) walk the canvas by the rational hop
    ``prompt_hop / prompt_den`` (include/avdiff_hip.h, "fractional prompt hop"; this function is its pure-torch statement and the CPU
    reference of ``functional.fifo_prompt_gather_frac``): for the clip slot q = first + k*stride of sample k, i0 = floor(q * prompt_hop /
    prompt_den) and rem = q * prompt_hop - i0 * prompt_den; "nearest" reads positions i0 + (2*rem >= prompt_den) .., "linear" the fp32
    value a + f * (b - a) of positions i0 + l and i0 + l + 1 with f = float32(rem) / float32(prompt_den), a itself when rem == 0.  A
    ``prompt_den`` > 1 without a mode is a ValueError."""
    if prompt_canvas.dim() not in (2, 4):
        raise ValueError(f"a prompt canvas is [C, P, H, W] (video) or [Ca, P] (audio), got shape {tuple(prompt_canvas.shape)}")
    if min(B, S, prompt_hop, prompt_len) < 1 or m < 0:
        raise ValueError(f"fifo_prompt_windows: need B, S, prompt_hop, prompt_len >= 1 and m >= 0 (got {B}, {S}, {prompt_hop}, "
                         f"{prompt_len}, {m})")
    for name, v in (("stride", stride), ("first", first)):
        if v is not None and (isinstance(v, bool) or not isinstance(v, int) or (name == "stride" and v < 1)):
            raise ValueError(f"fifo_prompt_windows: {name} must be an int{' >= 1' if name == 'stride' else ''} or None, got {v!r}")
    if prompt_den != 1 or prompt_interp is not None:
        Fn.check_prompt_frac(prompt_hop, prompt_den, prompt_interp)
        if prompt_interp == "linear" and prompt_canvas.dtype != torch.float32:
            raise ValueError(f"prompt_interp='linear' blends in float32: the prompt canvas is {prompt_canvas.dtype}")
    stride = S if stride is None else stride
    first = m if first is None else first
    P_ = prompt_canvas.shape[1]
    out = prompt_canvas.new_zeros((B, prompt_canvas.shape[0], prompt_len) + tuple(prompt_canvas.shape[2:]))

    def rows(dst: torch.Tensor, p0: int) -> torch.Tensor:
        """canvas positions p0 .. p0 + prompt_len - 1 into ``dst`` (zeros to start with), where they lie on the canvas"""
        lo, hi = max(p0, 0), min(p0 + prompt_len, P_)
        if hi > lo:
            dst[:, lo - p0:hi - p0] = prompt_canvas[:, lo:hi]
        return dst

    for k in range(B):
        if prompt_interp is None:
            rows(out[k], (first + k * stride) * prompt_hop)
            continue
        t = (first + k * stride) * prompt_hop                      # Python ints: exact, and // is a floor for negative slots too
        i0 = t // prompt_den
        rem = t - i0 * prompt_den
        if prompt_interp == "nearest":
            rows(out[k], i0 + (1 if 2 * rem >= prompt_den else 0))
        else:
            a = rows(out[k], i0)
            if rem:                                                # rem == 0: a itself, the neighbour is not read
                b = rows(torch.zeros_like(a), i0 + 1)
                f = (torch.tensor(rem, dtype=torch.float32) / prompt_den).to(a.device)      # divided on the CPU: one IEEE division
                out[k] = a + f * (b - a)
    return out


def fifo_prompt_len(engine: DenoiseEngine, prompt_canvas: torch.Tensor) -> int:
    """The prompt latent's length along its sliding axis that gives the engine's ``prompt_tokens``: an audio prompt (video target)
    of Np chunks is (Np - 1) * stride + length frames; a video prompt (audio target) [C, P, H, W] of Np tubes is Np / (H/h * W/w)
    token frames of the tube's t."""
    Np = engine.embed.Np
    if engine.target == "video":
        if prompt_canvas.dim() != 2:
            raise ValueError(f"a video target takes an audio prompt canvas [Ca, P], got shape {tuple(prompt_canvas.shape)}")
        ln, st = engine.chunk
        return (Np - 1) * st + ln
    if prompt_canvas.dim() != 4:
        raise ValueError(f"an audio target takes a video prompt canvas [C, P, H, W], got shape {tuple(prompt_canvas.shape)}")
    t, h, w = engine.tube
    H, W = prompt_canvas.shape[2:]
    if H % h or W % w or Np % ((H // h) * (W // w)):
        raise ValueError(f"a prompt canvas of {H} x {W} does not tile into the engine's {Np} prompt tokens with tube {engine.tube}")
    return Np // ((H // h) * (W // w)) * t


@torch.no_grad()
def fifo_denoise(engine: DenoiseEngine, prompt_canvas: torch.Tensor, prompt_hop: int, sched, n_slots: int, noise_seed: int,
                 graph: Optional[bool] = False, lookahead: int = 0, context: Optional[torch.Tensor] = None,
                 init_canvas: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None, guide_seed: int = 0,
                 guide_start: str = "noise", guidance_by_level=None, rescale_by_level=None, apg: Optional[dict] = None,
                 guided_shift: bool = False, prompt_den: int = 1, prompt_interp: Optional[str] = None,
                 apg_momentum: Optional[float] = None) -> torch.Tensor:
    """FIFO diagonal denoising (FIFO-Diffusion, Kim et al. 2024, with latent partitioning): a clip of ``n_slots`` slots of
    ``engine.slot_len`` latent positions, denoised in a queue whose slots sit at different noise levels.  Returns the finished latent
    canvas [C, n_slots * slot_len, H, W] (video target) or [Ca, n_slots * slot_len] (audio target).

    ``sched`` = s_0 > ... > s_n = -1 with n = engine batch * ``engine.slots`` (``schedule_utils.fifo_plan``): the engine's batch is
    the queue, n slots from nearly clean (head) to pure noise (tail).  The queue starts as seeded noise at s_0
    (``functional.canvas_noise``: clip slot c always starts from the same normals, however long the clip), n - 1 ramp steps bring it
    to the diagonal, then every steady iteration is one ``step_slots`` — each slot moves one level — and one ``functional.fifo_shift``:
    the head leaves finished, fresh noise enters at the tail.  Memory is constant in the clip length and a finished slot costs n / S
    sample-steps, what non-overlapping windows cost; nothing is cross-faded or averaged.  Every driver below takes its checked plan from
    ``DenoiseEngine.fifo_plan`` before anything is allocated or launched: a schedule that does not fit the queue, a clip whose
    (n + n_slots) * slot_len leaves the stream's 2**32 canvas positions and what ``step_slots`` refuses are ValueErrors raised there.
    ``prompt_canvas`` is the prompt modality's latent along its sliding axis and ``prompt_hop`` its positions per target slot: before
    the step of steady iteration m (the ramp: m = 0) sample k is conditioned on ``fifo_prompt_windows(prompt_canvas, m, ...)[k]``,
    the prompt under the clip slots the sample holds (``set_prompt`` into the same buffer).  The engine's limits are ``step_slots``'s
    (no guide / control / consensus).
    An engine with eta > 0 and a ``noise_seed`` samples stochastically, in every driver below: each ``step_slots`` is keyed by the clip
    slots the batch holds (``schedule_utils.fifo_slot_keying``; include/avdiff_hip.h, "clip-keyed slot noise"), so clip slot c draws
    the same step normals at each of its n steps in the eager loop, the replayed one and the lookahead queue, whatever the clip
    length.  The step noise is seeded by ``engine.noise_seed``; the ``noise_seed`` argument keeps seeding the start and the entering
    noise, and the two may be equal: the step noise has a domain tag of its own.  An eta > 0 engine without a ``noise_seed`` is
    refused, as ``step_slots`` refuses it.
    ``graph`` (False, True or None; default False = the eager loop: per finished slot the host runs one ``set_prompt``, one
    ``step_slots`` and one ``fifo_shift``): True replays the iterations from captured HIP graphs and returns the same bits.  The ramp
    row, the prompt positions and the clip slot are then read off two int32 device cursors (``DenoiseEngine.fifo_open``;
    include/avdiff_hip.h, "FIFO device cursors"), so an iteration is a fixed chain of launches; each phase takes its first iteration
    eagerly through those kernels, replays a captured pair of iterations while two or more are left, and takes an odd last one
    eagerly.  The graphs are captured per call and dropped with it: they hold the seed, the clip length, the hops and every address by
    value.  None follows ``DenoiseEngine.run``'s rule: replay when 2 * B * N < ``GRAPH_BELOW_ROWS``.  ``step_slots``'s refusals are
    raised before anything is captured.  Either way the returned canvas is a fresh tensor the caller owns (with ``graph`` the queue's
    clip canvas, which the shift kernel wrote in place; no graph that could write it again outlives the call).
    The driver follows ``engine.solver``.  "dpmpp_2m" adds the ``t_last`` tables (``schedule_utils.fifo_plan_last``) and shifts with
    ``engine.fifo_shift``, which carries every slot's history along with it; ``x0_hist`` needs no initialisation, every slot's first
    step being first order.  The queue is as long as the schedule, so the faster solver's shorter schedule also means a shorter
    queue, a shorter ramp and fewer sample-steps per finished slot.
    ``lookahead`` = ctx > 0 (ctx < S, else ValueError) is FIFO lookahead denoising (the paper's second half; layout and plan in
    include/avdiff_hip.h, "FIFO lookahead", and ``schedule_utils.fifo_lookahead_plan``): the engine's samples are overlapping windows of
    the queue, h = S - ctx slots apart; the first ctx slots of every window are held context, the cleaner slots in front of the h slots
    the window updates, and ctx context slots before the head keep the most recently finished slots in view.  ``sched`` then has n =
    batch * h steps.  The queue starts as canvas-keyed noise at s_0: clip slot c >= 0 from the normals it starts from without
    lookahead, context slot q from those of canvas positions (q - ctx) * slot_len + j modulo 2^32, the positions just before the clip.
    The ramp is n - 1 times ``step_slots`` + ``engine.fifo_lookahead(shift=0)`` (the refresh of the duplicates), every steady iteration
    ``set_prompt`` -> ``step_slots`` on row min(m, ctx) of the plan -> ``engine.fifo_lookahead(shift=1)``, whose popped head goes into
    the clip.  Window k at steady iteration m is conditioned on prompt positions (m - ctx + k*h) * prompt_hop .. (the ramp: m = 0),
    zeros before the canvas start and past its end.  A finished slot costs batch = n / h sample-steps against n / S without lookahead:
    a factor S / h, 2 at ctx = S / 2.  Eager only: ``graph=True`` is refused before anything is allocated, None runs eagerly.
    ``context`` (with ``lookahead`` only): the clean latent of the ctx slots before the clip, [C, ctx * slot_len, H, W] (video) or
    [Ca, ctx * slot_len] (audio).  It fills the context slots at the start, labelled clean (the "clean" plan): the clip continues an
    existing one.  The prompt under a supplied context is zeros.  ``lookahead=0`` is the queue above, launch for launch.
    ``init_canvas`` (the plain eager queue, both solvers, eta == 0 and eta > 0) guides the clip by a clean latent canvas [C, P, H, W]
    / [Ca, P] (include/avdiff_hip.h, "clip-keyed latent guide"): long-form inpainting, outpainting and SDEdit.  ``mask``: None = 1
    everywhere, or values in [0, 1] broadcastable to the canvas (``sampler.canvas_frame_mask`` gives one): 1 keeps the canvas, 0 is
    generated, clip positions past P are unguided.  After the start noise is drawn one ``functional.clip_guide_slots`` call puts every
    slot on the forward path q(s_0) of its clip positions, after every shift one in-place call does so for the entering tail slot
    alone, and every ``step_slots`` runs under ``engine.set_clip_guide`` at the clip slot then at queue slot 0 — so a held region
    leaves the queue equal to the canvas bit for bit.  The known noise is keyed by ``guide_seed`` and clip position, the stream of
    ``stream_generate``'s canvas-keyed guide.  ``guide_start``: "noise" starts the unmasked positions from noise; "init" (SDEdit)
    starts every in-canvas position from q(s_0) of the canvas — pass the truncated schedule
    (``schedule_utils.truncate_schedule``), whose length sets the queue.  The engine's clip guide is set for the call and cleared
    after it.  ``graph=True`` or ``lookahead > 0`` with ``init_canvas`` raises ValueError before anything is allocated.
    ``guided_shift=True`` (with ``init_canvas``; default False: the launches above) folds the tail slot's pass into the shift's own
    launch (``functional.fifo_shift(guide=)``; include/avdiff_hip.h, "Guided FIFO queue shift"): one launch fewer per finished slot,
    the same bits.  ``stream_generate(sampler="fifo")`` runs its init clips this way.
    ``guidance_by_level`` / ``rescale_by_level`` / ``apg`` (every driver: eager, ``graph=True``, ``lookahead``, and the eager one under
    ``init_canvas``) control the CFG combine per slot (``DenoiseEngine.set_slot_cfg``; include/avdiff_hip.h, "slot CFG control"): the
    first two are ``schedule_utils.level_table`` specs looked up at each slot's own noise level (``guidance_interval_table`` gives a
    guidance interval), ``apg`` {"norm_threshold":, "eta_parallel":} is per-slot adaptive projected guidance.  They are
    checked before anything is allocated; the engine's slot control is set for the call and cleared after it, also when it raises.
    ``apg_momentum`` (with ``apg``; every driver; a finite number, negative in the APG paper; None or 0 = none) adds APG's momentum per
    slot (include/avdiff_hip.h, "slot APG momentum"): every slot's direction accumulates over the steps it takes, in an engine-owned
    buffer that each queue move carries along with the slot (one ``functional.fifo_carry`` launch behind the shift); the call starts
    from a zeroed buffer and an entering slot from zero.  The ``apg`` dict's own "momentum" key stays refused: it names the
    per-sample buffer of ``DenoiseEngine.set_apg``.
    ``prompt_den`` / ``prompt_interp`` (every driver; defaults 1 / None) make the prompt hop the fraction ``prompt_hop / prompt_den`` of
    prompt positions per target slot (include/avdiff_hip.h, "fractional prompt hop"): a video prompt under an audio target, 8 / 25 at
    the shipped geometry.  ``prompt_hop`` keeps its meaning and its check: it is the numerator.  ``prompt_interp`` "nearest" reads the
    real latent rows nearest to where a slot's window starts, "linear" blends the two neighbouring rows in fp32; which serves a trained
    model better cannot be measured on synthetic weights.  With ``prompt_den`` > 1 (which needs a mode: ValueError without) the eager
    loops take each iteration's prompt from ``functional.fifo_prompt_gather_frac`` (the lookahead one with stride = h, first = m - ctx)
    and ``set_prompt`` it, and ``graph=True`` launches the same gather off the cursor m (``DenoiseEngine.fifo_open(prompt_den=,
    prompt_interp=)``).  Sample k is then conditioned on ``fifo_prompt_windows(..., prompt_den=, prompt_interp=)[k]``, bit for bit.
    With ``prompt_den`` == 1 every driver is the one above, launch for launch, whatever the mode."""
    scfg, frac = _fifo_scalar_checks("fifo_denoise", engine, n_slots, prompt_hop, prompt_den, prompt_interp, guide_start,
                                     (guidance_by_level, rescale_by_level, apg, apg_momentum))
    if graph is not None and not isinstance(graph, bool):
        raise TypeError(f"graph must be True, False or None, got {graph!r}")
    if isinstance(lookahead, bool) or not isinstance(lookahead, int) or not 0 <= lookahead < engine.slots:
        raise ValueError(f"lookahead must be an int in [0, S = {engine.slots}): the context slots of a window of S, got {lookahead!r}")
    if init_canvas is None and (mask is not None or guide_start != "noise"):
        raise ValueError("mask and guide_start belong to the clip guide: pass init_canvas")
    if not isinstance(guided_shift, bool) or (guided_shift and init_canvas is None):
        raise ValueError(f"guided_shift must be a bool, and True only with init_canvas (it guides the entering slot), got {guided_shift!r}")
    if init_canvas is not None:
        if graph:
            raise ValueError("fifo_denoise(init_canvas=...) runs eagerly: the replayed queue has no guided tail pass, graph=True is refused")
        if lookahead:
            raise ValueError("fifo_denoise(init_canvas=...) drives the plain queue: the lookahead queue takes no clip guide, lookahead > 0 "
                             "is refused")
        Fn.noise_key(guide_seed, 0)
        graph = False      # None follows the row rule only without a guide
    if lookahead:
        if graph:
            raise ValueError("fifo_denoise(lookahead > 0) runs eagerly: the lookahead queue has no device cursors, graph=True is refused")
        with _slot_cfg_scope(engine, scfg):
            return _fifo_denoise_lookahead(engine, prompt_canvas, prompt_hop, sched, n_slots, noise_seed, lookahead, context, frac)
    if context is not None:
        raise ValueError("context is the clean latent of the lookahead's context slots: it needs lookahead > 0")
    Lp = fifo_prompt_len(engine, prompt_canvas)
    if graph is None:
        graph = 2 * engine.embed.B * engine.N < engine.GRAPH_BELOW_ROWS
    if graph:      # fifo_open makes the plan's checks itself
        with _slot_cfg_scope(engine, scfg):
            return _fifo_denoise_graph(engine, engine.fifo_open(prompt_canvas, prompt_hop, Lp, sched, n_slots, noise_seed,
                                                                prompt_den=prompt_den, prompt_interp=prompt_interp))
    # under a clip guide, the call's or the engine's own, the steps are keyed by the clip slot at queue slot 0 at any eta
    keying = _fifo_clip_keying(engine, engine.slots, 0, guided=init_canvas is not None or engine._clip is not None)
    plan = engine.fifo_plan(sched, n_slots, clip_first=keying[0](0))
    Fn.noise_key(noise_seed, 0)
    pc = L.dev_f32(prompt_canvas.to(engine.device), "prompt canvas")
    if init_canvas is not None:
        engine.set_clip_guide(init_canvas, mask, guide_seed=guide_seed)
    try:
        with _slot_cfg_scope(engine, scfg):
            return _fifo_denoise_eager(engine, pc, prompt_hop, Lp, plan, keying, n_slots, noise_seed, guide_start == "init", guided_shift,
                                       frac)
    finally:
        if init_canvas is not None:
            engine.clear_clip_guide()


def _fifo_scalar_checks(what: str, engine, n_slots, prompt_hop, prompt_den, prompt_interp, guide_start, slot_cfg):
    """the argument checks ``fifo_denoise`` and ``fifo_denoise_clips`` share, the slot CFG arguments (``slot_cfg``: guidance, rescale,
    apg, apg_momentum) first: returns (``_check_slot_cfg``'s result or None, (prompt_den, prompt_interp) or None on a whole hop)"""
    if not isinstance(engine, DenoiseEngine):
        raise TypeError(f"{what} drives a DenoiseEngine")
    scfg = None if all(a is None for a in slot_cfg) else engine._check_slot_cfg(*slot_cfg)
    if isinstance(n_slots, bool) or not isinstance(n_slots, int) or n_slots < 1:
        raise ValueError(f"n_slots must be an int >= 1, got {n_slots!r}")
    if isinstance(prompt_hop, bool) or not isinstance(prompt_hop, int) or prompt_hop < 1:
        raise ValueError(f"prompt_hop must be an int >= 1 (prompt positions per target slot), got {prompt_hop!r}")
    Fn.check_prompt_frac(prompt_hop, prompt_den, prompt_interp)
    if guide_start not in ("noise", "init"):
        raise ValueError(f"guide_start must be 'noise' or 'init', got {guide_start!r}")
    return scfg, (prompt_den, prompt_interp) if prompt_den > 1 else None


@contextlib.contextmanager
def _slot_cfg_scope(engine: DenoiseEngine, checked):
    """the engine's slot CFG control for one fifo_denoise call: ``checked`` is ``_check_slot_cfg``'s result, None = leave the engine as
    it is.  Either way a slot momentum starts the call from zero."""
    if checked is not None:
        engine._apply_slot_cfg(*checked)
    if engine.slot_momentum is not None:
        engine.slot_momentum.zero_()
    try:
        yield
    finally:
        if checked is not None:
            engine.clear_slot_cfg()


def _fifo_queue_loop(engine: DenoiseEngine, z: torch.Tensor, plan, tabs, n_slots: int, windows, first, step_kw: dict, ramp_move,
                     steady_move) -> None:
    """The loop every eager FIFO driver runs on a queue ``z`` whose prompt of m = 0 is set: n - 1 ramp iterations of ``step_slots`` on
    row r of the ramp tables and ``ramp_move``, then per finished slot m ``set_prompt(windows(m))`` (m > 0), ``step_slots`` on the
    plan's steady tables of m, and ``steady_move``.  The driver supplies what differs:
    ``tabs`` = (ramp, steady), the plan's tables where and how the driver laid them out; ``windows``: m -> the prompt batch; ``first``:
    m -> ``clip_first`` and ``step_kw`` the other keywords of every ``step_slots``; ``ramp_move(new, old)`` -> (the queue after a ramp
    step, the buffer the next step writes); ``steady_move(new, m)`` -> the queue after the move, which also puts the finished head
    where it belongs and runs the driver's pass over the entering tail, if it has one."""
    ramp, steady = tabs
    other = torch.empty_like(z)
    for r in range(plan.n - 1):
        other = engine.step_slots(z, ramp[0][r], ramp[1][r], out=other, t_last=ramp[2][r] if len(ramp) == 3 else None,
                                  clip_first=first(0), **step_kw)
        z, other = ramp_move(other, z)
    for m in range(n_slots):
        if m:
            engine.set_prompt(windows(m))
        now, prev, *last = plan.steady_tables(steady, m)
        other = engine.step_slots(z, now, prev, out=other, t_last=last[0] if last else None, clip_first=first(m), **step_kw)
        z = steady_move(other, m)


def _fifo_denoise_eager(engine: DenoiseEngine, pc: torch.Tensor, prompt_hop: int, Lp: int, plan, keying, n_slots: int, noise_seed: int,
                        everywhere: bool, guided_shift: bool = False, frac=None) -> torch.Tensor:
    """``fifo_denoise``'s plain queue for ``_fifo_queue_loop``; under ``engine.set_clip_guide`` the guided one (the contract is in
    ``fifo_denoise``): the start and every entering tail slot go through ``functional.clip_guide_slots`` at s_0 — with ``guided_shift``
    the tail slot inside the shift's own launch (``engine.fifo_shift(guided=)``).  ``keying``: ``_fifo_clip_keying``'s result, which
    the plan was checked with; ``frac`` = (prompt_den, prompt_interp) takes the prompt from the fractional gather, not the slices."""
    B, S, sl = engine.embed.B, engine.slots, engine.slot_len
    n, s0, dev = plan.n, plan.s0, engine.device
    z = Fn.canvas_noise(noise_seed, torch.full((B,), s0, dtype=torch.long, device=dev), engine.latent_shape, plan.L)
    windows = _fifo_prompt_source(pc, B, S, prompt_hop, Lp, S, 0, frac)
    engine.set_prompt(windows(0))
    clip, guided, tail_pass = engine._clip, None, None
    if clip is not None:
        ab = engine.alpha_bar.to(dev, torch.float32)
        guide = dict(slot_len=sl, seed=clip[2], everywhere=everywhere)
        Fn.clip_guide_slots(clip[0], torch.full((B, S), s0, dtype=torch.long, device=dev), ab, z, clip[1], first=0, out=z, **guide)
        if guided_shift:      # clip slot n + m enters at q(s_0) inside the shift
            guided = "everywhere" if everywhere else "mask"
        else:      # the entering tail slot alone: clip slot n + m, now that clip slot m + 1 is at queue slot 0
            tail = torch.full((B, S), Fn.SLOT_LEAVE, dtype=torch.long, device=dev)
            tail[B - 1, S - 1] = s0
            tail_pass = (lambda z, m: Fn.clip_guide_slots(clip[0], tail, ab, z, clip[1], first=m + 1, out=z, **guide))
    canvas = torch.empty((plan.outer, n_slots * sl) + plan.trailing, device=dev, dtype=torch.float32)

    def shift(new, m):
        z, popped = engine.fifo_shift(new, n + m, s0, seed=noise_seed, guided=guided)
        if tail_pass is not None:
            tail_pass(z, m)
        canvas[:, m * sl:(m + 1) * sl] = popped
        return z

    _fifo_queue_loop(engine, z, plan, ([t.to(dev) for t in plan.ramp], [t.to(dev) for t in plan.steady]), n_slots, windows, keying[0],
                     dict(clip_stride=keying[1]), lambda new, old: (new, old), shift)
    return canvas


@torch.no_grad()
def fifo_denoise_clips(engine: DenoiseEngine, prompt_canvases, prompt_hop: int, sched, n_slots: int, noise_seeds, prompt_den: int = 1,
                       prompt_interp: Optional[str] = None, guidance_by_level=None, rescale_by_level=None, apg: Optional[dict] = None,
                       apg_momentum: Optional[float] = None, step_seeds=None, init_canvases=None, masks=None, guide_seeds=None,
                       guide_start: str = "noise") -> torch.Tensor:
    """``fifo_denoise`` for K independent clips at once (include/avdiff_hip.h, "FIFO clip batch"): the engine's batch B = K * B_q is K
    queues in lockstep, queue k the samples k * B_q .. (k + 1) * B_q - 1 under prompt ``prompt_canvases[k]`` and seed
    ``noise_seeds[k]``, and every model call finishes one slot of every clip.  The queue's own batch is pinned to the schedule (B_q * S
    = n steps), so this is how a short schedule fills the machine.  Returns the K finished canvases [K, C, n_slots * slot_len, H, W]
    (video target) or [K, Ca, n_slots * slot_len] (audio target).
    ``prompt_canvases``: a sequence of K prompt canvases of one shape, or one stacked tensor [K, ...].  ``noise_seeds``: K ints; equal
    seeds are allowed and give correlated starts (the same start and entering noise under different prompts).  ``prompt_hop``,
    ``sched``, ``n_slots``, ``prompt_den`` / ``prompt_interp`` and the slot CFG control (``guidance_by_level``, ``rescale_by_level``,
    ``apg``, ``apg_momentum``: one control for all clips, the momentum buffer starting from zero) are ``fifo_denoise``'s.  The engine's
    batch must be K * B_q with B_q * S = n, else ValueError.
    It is the plain eager loop: queue k starts from ``canvas_noise(noise_seeds[k], ...)``, the ramp and steady tables are
    ``fifo_plan``'s (``fifo_plan_last``'s on solver "dpmpp_2m") tiled K times, and a steady iteration is one ``set_prompt`` of the K
    clips' prompt batches concatenated, one ``step_slots`` and one ``engine.fifo_shift_clips``, which moves every queue, its history
    and its slot momentum and writes the K heads into the result in one launch.  Nothing else on the host depends on K, and the loop
    never synchronises.  Clip k's samples see only their own prompt, tables and seed, so its canvas does not depend on the other clips
    of the batch; equal bits across different batch sizes are not promised (the GEMMs may pick a kernel by row count).
    ``step_seeds`` (K ints; include/avdiff_hip.h, "clip batch keying") admits an eta > 0 engine: it runs ``fifo_denoise``'s stochastic
    loop per queue, every ``step_slots`` under ``clip_queues=K, clip_seeds=step_seeds`` and keyed by the clip slot at slot 0 of each
    queue (``schedule_utils.fifo_slot_keying``, stride S inside a queue), so clip k draws the step normals ``fifo_denoise`` draws on an
    engine with ``noise_seed=step_seeds[k]``.  The engine's own ``noise_seed`` is not read.  On an eta == 0 engine ``step_seeds`` is
    checked (count and types) and otherwise ignored: nothing is drawn, the same launches, the same bits.
    ``init_canvases`` (K clean latent canvases of one shape, or a stacked tensor [K, C, P, H, W] / [K, Ca, P]) runs the guided queue
    per clip, ``fifo_denoise(init_canvas=)`` K times over: ``masks`` None or K masks (each broadcastable to a canvas), ``guide_seeds``
    K ints (None = K zeros, as ``guide_seed`` defaults to 0), ``guide_start`` "noise" or "init" with the truncated schedule, as
    there.  The start goes through one ``functional.clip_guide_slots_clips`` call at s_0, each ``fifo_shift_clips`` is followed by one
    in-place call for the K entering tails, and every step runs under ``engine.set_clip_guides`` (set for the call, cleared after
    it): a held region leaves queue k equal to canvas k bit for bit.  The guided shift inside the clip batch's own launch is not
    built; ``masks`` or a ``guide_start`` other than "noise" without ``init_canvases`` is refused.
    Limits, refused before anything is allocated: an engine with eta > 0 and no ``step_seeds`` (the clip-keyed slot noise would have one
    seed and one clip-position walk per call, so the K clips would draw the same step normals), an engine with a clip guide or clip
    guides of its own (``set_clip_guide`` is one canvas, one queue; pass ``init_canvases``), K = 0, canvases of differing shapes, a
    seed or canvas count other than K.  The replayed queue, the lookahead queue and a context are ``fifo_denoise``'s alone; the clips
    run in lockstep and so share ``n_slots``."""
    scfg, frac = _fifo_scalar_checks("fifo_denoise_clips", engine, n_slots, prompt_hop, prompt_den, prompt_interp, guide_start,
                                     (guidance_by_level, rescale_by_level, apg, apg_momentum))
    pcs = list(prompt_canvases.unbind(0)) if isinstance(prompt_canvases, torch.Tensor) else list(prompt_canvases)
    K = len(pcs)
    if K == 0:
        raise ValueError("fifo_denoise_clips needs at least one clip: K = 0 prompt canvases were passed")
    if any(not isinstance(p, torch.Tensor) or p.shape != pcs[0].shape for p in pcs):
        raise ValueError(f"the {K} prompt canvases must be tensors of one shape (the clips run in lockstep), got "
                         f"{[tuple(p.shape) if isinstance(p, torch.Tensor) else p for p in pcs]}")
    seeds = Fn.clip_seeds(noise_seeds, K)
    if step_seeds is not None:
        step_seeds = Fn.clip_seeds(step_seeds, K)
    if engine.eta > 0 and step_seeds is None:
        raise ValueError(f"fifo_denoise_clips needs eta == 0 (the engine has eta = {engine.eta}): the clip-keyed slot noise has one seed "
                         "and one clip-position walk per call, so the K clips would draw the same step normals; pass step_seeds, one "
                         "per clip, for per-clip step noise")
    engine._clip_refusal("fifo_denoise_clips", "a clip guide is one canvas walked by one queue, and a clip batch holds several")
    if engine._clips is not None:
        raise ValueError("fifo_denoise_clips sets the engine's clip guides for the call: clear_clip_guides() first and pass init_canvases")
    if init_canvases is None and (masks is not None or guide_seeds is not None or guide_start != "noise"):
        raise ValueError("masks, guide_seeds and guide_start belong to the clip guides: pass init_canvases")
    if init_canvases is not None:
        init_canvases = Fn.stack_clip_canvases(init_canvases, "init")
        if init_canvases.shape[0] != K:
            raise ValueError(f"{init_canvases.shape[0]} init canvases for {K} clips: fifo_denoise_clips needs one canvas per clip")
        if masks is not None and not isinstance(masks, torch.Tensor) and len(masks) != K:
            raise ValueError(f"{len(masks)} masks for {K} clips: fifo_denoise_clips needs one mask per clip, or None")
        guide_seeds = Fn.clip_seeds([0] * K if guide_seeds is None else guide_seeds, K)
    B, S, sl = engine.embed.B, engine.slots, engine.slot_len
    keyed, guided = engine.eta > 0, init_canvases is not None
    off, stride = su.fifo_slot_keying(S, 0)
    # the clip slot at slot 0 of sample 0 of every queue before the step of steady iteration m: read by the step noise and by the guides
    first = (lambda m: m + off) if keyed or guided else (lambda m: None)
    plan = engine.fifo_plan(sched, n_slots, queues=K, clip_first=first(0), seeded=keyed, guided=guided)
    n, s0, Bq, dev = plan.n, plan.s0, B // K, engine.device
    Lp = fifo_prompt_len(engine, pcs[0])
    pcs = [L.dev_f32(p.to(dev), "prompt canvas") for p in pcs]
    tile = (lambda t: t.repeat((1,) * (t.dim() - 2) + (K, 1)).to(dev))      # one queue's [.., B_q, S] rows, K times along the batch
    seeds_dev = seeds.to(dev)
    t0 = torch.full((Bq,), s0, dtype=torch.long, device=dev)
    z = torch.cat([Fn.canvas_noise(s, t0, (Bq,) + tuple(engine.latent_shape[1:]), plan.L) for s in noise_seeds], 0)
    sources = [_fifo_prompt_source(p, Bq, S, prompt_hop, Lp, S, 0, frac) for p in pcs]
    windows = (lambda m: torch.cat([w(m) for w in sources], 0))
    canvases = torch.empty((K, plan.outer, n_slots * sl) + plan.trailing, device=dev, dtype=torch.float32)
    # the plain deterministic batch steps as it always has; per-clip keys or guides ride on step_slots(clip_queues=K)
    kw = dict(clip_stride=stride, clip_queues=K, clip_seeds=step_seeds.to(dev) if keyed else None) if keyed or guided else {}
    if guided:
        engine.set_clip_guides(init_canvases, masks, guide_seeds=guide_seeds)
    try:
        with _slot_cfg_scope(engine, scfg):
            engine.set_prompt(windows(0))
            tail_pass = None
            if guided:      # the start, and after every shift the K entering tails, on their forward paths at s_0
                known, gmask, gseeds = engine._clips
                ab = engine.alpha_bar.to(dev, torch.float32)
                guide = dict(slot_len=sl, seeds=gseeds, everywhere=guide_start == "init")
                tails = torch.full((B, S), Fn.SLOT_LEAVE, dtype=torch.long, device=dev)
                tails[Bq - 1::Bq, S - 1] = s0
                Fn.clip_guide_slots_clips(known, torch.full((B, S), s0, dtype=torch.long, device=dev), ab, z, gmask, first=0, out=z, **guide)
                # clip slot n + m entered every queue, now that clip slot m + 1 is at its slot 0
                tail_pass = (lambda z, m: Fn.clip_guide_slots_clips(known, tails, ab, z, gmask, first=m + 1, out=z, **guide))

            def shift(new, m):
                z = engine.fifo_shift_clips(new, K, n + m, s0, seeds_dev, canvases, m)
                if tail_pass is not None:
                    tail_pass(z, m)
                return z

            _fifo_queue_loop(engine, z, plan, ([tile(t) for t in plan.ramp], [tile(t) for t in plan.steady]), n_slots, windows, first, kw,
                             lambda new, old: (new, old), shift)
    finally:
        if guided:
            engine.clear_clip_guides()
    return canvases


def _fifo_prompt_source(pc: torch.Tensor, B: int, S: int, prompt_hop: int, Lp: int, stride: int, ctx: int, frac):
    """m -> the prompt batch of the eager drivers' steady iteration m, sample k under clip slot m - ctx + k * stride: slices of the canvas
    (``fifo_prompt_windows``) on a whole hop, one ``functional.fifo_prompt_gather_frac`` launch with ``frac`` = (prompt_den,
    prompt_interp)"""
    if frac is None:
        return lambda m: fifo_prompt_windows(pc, m, B, S, prompt_hop, Lp, stride=stride, first=m - ctx)
    return lambda m: Fn.fifo_prompt_gather_frac(pc, None, B, m - ctx, stride, prompt_hop, frac[0], frac[1], Lp)


def _fifo_clip_keying(engine: DenoiseEngine, S: int, ctx: int, guided: bool = False):
    """(first, stride) of the eager drivers' ``step_slots`` calls: on an eta > 0 engine with a noise_seed, and at any eta on a
    ``guided`` queue (the clip guide reads clip positions), ``first(m)`` is the clip slot at slot 0 of sample 0 before the step of
    steady iteration m (``schedule_utils.fifo_slot_keying``); otherwise it is None, which an eta == 0 engine ignores and with which an
    unseeded eta > 0 engine is refused by ``step_slots``"""
    off, stride = su.fifo_slot_keying(S, ctx)
    if guided or (engine.eta > 0 and engine.noise_seed is not None):
        return (lambda m: m + off), stride
    return (lambda m: None), None


def _fifo_denoise_lookahead(engine: DenoiseEngine, prompt_canvas, prompt_hop: int, sched, n_slots: int, noise_seed: int, ctx: int,
                            context: Optional[torch.Tensor], frac=None) -> torch.Tensor:
    """``fifo_denoise(lookahead=ctx > 0)``: the eager loop over overlapping windows (the contract is in ``fifo_denoise``)"""
    B, S, sl = engine.embed.B, engine.slots, engine.slot_len
    h = S - ctx
    first, stride = _fifo_clip_keying(engine, S, ctx)
    plan = engine.fifo_plan(sched, n_slots, ctx, context="noise" if context is None else "clean", clip_first=first(0))
    n, s0, outer, hw, dev = plan.n, plan.s0, plan.outer, plan.trailing, engine.device
    Fn.noise_key(noise_seed, 0)
    if context is not None and not (isinstance(context, torch.Tensor) and tuple(context.shape) == (outer, ctx * sl) + hw):
        raise ValueError(f"context must be the clean latent of the {ctx} slots before the clip, shape {(outer, ctx * sl) + hw}, got "
                         f"{tuple(context.shape) if isinstance(context, torch.Tensor) else context!r}")
    Lp = fifo_prompt_len(engine, prompt_canvas)
    pc = L.dev_f32(prompt_canvas.to(dev), "prompt canvas")
    # the logical queue [outer, (ctx + n) * sl, ...]: the context, then clip slots 0 .. n - 1 keyed by their canvas positions
    t0 = torch.full((1,), s0, dtype=torch.long, device=dev)
    if context is None:
        head = Fn.canvas_noise(noise_seed, t0, (1, outer, ctx * sl) + hw, 1, window_offset=2 ** 32 - ctx * sl)[0]
    else:
        head = L.dev_f32(context.to(dev), "context")
    queue = torch.cat([head, Fn.canvas_noise(noise_seed, t0, (1, outer, n * sl) + hw, n * sl)[0]], 1)
    z = windows_from_canvas(queue, plan.L, h * sl)
    windows = _fifo_prompt_source(pc, B, S, prompt_hop, Lp, h, ctx, frac)
    engine.set_prompt(windows(0))
    canvas = torch.empty((outer, n_slots * sl) + hw, device=dev, dtype=torch.float32)

    def shift(new, m):      # the popped head goes into the clip
        z, canvas[:, m * sl:(m + 1) * sl] = engine.fifo_lookahead(new, ctx, 1, c=n + m, t=s0, seed=noise_seed)
        return z

    # a ramp step ends in the refresh of the duplicates, out of place: the stepped buffer is the next step's to write
    _fifo_queue_loop(engine, z, plan, ([t.to(dev) for t in plan.ramp], [t.to(dev) for t in plan.steady]), n_slots, windows, first,
                     dict(clip_stride=stride), lambda new, old: (engine.fifo_lookahead(new, ctx, 0)[0], new), shift)
    return canvas


def _fifo_denoise_graph(engine: DenoiseEngine, q) -> torch.Tensor:
    """``fifo_denoise``'s loop on an open queue (``DenoiseEngine.fifo_open``): per phase one eager iteration, captured pairs while
    two or more iterations are left, an odd last one eagerly — all through the cursor kernels, so the cursors count every iteration."""
    def phase(steady: bool, left: int, z, other):
        """``left`` iterations of one phase on (z, other); returns the pair with the latent first.  A ramp iteration steps z -> other,
        so the two swap; a steady one leaves the latent in z, and a replayed pair puts it back where it was either way."""
        def eager(z, other):
            (engine.fifo_steady if steady else engine.fifo_ramp)(q, z, other)
            return (z, other) if steady else (other, z)

        if left:      # every kernel of the phase runs once before it is captured
            z, other, left = *eager(z, other), left - 1
        if left >= 2:
            pair = engine.fifo_capture(q, steady, z, other)
            for _ in range(left // 2):
                pair.replay()
            left %= 2
        return eager(z, other) if left else (z, other)

    z, other = phase(False, q.n - 1, q.z, q.other)
    phase(True, q.n_slots, z, other)
    return q.clip


SAMPLERS = ("windows", "fifo")      # stream_generate(sampler=): independent / consensus windows, or the FIFO queue


# ---- what both samplers of stream_generate do around their denoising: split, encode, the mask on the canvas, decode, stitch ----
def _window_seconds(cfg: Dict) -> Tuple[float, float, float]:
    """(window, hop, crossfade) seconds of ``streaming``"""
    st = cfg.get("streaming", {})
    return float(st.get("window_seconds", 3.0)), float(st.get("hop_seconds", 1.0)), float(st.get("crossfade_seconds", 0.25))


def _prompt_windows(cfg: Dict, pc, prompt_modality: str, prompt_video, prompt_audio):
    """(chunks, zp_shape, lat): the prompt clip split into windows, the shape its encoded form has by the config, and the target's
    latent shape without the batch axis"""
    win_s, hop_s, _ = _window_seconds(cfg)
    if prompt_modality == "video":
        if prompt_video is None:
            raise ValueError("prompt_video frames required for prompt_modality=video")
        chunks = split_frames_into_windows(prompt_video, fps=pc.fps, win_s=win_s, hop_s=hop_s)[0]
        zp_shape = (chunks.shape[0], pc.Cv, chunks.shape[1] // pc.t_down, chunks.shape[2] // pc.s_down, chunks.shape[3] // pc.s_down)
        return chunks, zp_shape, (pc.Ca, pc.Fa)
    if prompt_audio is None:
        raise ValueError("prompt_audio required for prompt_modality=audio")
    chunks = split_audio_into_windows(prompt_audio, sr=pc.sr, win_s=win_s, hop_s=hop_s)[0]
    T_in = int(round(cfg["data"]["clip_seconds"] * pc.fps))
    return chunks, (chunks.shape[0], pc.Ca, pc.Fa), (pc.Cv, max(1, T_in // pc.t_down), pc.H // pc.s_down, pc.W // pc.s_down)


def _init_windows(cfg: Dict, pc, init: Optional[np.ndarray], n_windows: int) -> Optional[np.ndarray]:
    """the init clip split into windows like the prompt (None without one); it must give the prompt's number of windows"""
    if init is None:
        return None
    win_s, hop_s, _ = _window_seconds(cfg)
    split = split_frames_into_windows if pc.target == "video" else split_audio_into_windows
    init_chunks = split(init, pc.fps if pc.target == "video" else pc.sr, win_s, hop_s)[0]
    if init_chunks.shape[0] != n_windows:
        raise ValueError(f"the init clip splits into {init_chunks.shape[0]} windows, the prompt into {n_windows}: they must cover "
                         "the same long clip")
    return init_chunks


def _canvas_mask(mask, lat, n_windows: int, hop: int, L_: int) -> torch.Tensor:
    """``mask`` checked and expanded to the target's latent canvas [C, P, H, W] / [Ca, P], P = (n_windows - 1) * hop + L (CPU float32)"""
    if lat[1] != L_:
        raise ValueError(f"mask: the target latent has {lat[1]} positions along its sliding axis (data.clip_seconds), a window of "
                         f"streaming.window_seconds has {L_}: they must be equal")
    mask_canvas_shape = (lat[0], (n_windows - 1) * hop + L_) + tuple(lat[2:])
    mc = torch.as_tensor(mask).detach().to("cpu", torch.float32)
    try:
        mc = mc.expand(mask_canvas_shape)
    except RuntimeError:
        raise ValueError(f"mask shape {tuple(mc.shape)} does not broadcast to the latent canvas {mask_canvas_shape}") from None
    if not bool(((mc >= 0) & (mc <= 1)).all()):
        raise ValueError("mask values must lie in [0, 1]")
    return mc


def _encode_windows(modality: str, vid_vae, aud_codec, chunks: np.ndarray, device) -> torch.Tensor:
    return P.encode_video(vid_vae, chunks, device) if modality == "video" else P.encode_audio(aud_codec, chunks, device)


def _encode_init(target: str, vid_vae, aud_codec, init_chunks: np.ndarray, device, want) -> torch.Tensor:
    """the init clip's windows encoded as one batch: contiguous float32 of the target's window shape ``want``"""
    known = _encode_windows(target, vid_vae, aud_codec, init_chunks, device).float().contiguous()
    if tuple(known.shape) != tuple(want):
        raise ValueError(f"the init clip encodes to windows of shape {tuple(known.shape)}, the target's are {tuple(want)}")
    return known


def _decode_windows(cfg: Dict, pc, vid_vae, aud_codec, lat, z: torch.Tensor, device) -> torch.Tensor:
    """finished latents of some windows -> what the stitcher takes: waveforms [n, L] float32 or frames [n, T, H, W, 3] uint8"""
    if pc.target == "audio":
        if z.shape[0] == 0:
            hop_a = int(getattr(aud_codec, "hop", 0)) or int(round(pc.sr * float(cfg["data"]["clip_seconds"]))) // pc.Fa
            return torch.empty(0, pc.Fa * hop_a, device=device)
        return aud_codec.decode(z)[:, 0, :].contiguous()
    if z.shape[0] == 0:
        return torch.empty(0, lat[1] * pc.t_down, lat[2] * pc.s_down, lat[3] * pc.s_down, 3, dtype=torch.uint8, device=device)
    x = vid_vae.decode(z).clamp(0, 1)                                         # [n,3,T,H,W]
    return (x.permute(0, 2, 3, 4, 1) * 255.0).to(torch.uint8).contiguous()    # as the reference's astype(np.uint8)


def _stitch(cfg: Dict, pc, out: torch.Tensor) -> Dict:
    """the decoded windows cross-faded into the result dict"""
    _, hop_s, xfade_s = _window_seconds(cfg)
    if pc.target == "audio":
        w = torch.from_numpy(audio_fade_window(out.shape[1], int(round(pc.sr * xfade_s))))
        return {"audio": crossfade_tensor(out, w, int(round(pc.sr * hop_s))).cpu().numpy(), "sr": pc.sr}
    w = torch.from_numpy(video_fade_window(out.shape[1], int(round(xfade_s * pc.fps))))
    return {"video": crossfade_tensor(out, w, int(round(pc.fps * hop_s))).cpu().numpy(), "fps": pc.fps}


# ---- stream_generate(sampler="fifo"): the FIFO queue behind the pipeline's front end ----
class FifoGeometry(NamedTuple):
    """``fifo_geometry``'s result: latent positions and slots of a long clip run through the FIFO queue"""
    hop_t: int          # the target's hop and window length in latent positions (``latent_hop``)
    L_t: int
    hop_p: int          # the prompt's
    L_p: int
    slot_len: int       # latent positions per slot: the tube's t (video target) or the chunk length (audio target)
    S: int              # slots per sample; the engine's sliding length is S * slot_len <= L_t
    prompt_hop: int     # prompt positions per target slot; with ``prompt_den`` > 1 the numerator of the reduced fraction
    h: int              # stepping slots per sample, S - lookahead
    B: int              # the engine's batch, steps // h
    P: int              # the target canvas' positions, (n_windows - 1) * hop_t + L_t
    n_slots: int        # ceil(P / slot_len): the queue runs whole slots, the canvas is cropped to P
    P_p: int            # the prompt canvas' positions
    prompt_den: int = 1 # the denominator of the prompt hop (> 1 only under ``fifo_geometry(prompt_interp=)``)

    @property
    def clips(self) -> int:
        """K, the clips queued in lockstep in one engine: 1 here, K on the ``FifoClipsGeometry`` of ``fifo_geometry(clips=K)``"""
        return 1


class FifoClipsGeometry(FifoGeometry):
    """``fifo_geometry(clips=K)``'s result for K > 1: one clip's ``FifoGeometry`` with ``B`` the whole engine's batch, K times one
    queue's, and ``clips`` = K (an attribute beside the tuple's fields, which keep their order and number)."""
    clips = 1

    def __new__(cls, geo: FifoGeometry, clips: int):
        self = super().__new__(cls, *geo._replace(B=clips * geo.B))
        self.clips = clips
        return self


def fifo_geometry(cfg: Dict, prompt_modality: str, n_windows: int, steps: int, lookahead: int = 0,
                  prompt_interp: Optional[str] = None, clips: int = 1) -> FifoGeometry:
    """The geometry of ``stream_generate(sampler="fifo")`` from the config alone (no device): how ``n_windows`` windows of
    ``streaming.window_seconds`` / ``hop_seconds`` become a target canvas of P latent positions, a queue of samples of S slots and a
    prompt canvas the queue's prompt gather walks by whole positions.  ``steps`` is the length of the schedule the queue will run (after
    any truncation by ``strength``).  ValueError, naming the numbers, where the config does not fit the queue.
    ``prompt_interp`` ("nearest" or "linear"; default None) admits a prompt with a fractional number of positions per target slot
    (include/avdiff_hip.h, "fractional prompt hop"): the hop L_p * slot_len / L_t comes back reduced, ``prompt_hop`` its numerator and
    ``prompt_den`` its denominator — a video prompt at the shipped geometry is 12 * 4 / 150 = 8 / 25.  Without a mode such a prompt
    is refused.
    ``clips`` = K >= 1 (default 1) is the number of equally long clips queued in lockstep in one engine (``fifo_denoise_clips``): the
    result carries it and ``B`` is K times one queue's batch; every other number is one clip's."""
    if prompt_modality not in ("video", "audio"):
        raise ValueError("prompt_modality must be 'video' or 'audio'")
    if prompt_interp is not None and prompt_interp not in Fn.PROMPT_INTERPS:
        raise ValueError(f"prompt_interp must be None or one of {Fn.PROMPT_INTERPS}, got {prompt_interp!r}")
    target = "audio" if prompt_modality == "video" else "video"
    for name, v, lo in (("n_windows", n_windows, 1), ("steps", steps, 1), ("lookahead", lookahead, 0), ("clips", clips, 1)):
        if isinstance(v, bool) or not isinstance(v, int) or v < lo:
            raise ValueError(f"{name} must be an int >= {lo}, got {v!r}")
    hop_t, L_t = latent_hop(cfg, target)
    hop_p, L_p = latent_hop(cfg, prompt_modality)
    if target == "video":
        slot_len = P.tube_from_config(cfg)[0]
    else:
        chunk = cfg["tokenizer"]["audio"]["chunk"]
        slot_len, stride = int(chunk["length"]), int(chunk["stride"])
        if stride != slot_len:
            raise ValueError(f"the audio chunk has length {slot_len} and stride {stride}: a queue slot is one chunk, so the FIFO sampler "
                             "needs non-overlapping chunks (stride == length)")
    S = L_t // slot_len
    if S < 1:
        raise ValueError(f"a window of {L_t} latent positions holds no slot of {slot_len}: the FIFO sampler needs at least one")
    if (L_p * slot_len) % L_t and prompt_interp is None:
        raise ValueError(f"the prompt has {L_p * slot_len / L_t:g} latent positions per target slot ({L_p} per window of {L_t} target "
                         f"positions, slots of {slot_len}); the queue's prompt gather moves by whole positions")
    g = math.gcd(L_p * slot_len, L_t)
    prompt_hop, prompt_den = L_p * slot_len // g, L_t // g
    if not lookahead < S:
        raise ValueError(f"lookahead {lookahead} must be below the S = {S} slots of a sample")
    h = S - lookahead
    if steps % h:
        raise ValueError(f"{steps} steps do not fill a queue of samples with {h} stepping slots (S = {S}, lookahead {lookahead}): the "
                         f"nearest step counts are {steps // h * h} and {(steps // h + 1) * h}")
    P_ = (n_windows - 1) * hop_t + L_t
    geo = FifoGeometry(hop_t, L_t, hop_p, L_p, slot_len, S, prompt_hop, h, steps // h, P_, -(-P_ // slot_len),
                       (n_windows - 1) * hop_p + L_p, prompt_den)
    return geo if clips == 1 else FifoClipsGeometry(geo, clips)


def _fifo_options(cfg: Dict, *, shard, consensus, noise_keying, resample, init_noise, fifo) -> dict:
    """What ``stream_generate(sampler="fifo")`` refuses, before anything is read or encoded, and its ``fifo`` options ({"steps":
    None = the target's sampler_steps, "lookahead": 0, "graph": False, "prompt_interp": None, "apg_momentum": None}; the argument
    wins over ``streaming.fifo``)."""
    st = cfg.get("streaming", {})
    if shard:
        raise ValueError("sampler='fifo' with shard=True is not implemented: the queue is one chain of steps on one device")
    if (consensus if consensus is not None else st.get("latent_consensus")) not in (None, False):
        raise ValueError("sampler='fifo' takes no consensus: the queue generates one latent canvas, there are no windows to average")
    if (noise_keying if noise_keying is not None else st.get("noise_keying", "sample")) == "canvas":
        raise ValueError("sampler='fifo' takes no noise_keying='canvas': that keys the windows' step noise, the queue keys its own by "
                         "clip slot")
    if su.check_resample(resample) or su.resample_from_config(cfg["sampling"]):
        raise ValueError("sampler='fifo' takes no resample: a queue slot moves down the schedule one level per step and cannot jump back")
    if init_noise is not None:
        raise ValueError("sampler='fifo' takes no init_noise: the queue starts from the canvas-keyed noise stream of seed")
    opts = fifo if fifo is not None else st.get("fifo")
    opts = {} if opts is None else opts
    if not isinstance(opts, dict) or set(opts) - {"steps", "lookahead", "graph", "prompt_interp", "apg_momentum"}:
        raise ValueError(f"fifo takes a dict with any of steps, lookahead and graph, or prompt_interp, or apg_momentum, got {opts!r}")
    opts = dict({"steps": None, "lookahead": 0, "graph": False, "prompt_interp": None, "apg_momentum": None}, **opts)
    if opts["apg_momentum"] is not None:      # the slot APG momentum (fifo_denoise(apg_momentum=)): a finite number, not a bool
        opts["apg_momentum"] = Fn.apg_params(momentum=opts["apg_momentum"])[2]
    if opts["steps"] is not None and (isinstance(opts["steps"], bool) or not isinstance(opts["steps"], int) or opts["steps"] < 1):
        raise ValueError(f"fifo['steps'] must be an int >= 1 or None, got {opts['steps']!r}")
    if isinstance(opts["lookahead"], bool) or not isinstance(opts["lookahead"], int) or opts["lookahead"] < 0:
        raise ValueError(f"fifo['lookahead'] must be an int >= 0, got {opts['lookahead']!r}")
    if opts["graph"] is not None and not isinstance(opts["graph"], bool):
        raise ValueError(f"fifo['graph'] must be True, False or None, got {opts['graph']!r}")
    if opts["prompt_interp"] is not None and not (isinstance(opts["prompt_interp"], str) and opts["prompt_interp"] in Fn.PROMPT_INTERPS):
        raise ValueError(f"fifo['prompt_interp'] must be None or one of {Fn.PROMPT_INTERPS}, got {opts['prompt_interp']!r}")
    return opts


def _fifo_slot_controls(pc, opts: dict, T_train: int) -> dict:
    """the config's per-sample CFG controls as ``fifo_denoise``'s slot controls (a queue sample holds S noise levels)"""
    ctl = {}
    if pc.interval is not None:
        ctl["guidance_by_level"] = su.guidance_interval_table(pc.guidance, pc.interval, T_train)
    if pc.rescale != 0.0:
        ctl["rescale_by_level"] = pc.rescale
    if pc.apg is not None:
        if pc.apg[2] != 0.0:
            raise ValueError(f"sampling.apg momentum {pc.apg[2]:g} is the per-sample buffer's and gives the FIFO queue no slot momentum "
                             "(that buffer does not travel with a slot through the shift): set it to 0 and use "
                             "streaming.fifo.apg_momentum (fifo={'apg_momentum': beta})")
        ctl["apg"] = {"norm_threshold": pc.apg[0], "eta_parallel": pc.apg[1]}
    if opts["apg_momentum"] is not None:
        if pc.apg is None:
            raise ValueError(f"fifo['apg_momentum'] {opts['apg_momentum']:g} needs sampling.apg for the target: the momentum is adaptive "
                             "projected guidance's")
        ctl["apg_momentum"] = opts["apg_momentum"]
    return ctl


def _one_canvas(windows: torch.Tensor, hop: int) -> torch.Tensor:
    """windows encoded alone disagree on their overlaps: one uniform consensus pass, then the canvas"""
    return canvas_from_windows(Fn.window_consensus(windows, hop), hop)


def _fifo_prompt_canvas(pc, mods: Dict, device, prompt_modality: str, chunks: np.ndarray, geo: FifoGeometry):
    """(the prompt canvas of one clip's chunks, its prompt token count): the encoder's own output decides the count, as in the windows
    sampler"""
    z_p = _encode_windows(prompt_modality, mods["vid_vae"], mods["aud_codec"], chunks, device)
    n_prompt = P.prompt_tokens(pc, tuple(z_p.shape))
    if z_p.shape[2] != geo.L_p:
        raise ValueError(f"encoded prompt windows have {z_p.shape[2]} latent positions, the config implies {geo.L_p}: the prompt "
                         "canvas cannot be laid out")
    return _one_canvas(z_p.float().contiguous(), geo.hop_p), n_prompt


def _fifo_engine(pc, mods: Dict, geo: FifoGeometry, lat, n_prompt: int, noise_seed) -> DenoiseEngine:
    """the engine of a queue geometry.  The per-sample CFG controls stay off it: a queue sample holds S noise levels, and
    ``_fifo_slot_controls`` gives their slot form"""
    return P.build_engine(pc._replace(rescale=0.0, interval=None, apg=None), adapt_v=mods["adapt_v"], adapt_a=mods["adapt_a"],
                          core=mods["core"], head=mods["head"], tstep_dim=mods["tstep_dim"],
                          latent_shape=(geo.B, lat[0], geo.S * geo.slot_len) + tuple(lat[2:]), n_prompt=n_prompt, noise_seed=noise_seed)


def _fifo_result(cfg: Dict, pc, mods: Dict, device, lat, geo: FifoGeometry, canvas: torch.Tensor, return_latents: bool,
                 max_windows_per_batch: int) -> Dict:
    """the result dict of one finished latent canvas: its windows decoded in batches and cross-faded as the windows sampler's are"""
    windows = windows_from_canvas(canvas, geo.L_t, geo.hop_t)
    out = torch.cat([_decode_windows(cfg, pc, mods["vid_vae"], mods["aud_codec"], lat, windows[lo:lo + max_windows_per_batch], device)
                     for lo in range(0, windows.shape[0], max_windows_per_batch)], 0)
    res = _stitch(cfg, pc, out)
    if return_latents:
        res["latents"], res["latent_canvas"] = windows.cpu().numpy(), canvas.cpu().numpy()
    return res


def _stream_generate_fifo(cfg: Dict, pc, mods: Dict, device, prompt_modality: str, chunks: np.ndarray, zp_shape, lat, init_chunks,
                          mask, strength: float, opts: dict, *, seed, noise_seed, guide_seed, return_latents: bool,
                          max_windows_per_batch: int) -> Dict:
    """``stream_generate(sampler="fifo")`` after the common checks and splits (the contract is in ``stream_generate``): the prompt
    windows become one prompt canvas, ``fifo_denoise`` generates the target canvas, and its windows are decoded and cross-faded as the
    windows sampler's are."""
    Nw, T_train = zp_shape[0], int(pc.alpha_bar.numel())
    whole = su.make_sampling_schedule(T_train, opts["steps"]) if opts["steps"] is not None else pc.sched
    sched = su.truncate_schedule(whole, strength) if init_chunks is not None and strength < 1.0 else whole
    n = int(sched.numel()) - 1
    # strength 0 runs no step: the geometry is then checked for the whole schedule
    geo = fifo_geometry(cfg, prompt_modality, Nw, n or int(whole.numel()) - 1, opts["lookahead"], opts["prompt_interp"])
    if lat[1] != geo.L_t:
        raise ValueError(f"the target latent has {lat[1]} positions along its sliding axis (data.clip_seconds), a window of "
                         f"streaming.window_seconds has {geo.L_t}: they must be equal")
    ctl = _fifo_slot_controls(pc, opts, T_train)
    mc = None if mask is None else _canvas_mask(mask, lat, Nw, geo.hop_t, geo.L_t)
    init_canvas = None
    if init_chunks is not None:
        init_canvas = _one_canvas(_encode_init(pc.target, mods["vid_vae"], mods["aud_codec"], init_chunks, device, (Nw, *lat)), geo.hop_t)
    if n == 0:                                     # strength 0: no steps, the known canvas
        canvas = init_canvas
    else:
        prompt_canvas, n_prompt = _fifo_prompt_canvas(pc, mods, device, prompt_modality, chunks, geo)
        eng = _fifo_engine(pc, mods, geo, lat, n_prompt, noise_seed)
        if seed is None:                           # once, from torch's global CPU generator: torch.manual_seed governs it
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        guide = {}
        if init_canvas is not None:
            sdedit = strength < 1.0
            guide = dict(init_canvas=init_canvas, mask=mc if mc is not None else (torch.zeros(1) if sdedit else None),
                         guide_seed=P.default_guide_seed(guide_seed, noise_seed), guide_start="init" if sdedit else "noise",
                         guided_shift=True)
        canvas = fifo_denoise(eng, prompt_canvas, geo.prompt_hop, sched, geo.n_slots, int(seed), graph=opts["graph"],
                              lookahead=opts["lookahead"], prompt_den=geo.prompt_den, prompt_interp=opts["prompt_interp"], **guide,
                              **ctl)[:, :geo.P].contiguous()
    return _fifo_result(cfg, pc, mods, device, lat, geo, canvas, return_latents, max_windows_per_batch)


def _fifo_clips_refusals(cfg: Dict, opts: dict, K: int, has_init: bool, has_mask: bool, noise_seed=None) -> None:
    """What ``stream_generate(sampler="fifo")`` refuses of a LIST of prompt clips, before anything is read or encoded: the limits of
    ``fifo_denoise_clips`` (``opts``: ``_fifo_options``' result).  ``noise_seed``: a list of K ints keys the step noise per clip
    (``fifo_denoise_clips(step_seeds=)``) and admits ``sampling.ddim_eta`` > 0; an int or None does not"""
    if K < 1:
        raise ValueError("a list of prompt clips needs at least one clip, got an empty one")
    if has_init or has_mask:
        raise ValueError("a list of prompt clips takes no init clip or mask: the clip guide is one canvas walked by one queue, and the "
                         "clips share an engine (run a guided clip on its own)")
    eta = float(cfg["sampling"].get("ddim_eta", 0.0))
    if isinstance(noise_seed, (list, tuple)):
        Fn.clip_seeds(noise_seed, K)      # one step seed per clip, each a seed of the stream
    elif eta > 0:
        raise ValueError(f"a list of prompt clips needs sampling.ddim_eta == 0 (got {eta:g}): the queue's step noise has one seed and one "
                         "clip-position walk per call, so the clips would draw the same step normals; a noise_seed list of one int per "
                         "clip keys the step noise per clip")
    if opts["graph"]:
        raise ValueError("a list of prompt clips runs the plain eager queue: fifo['graph'] True is refused (the replayed queue's device "
                         "cursors and clip canvas serve one clip)")
    if opts["lookahead"]:
        raise ValueError(f"a list of prompt clips runs the plain eager queue: fifo['lookahead'] {opts['lookahead']} is refused (the "
                         "lookahead move has no multi-queue form)")


def _stream_generate_fifo_clips(cfg: Dict, pc, mods: Dict, device, prompt_modality: str, clips, opts: dict, *, seed, noise_seed,
                                return_latents: bool, max_windows_per_batch: int) -> list:
    """``stream_generate(sampler="fifo")`` with a list of K prompt clips (the contract is in ``stream_generate``): every clip is split,
    encoded and made a prompt canvas as a single clip is, one engine of batch K * B runs ``fifo_denoise_clips``, and every canvas is
    decoded and cross-faded as a single clip's is.  Returns the K result dicts."""
    K, T_train = len(clips), int(pc.alpha_bar.numel())
    shapes = [tuple(np.shape(c)) for c in clips]
    if any(s != shapes[0] for s in shapes):
        raise ValueError(f"the prompt clips of a list must have equal length (the queues run in lockstep), got shapes {shapes}")
    if isinstance(seed, (list, tuple)):
        if len(seed) != K:
            raise ValueError(f"seed lists {len(seed)} seeds for {K} prompt clips: one per clip, or one int (clip k then takes seed + k)")
        seeds = [s for s in seed]
    else:
        if seed is None:                               # once, from torch's global CPU generator: torch.manual_seed governs it
            seed = int(torch.randint(0, 2 ** 62, (1,)).item())
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise ValueError(f"seed must be an int, a list of {K} ints or None, got {seed!r}")
        seeds = [seed + k for k in range(K)]
    Fn.clip_seeds(seeds, K)
    split = [_prompt_windows(cfg, pc, prompt_modality, c if prompt_modality == "video" else None,
                             c if prompt_modality == "audio" else None) for c in clips]
    chunks0, zp_shape, lat = split[0]
    Nw = zp_shape[0]
    sched = su.make_sampling_schedule(T_train, opts["steps"]) if opts["steps"] is not None else pc.sched
    geo = fifo_geometry(cfg, prompt_modality, Nw, int(sched.numel()) - 1, 0, opts["prompt_interp"], clips=K)
    if lat[1] != geo.L_t:
        raise ValueError(f"the target latent has {lat[1]} positions along its sliding axis (data.clip_seconds), a window of "
                         f"streaming.window_seconds has {geo.L_t}: they must be equal")
    ctl = _fifo_slot_controls(pc, opts, T_train)
    prompts = [_fifo_prompt_canvas(pc, mods, device, prompt_modality, chunks, geo) for chunks, _, _ in split]
    # a noise_seed list is the K clips' step seeds: the engine's own seed (which the SDE solver asks for at construction) is not read
    step_seeds = list(noise_seed) if isinstance(noise_seed, (list, tuple)) else None
    eng = _fifo_engine(pc, mods, geo, lat, prompts[-1][1], noise_seed if step_seeds is None else step_seeds[0])
    canvases = fifo_denoise_clips(eng, [c for c, _ in prompts], geo.prompt_hop, sched, geo.n_slots, seeds, prompt_den=geo.prompt_den,
                                  prompt_interp=opts["prompt_interp"], step_seeds=step_seeds, **ctl)
    return [_fifo_result(cfg, pc, mods, device, lat, geo, canvases[k, :, :geo.P].contiguous(), return_latents, max_windows_per_batch)
            for k in range(K)]


@torch.no_grad()
def stream_generate(*, cfg: Dict, vid_vae, aud_codec, adapt_v, adapt_a, core, head, tstep_dim: int, prompt_modality: str,
                    prompt_video: Optional[np.ndarray], prompt_audio: Optional[np.ndarray], device: torch.device,
                    init_noise: Optional[torch.Tensor] = None, max_windows_per_batch: int = 32, shard: bool = False,
                    seed: Optional[int] = None, comm_device: Optional[torch.device] = None,
                    noise_seed: Optional[int] = None, guidance_interval=None, consensus=None,
                    return_latents: bool = False, noise_keying: Optional[str] = None, init_video: Optional[np.ndarray] = None,
                    init_audio: Optional[np.ndarray] = None, strength: float = 1.0, mask=None,
                    guide_seed: Optional[int] = None, resample=None, sampler: Optional[str] = None,
                    fifo: Optional[dict] = None) -> Optional[Dict[str, np.ndarray]]:
    """The body of the reference's ``main()`` (stream_infer.py:146-225) minus file I/O, with all windows batched.

    Returns {"audio": wav, "sr"} for a video prompt or {"video": frames uint8, "fps"} for an audio prompt.
    ``init_noise`` [N_windows, *latent] fixes the initial latents (the reference draws them window by window); ``seed`` draws them
    from a CPU generator for the WHOLE window list instead (the same numbers whatever the number of ranks).  ``noise_seed`` does the
    same for the per-step DDIM noise of ``sampling.ddim_eta`` > 0 (default None: the reference's per-step ``randn_like`` from the device
    generator): window i draws its noise as sample i of the seeded stream (DenoiseEngine ``noise_seed`` / ``sample_offset``), whatever
    batch or rank steps it.  ``sampling.solver: dpmpp_2m`` with ``ddim_eta`` > 0 runs the solver's SDE form (SDE-DPM-Solver++(2M)) on
    the same stream; it draws seeded noise only, so it needs ``noise_seed``.

    ``shard=True`` (every rank of the default process group calls this with the same arguments; one process per GPU): rank 0 encodes
    the prompt windows, ONE broadcast (``dist.broadcast_conditioning``; over ``comm_device``, default: ``device`` for the nccl = RCCL
    backend, the CPU for gloo) hands them to all ranks, rank r steps windows ``dist.shard_range(N_windows, r, world)`` and decodes them
    (``vid_vae.decode`` -> uint8 frames / ``aud_codec.decode`` -> waveform: per rank N_windows / world loops AND decodes — the decode is
    8 ms per 256 x 256 window against 14 ms for its 50-step loop, so leaving it on one rank would cap an 8-rank run near 2x), one
    gather brings the decoded windows to rank 0, which stitches and returns the result — the other ranks return None.
    If rank 0 fails before the broadcast (encode error, a prompt shape the config does not imply), every rank raises.
    Windows never interact inside the loop or the decode, so the stitched output equals the single-process one bit for bit as long as
    both runs take the same kernels (the matrix-pipe mode "auto" switches kernels at 2,048 / 6,144 rows: fix ``core.matmul`` to
    compare across sizes).  With ``ddim_eta`` > 0 this holds when ``noise_seed`` is set (then also for any ``max_windows_per_batch``);
    without it every rank draws from its own device generator.
    ``guidance_interval`` (default None) or ``sampling.guidance_interval`` (per modality, [t_lo, t_hi]; the argument wins): guidance
    on the steps with t_lo <= t_now <= t_hi only, cond-only steps elsewhere (DenoiseEngine ``guidance_interval``).
    ``sampling.apg`` (per modality, a dict of norm_threshold / eta_parallel / momentum; default none): adaptive projected guidance in
    place of the CFG combine on every window's engine (DenoiseEngine ``apg``).  Every window is its own sample — its coefficients and
    its momentum buffer depend on that window alone, also under a consensus — so any ``max_windows_per_batch`` and ``shard`` give the
    same windows.
    ``consensus`` (default None = independent windows, today's output; else ``streaming.latent_consensus``, the argument wins):
    "uniform" or a table of L weights > 0 (L latent positions per window, ``latent_hop``) switches latent window consensus on: the
    windows are views of one latent canvas and after every step each canvas position under several windows becomes their weighted
    mean in all of them (DenoiseEngine ``set_window_consensus``), so the finished latents agree on every overlap.  The initial
    latents must agree there too (the first mean would shrink the noise otherwise): ``seed`` draws one canvas from the CPU generator
    and crops it, no seed draws the canvas on the device, and a caller's ``init_noise`` keeps its [N_windows, *latent] shape and must
    be windows of a canvas (``windows_from_canvas``).  Up to ``max_windows_per_batch`` windows are one engine, run as without
    consensus; more are several engines stepped in lock-step (eager) with one consensus pass over all windows per step; the latents
    are the same bits either way where the engines take the same kernels.  Decode and stitching are unchanged: every window is
    decoded on its own and cross-faded, now over near-identical content.  Needs ``shard=False``: windows on different ranks would need
    a halo exchange of their overlaps after every step, which is not implemented.  With the default noise keying it also needs
    ``ddim_eta`` == 0: windows draw independent noise, and the mean over an overlap would shrink its variance.
    ``noise_keying`` (default None = ``streaming.noise_keying``, else "sample"; the argument wins): "canvas" keys the per-step noise
    (DDIM's, or that of solver "dpmpp_2m" at ``ddim_eta`` > 0) by canvas position instead of by window (DenoiseEngine ``noise_keying``; include/avdiff_hip.h, "canvas-keyed noise"), so
    every window draws the same normal at a shared position and the consensus leaves the noise term intact: stochastic sampling
    (``ddim_eta`` > 0) under consensus.  It needs consensus on and ``noise_seed``; the engines are built with ``canvas_hop`` =
    ``latent_hop`` and ``sample_offset`` = their first window, so the latents are the same bits for any ``max_windows_per_batch``
    where the engines take the same kernels.  ``shard=True`` stays refused.
    ``return_latents`` adds "latents": the finished [N_windows, *latent] float32 latents (single process only).
    ``init_video`` (uint8 [T_total,H,W,3], audio->video) / ``init_audio`` (float waveform, video->audio), ``strength``, ``mask``,
    ``guide_seed`` (the defaults change nothing): the latent guide of ``sample_one_direction`` — inpainting, outpainting, SDEdit —
    applied to the whole long clip.  The init clip is split into windows like the prompt (it must give the same number of windows)
    and the windows are encoded as one batch.  ``mask`` lives on the target's latent canvas ([C,P,H,W] / [Ca,P] with P = (N_windows -
    1)*hop + L latent positions, ``latent_hop``; or anything that broadcasts to it; values in [0, 1], 1 = keep; ``canvas_frame_mask``)
    and is cut into per-window masks with ``windows_from_canvas``.  ``strength`` < 1 runs the tail of the schedule from the encoded
    windows noised to that point (``truncate_schedule``; 0 returns the decoded known windows, stitched); without a mask the guide is
    cleared after the start and the whole latent is free, as in ``sample_one_direction``.  ``guide_seed`` keys the clip's forward
    noise (default ``noise_seed``, else 0).  Without consensus the windows stay independent: window i is sample i of the per-sample
    known-noise stream, whatever ``max_windows_per_batch``.  With consensus the encoded windows, which disagree on their overlaps
    because each was encoded alone, are first made one canvas (one ``window_consensus`` pass with the consensus weights), and the
    engines hold them with the known noise keyed by canvas position (DenoiseEngine ``set_known(keying="canvas", hop=latent_hop)``;
    include/avdiff_hip.h, "canvas-keyed known noise"), window offset = the engine's first window: a held region stays on its forward
    path through every consensus mean and the finished latents equal the known canvas there, for any ``max_windows_per_batch``.
    ``ddim_eta`` > 0 needs ``noise_seed`` (and under consensus ``noise_keying="canvas"``), as without a guide.  An init clip with
    ``shard=True`` is refused: the known windows would need a second broadcast, which is not implemented.
    ``resample`` (default None) = (jump, resamples), or ``sampling.resample: {jump:, resamples:}`` (the argument wins): RePaint
    resampling as in ``sample_one_direction`` — the schedule, truncated by ``strength`` first, is expanded with
    ``schedule_utils.resample_schedule`` and every up-jump is a seeded forward jump of all windows (DenoiseEngine ``renoise``).  It needs
    an init clip with a ``mask``, and ``noise_seed``.  Without consensus window i draws its renoise normals as sample i; with
    consensus they are keyed by canvas position like the guide's known noise (window offset = the engine's first window), so every
    window draws the same normals at a shared position: agreeing windows still agree after a jump, no consensus pass follows it, and
    the latents are the same bits for any ``max_windows_per_batch`` where the engines take the same kernels.
    ``sampler`` (default None = ``streaming.sampler``, else "windows"; the argument wins): "windows" is everything above; "fifo"
    generates the clip with FIFO diagonal denoising (``fifo_denoise``) behind the same front end.  The prompt windows are split and
    encoded as above and made ONE prompt canvas (a uniform ``window_consensus`` pass, since each window was encoded alone, then
    ``canvas_from_windows``); one engine of batch B runs the queue over the target canvas of P = (N_windows - 1)*hop + L latent
    positions (``fifo_geometry`` gives every number and refuses a config that does not fit: the audio chunks must not overlap, the
    prompt must have a whole number of latent positions per target slot unless ``fifo["prompt_interp"]`` is set, and the step count
    must be a multiple of the S - lookahead stepping slots of a sample); the canvas is cut into the windows' latents (``windows_from_canvas``), which are decoded in batches of
    ``max_windows_per_batch`` and cross-faded as above, so the output has the windows sampler's length and dtype.
    ``fifo`` (or ``streaming.fifo``; the argument wins) = {"steps": the target's ``sampler_steps``, "lookahead": 0, "graph": False,
    "prompt_interp": None, "apg_momentum": None}, ``fifo_denoise``'s arguments; unknown keys are refused.  ``apg_momentum`` (a finite
    number; needs ``sampling.apg`` for the target) is APG's momentum per slot, carried with the slot through the queue
    (include/avdiff_hip.h, "slot APG momentum").  ``prompt_interp`` "nearest" or "linear" admits a
    prompt with a fractional number of latent positions per target slot (include/avdiff_hip.h, "fractional prompt hop"; a video prompt
    at the shipped geometry: 8 / 25): ``fifo_geometry`` reduces the hop and ``fifo_denoise`` walks it, reading between two prompt
    positions by the nearest row or by an fp32 blend of the two.  The choice is the user's: which conditions a trained model better
    cannot be measured on synthetic weights.  None keeps the refusal of such a prompt.
    ``seed`` seeds the queue's start and entering noise (None: drawn once from torch's global CPU generator), ``noise_seed`` the engine's step noise (``ddim_eta`` > 0 needs it).  The config's solver, eta and
    guidance go to the engine; its per-sample CFG controls become ``fifo_denoise``'s slot controls: the guidance interval a
    ``guidance_interval_table``, ``guidance_rescale`` a constant ``rescale_by_level``, ``sampling.apg`` the per-slot APG (its own momentum
    key != 0 is refused: that is the per-sample buffer; the queue's is ``fifo["apg_momentum"]``).  An init clip is made one canvas like the prompt and guides the queue (``init_canvas``):
    ``mask`` is passed whole, ``strength`` < 1 truncates the schedule (the truncated length must still divide) and starts every
    position from the clip (``guide_start="init"``; without a mask everything is free afterwards), ``strength`` 0 returns the decoded
    known canvas.  The entering slots are guided inside the shift's launch (``guided_shift=True``).  It runs eagerly on the plain queue:
    ``fifo_denoise`` refuses it with ``graph`` True or a ``lookahead``.  Refused, before anything is encoded: ``shard=True``,
    ``consensus``, ``noise_keying="canvas"``, ``resample`` and ``init_noise``.
    ``return_latents`` adds "latents", the [N_windows, *latent] windows of the canvas, and "latent_canvas" [C, P, H, W] / [Ca, P].
    A LIST or tuple of K prompt clips of equal length in ``prompt_video`` / ``prompt_audio`` (``sampler="fifo"`` only) generates K clips
    at once (``fifo_denoise_clips``; include/avdiff_hip.h, "FIFO clip batch"): every clip is split, encoded and made a prompt canvas as
    above, one engine of batch K * B (``fifo_geometry(clips=K)``) runs the K queues in lockstep, one model call finishing one slot of
    every clip, and every canvas is decoded and cross-faded as above.  The result is a list of K dicts of the single clip's kind
    (``return_latents`` adds each clip's "latents" and "latent_canvas").  ``seed`` is then a list of K ints, one per clip, or one int
    (or None, drawn as above) from which clip k takes seed + k; equal seeds give correlated starts.  Refused with a list, before
    anything is encoded: an init clip or mask (the pipeline encodes one init clip; ``fifo_denoise_clips(init_canvases=)`` guides K
    clips from K latent canvases), ``sampling.ddim_eta`` > 0 under an int ``noise_seed`` or none (the step noise would have one seed
    and one clip-position walk per call), ``fifo["graph"]`` True and a nonzero ``fifo["lookahead"]`` (the clip batch is the plain
    eager queue).  ``noise_seed`` may be a LIST of K ints with a list of clips: clip k then draws its ``ddim_eta`` > 0 step noise under
    ``noise_seed[k]`` (``fifo_denoise_clips(step_seeds=)``; include/avdiff_hip.h, "clip batch keying").  A single clip that is not in
    a list runs exactly as before.
    """
    # the latent guide's argument checks that need no device (the window count and the mask's shape follow the prompt split below)
    strength = P.check_init_args(prompt_modality, init_video, init_audio, strength, mask)
    st = cfg.get("streaming", {})
    if sampler is None:
        sampler = st.get("sampler", "windows")
    if sampler not in SAMPLERS:
        raise ValueError(f"sampler must be one of {SAMPLERS}, got {sampler!r}")
    if sampler == "fifo":
        fifo = _fifo_options(cfg, shard=shard, consensus=consensus, noise_keying=noise_keying, resample=resample, init_noise=init_noise,
                             fifo=fifo)
    has_init = init_video is not None or init_audio is not None
    clip_list = prompt_video if prompt_modality == "video" else prompt_audio
    if sampler == "fifo" and isinstance(clip_list, (list, tuple)):      # K clips as K queues in one engine
        _fifo_clips_refusals(cfg, fifo, len(clip_list), has_init, mask is not None, noise_seed)
        pc = P.read_config(cfg, prompt_modality, guidance_interval=guidance_interval, resample=resample, has_init=False, has_mask=False,
                           noise_seed=noise_seed)
        mods = dict(vid_vae=vid_vae, aud_codec=aud_codec, adapt_v=adapt_v, adapt_a=adapt_a, core=core, head=head, tstep_dim=tstep_dim)
        return _stream_generate_fifo_clips(cfg, pc, mods, device, prompt_modality, list(clip_list), fifo, seed=seed, noise_seed=noise_seed,
                                           return_latents=return_latents, max_windows_per_batch=max_windows_per_batch)
    if has_init and shard:
        raise ValueError("an init clip with shard=True is not implemented: the known windows would need a second broadcast to the "
                         "ranks; run the windows in one process")
    init = P.init_clip_array(init_video, init_audio)
    pc = P.read_config(cfg, prompt_modality, guidance_interval=guidance_interval, resample=resample, has_init=has_init,
                       has_mask=mask is not None, noise_seed=noise_seed)
    target, eta, sched = pc.target, pc.eta, pc.sched
    if consensus is None:
        consensus = st.get("latent_consensus")
    if noise_keying is None:
        noise_keying = st.get("noise_keying", "sample")
    if noise_keying not in DenoiseEngine.NOISE_KEYINGS:
        raise ValueError(f"noise_keying must be one of {DenoiseEngine.NOISE_KEYINGS}, got {noise_keying!r}")
    canvas_keyed = noise_keying == "canvas"
    if canvas_keyed and (consensus is None or consensus is False):
        raise ValueError("noise_keying='canvas' keys the DDIM noise by the position on the windows' shared latent canvas: it needs "
                         "consensus (or streaming.latent_consensus)")
    if canvas_keyed and noise_seed is None:
        raise ValueError("noise_keying='canvas' is a keying of the seeded noise stream: it needs noise_seed")
    if consensus is not None and consensus is not False:
        if shard:
            raise ValueError("consensus with shard=True is not implemented: windows on different ranks would have to exchange their "
                             "overlapping latent positions (a halo) after every step; run the windows on one device")
        if eta > 0 and not canvas_keyed:
            raise ValueError("consensus needs sampling.ddim_eta == 0 with the per-window noise stream: the mean of the windows' "
                             "independent noise draws would shrink their variance (noise_keying='canvas' with noise_seed keys the "
                             "noise by canvas position instead)")
        cons_hop, cons_L = latent_hop(cfg, target)
        cons_w = None if isinstance(consensus, str) and consensus == "uniform" else consensus
        if isinstance(cons_w, str):
            raise ValueError(f"consensus must be None, 'uniform' or a table of {cons_L} weights, got {consensus!r}")
        cons_w = Fn.consensus_weights(cons_w, cons_L)
        consensus = True
    else:
        consensus = False

    import torch.distributed as tdist
    world = tdist.get_world_size() if (shard and tdist.is_initialized()) else 1
    rank = tdist.get_rank() if world > 1 else 0
    root = rank == 0

    # the prompt windows and the shape of their encoded form (known on every rank without encoding: only rank 0 runs the encoder)
    chunks, zp_shape, lat = _prompt_windows(cfg, pc, prompt_modality, prompt_video, prompt_audio)
    n_prompt = P.prompt_tokens(pc, zp_shape)
    # the init clip's windows and the mask on the latent canvas, checked before anything is encoded
    init_chunks = _init_windows(cfg, pc, init, zp_shape[0])
    if sampler == "fifo":
        mods = dict(vid_vae=vid_vae, aud_codec=aud_codec, adapt_v=adapt_v, adapt_a=adapt_a, core=core, head=head, tstep_dim=tstep_dim)
        return _stream_generate_fifo(cfg, pc, mods, device, prompt_modality, chunks, zp_shape, lat, init_chunks, mask, strength, fifo,
                                     seed=seed, noise_seed=noise_seed, guide_seed=guide_seed, return_latents=return_latents,
                                     max_windows_per_batch=max_windows_per_batch)
    mask_w = None
    if mask is not None:
        g_hop, g_L = (cons_hop, cons_L) if consensus else latent_hop(cfg, target)
        mask_w = windows_from_canvas(_canvas_mask(mask, lat, zp_shape[0], g_hop, g_L), g_L, g_hop)      # [N_windows, *latent]
    z_p, root_error = None, None
    if root:
        try:
            z_p = _encode_windows(prompt_modality, vid_vae, aud_codec, chunks, device)
            if tuple(z_p.shape) != zp_shape:
                if world > 1:       # the other ranks sized their buffers from the config
                    raise L.AvdError(f"encoded prompt windows have shape {tuple(z_p.shape)}, the config implies {zp_shape}")
                # single process (e.g. a caller-supplied encoder): the encoder's own output decides, as in the reference
                zp_shape = tuple(z_p.shape)
                n_prompt = P.prompt_tokens(pc, zp_shape)
        except Exception as exc:            # noqa: BLE001 — re-raised below; a sharded run first tells the other ranks
            if world == 1:
                raise
            root_error = exc

    Nw = zp_shape[0]
    if return_latents and world > 1:
        raise ValueError("return_latents needs a single process: a sharded run gathers the decoded windows only")
    if consensus:
        if lat[1] != cons_L:
            raise ValueError(f"consensus: the target latent has {lat[1]} positions along its sliding axis (data.clip_seconds), a window of "
                             f"streaming.window_seconds has {cons_L}: they must be equal")
        canvas_shape = (lat[0], (Nw - 1) * cons_hop + cons_L) + tuple(lat[2:])
    if consensus and init_noise is not None:
        z0 = init_noise
        if tuple(z0.shape) == (Nw, *lat) and not torch.equal(windows_from_canvas(canvas_from_windows(z0, cons_hop), cons_L, cons_hop), z0):
            raise ValueError(f"consensus: init_noise differs between windows where they overlap (hop {cons_hop} of {cons_L} latent "
                             "positions); build it with windows_from_canvas(canvas, L, hop)")
    elif consensus and seed is not None:
        z0 = windows_from_canvas(torch.randn(*canvas_shape, generator=torch.Generator().manual_seed(int(seed))), cons_L, cons_hop)
    elif consensus:
        z0 = windows_from_canvas(torch.randn(*canvas_shape, device=device), cons_L, cons_hop)
    elif init_noise is not None:
        z0 = init_noise
    elif seed is not None:
        z0 = torch.randn(Nw, *lat, generator=torch.Generator().manual_seed(int(seed)))
    elif world > 1:
        raise ValueError("a sharded run needs init_noise or seed: every rank must start its windows from the same global draw")
    else:
        z0 = torch.randn(Nw, *lat, device=device)
    if tuple(z0.shape) != (Nw, *lat):
        raise ValueError(f"init_noise has shape {tuple(z0.shape)}, expected {(Nw, *lat)}")

    # the known windows of an init clip: encoded as one batch; under consensus made one canvas first (each window was encoded alone)
    known = None
    if init_chunks is not None:
        known = _encode_init(target, vid_vae, aud_codec, init_chunks, device, (Nw, *lat))
        if consensus:
            Fn.window_consensus(known, cons_hop, cons_w)

    def start(eng: DenoiseEngine, lo: int, hi: int):
        """(z_start, schedule) of the engine of windows [lo, hi): the initial latents and the whole schedule, or with an init clip the
        guided start (DenoiseEngine.set_known / start_latent; the guide stays set only under a mask)"""
        z = z0[lo:hi].to(device)
        if known is None:
            return z.contiguous(), sched           # in its own dtype: run refuses an init_noise that is not float32
        keying = dict(keying="canvas", hop=cons_hop) if consensus else {}
        return P.guided_start(eng, pc, known[lo:hi], None if mask_w is None else mask_w[lo:hi], z.float().contiguous(), strength,
                              P.default_guide_seed(guide_seed, noise_seed), sample_offset=lo, **keying)

    def engine(zp_part: torch.Tensor, lo0: int, lo: int, hi: int) -> DenoiseEngine:
        """the engine of windows [lo, hi), its prompt rows set from zp_part (which starts at window lo0)"""
        eng = P.build_engine(pc, adapt_v=adapt_v, adapt_a=adapt_a, core=core, head=head, tstep_dim=tstep_dim, latent_shape=(hi - lo, *lat),
                             n_prompt=n_prompt, noise_seed=noise_seed, sample_offset=lo if noise_seed is not None else 0,
                             noise_keying=noise_keying, canvas_hop=cons_hop if canvas_keyed else None)
        eng.set_prompt(zp_part[lo - lo0:hi - lo0].to(device).float().contiguous())
        return eng

    def denoise(zp_part: torch.Tensor, lo0: int, hi0: int) -> torch.Tensor:
        """the windows [lo0, hi0) of the list, stepped in batches of at most max_windows_per_batch; no communication"""
        outs = []
        for lo in range(lo0, hi0, max_windows_per_batch):
            hi = min(hi0, lo + max_windows_per_batch)
            eng = engine(zp_part, lo0, lo, hi)
            outs.append(eng.run(*start(eng, lo, hi)))
        if not outs:
            return torch.empty(0, *lat, device=device)
        return torch.cat(outs, 0) if len(outs) > 1 else outs[0]

    def denoise_consensus(zp_all: torch.Tensor) -> torch.Tensor:
        """all windows as views of one latent canvas: one engine with the consensus inside its step, or, above
        max_windows_per_batch, several engines in lock-step with one consensus pass over all windows after every step"""
        if Nw <= max_windows_per_batch:
            eng = engine(zp_all, 0, 0, Nw)
            eng.set_window_consensus(cons_hop, cons_w)
            return eng.run(*start(eng, 0, Nw))
        engs = [(lo, min(Nw, lo + max_windows_per_batch)) for lo in range(0, Nw, max_windows_per_batch)]
        engs = [(lo, hi, engine(zp_all, 0, lo, hi)) for lo, hi in engs]
        starts = [start(eng, lo, hi) for lo, hi, eng in engs]
        sched_k = starts[0][1]                     # one strength: every engine runs the same tail of the schedule
        za = torch.cat([z for z, _ in starts], 0).float()
        for _, _, eng in engs:
            eng.check_schedule(sched_k)
            eng.begin(sched_k)
        w_dev = cons_w.to(device)
        zb = torch.empty_like(za)
        if sched_k.numel() < 2:
            return za                              # strength 0: no steps, the known windows
        for first, stop, kind in su.trajectory_segments(sched_k, pc.interval):      # the kind of every pair, read on the host as run() does
            for i in range(first, stop):
                if kind == "renoise":              # canvas-keyed: the same linear map with the same normals on agreeing windows
                    for lo, hi, eng in engs:
                        eng.advance_renoise(za[lo:hi], i)
                    continue
                for lo, hi, eng in engs:
                    eng.advance(za[lo:hi], zb[lo:hi], cond_only=kind == "cond")
                Fn.window_consensus(zb, cons_hop, w_dev)
                za, zb = zb, za
        return za

    def decode_windows(z: torch.Tensor) -> torch.Tensor:
        return _decode_windows(cfg, pc, vid_vae, aud_codec, lat, z, device)

    if world > 1:
        if comm_device is None:
            comm_device = device if tdist.get_backend() == "nccl" else torch.device("cpu")
        out = D.run_sharded(Nw, z_p if root else None, zp_shape, comm_device, lambda part, lo, hi: decode_windows(denoise(part, lo, hi)),
                            result="root", error=root_error)
        if not root:
            return None
        out = out.to(device)
    else:
        z_fin = denoise_consensus(z_p) if consensus else denoise(z_p, 0, Nw)
        out = decode_windows(z_fin)

    res = _stitch(cfg, pc, out)
    if return_latents:
        res["latents"] = z_fin.cpu().numpy()
    return res
