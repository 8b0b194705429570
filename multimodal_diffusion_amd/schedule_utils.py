"""Diffusion schedule utilities — host-side mirror of ``avdiff/utils/schedule_utils.py`` over the HIP C ABI.

Schedule tables are a once-per-run host computation: they are built on the CPU with the same
fp32 operation sequence as the reference so the tables are bit-identical, then uploaded.  The per-step ops
(``timestep_embedding``, ``ddim_step``) run as HIP kernels.  ``q_sample`` is training-only and not provided.
"""
from __future__ import annotations

import math
import numbers
from typing import List, Optional, Tuple

import torch

from . import functional as Fn

_KINDS = ("linear", "sigmoid", "cosine")


def make_beta_schedule(steps: int, kind: str = "cosine", min_beta: float = 1e-4, max_beta: float = 2e-2) -> torch.Tensor:
    """betas[t], t = 0..steps-1 (schedule_utils.py:14-49).  fp32 CPU tensor."""
    kind = kind.lower()
    if kind not in _KINDS:
        raise ValueError(f"Unknown schedule kind: {kind}")
    f32 = torch.float32
    if kind == "cosine":
        u = torch.linspace(0, steps, steps + 1, dtype=f32) / steps
        curve = torch.cos((u + 0.008) / (1 + 0.008) * math.pi / 2) ** 2
        curve = curve / curve[0]
        betas = 1 - curve[1:] / curve[:-1]
    elif kind == "linear":
        betas = torch.linspace(min_beta, max_beta, steps, dtype=f32)
    else:
        betas = min_beta + (max_beta - min_beta) * torch.sigmoid(torch.linspace(-6, 6, steps, dtype=f32))
    return betas.clamp(1e-8, 0.999)


def alphas_cumprod_from_betas(betas: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(alphas, alpha_bar) — schedule_utils.py:52-57."""
    alphas = 1.0 - betas.to(torch.float32)
    return alphas, alphas.cumprod(0)


def make_sampling_schedule(T_train: int, T_sample: int) -> torch.Tensor:
    """T_sample+1 decreasing int64 timesteps from T_train-1 to -1 (schedule_utils.py:132-143)."""
    return torch.linspace(T_train - 1, -1, T_sample + 1).round().to(torch.long)


def truncate_schedule(sched, strength: float) -> torch.Tensor:
    """The tail of a sampling schedule that SDEdit / a partial denoise runs: with n = len(sched) - 1 steps, keep
    k = min(n, floor(strength * n + 1e-9)) steps, i.e. the last k + 1 entries (k = 0: the one entry -1 of a finished trajectory,
    no steps).  ``strength`` must lie in [0, 1]; 1 returns the whole schedule.  Host-side (int64 CPU tensor)."""
    strength = float(strength)
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f"strength must lie in [0, 1], got {strength}")
    sc = torch.as_tensor(sched).reshape(-1).to("cpu", torch.long)
    if sc.numel() < 1:
        raise ValueError("the schedule is empty")
    n = sc.numel() - 1
    k = min(n, math.floor(strength * n + 1e-9))
    return sc[n - k:].clone()


def check_guidance_interval(interval) -> Optional[Tuple[int, int]]:
    """Validate a guidance interval: None (guidance on every step), or (t_lo, t_hi) — two integers in training timesteps with
    0 <= t_lo <= t_hi, both ends inclusive.  Returns None or the pair as Python ints.  Host-side."""
    if interval is None:
        return None
    if isinstance(interval, (str, bytes)) or not hasattr(interval, "__len__") or len(interval) != 2:
        raise ValueError(f"guidance_interval must be None or a pair (t_lo, t_hi), got {interval!r}")
    out = []
    for v in interval:
        if isinstance(v, torch.Tensor) and v.numel() == 1:
            v = v.item()
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise ValueError(f"guidance_interval holds training timesteps (integers), got {v!r}")
        out.append(int(v))
    lo, hi = out
    if lo < 0 or lo > hi:
        raise ValueError(f"guidance_interval needs 0 <= t_lo <= t_hi, got ({lo}, {hi})")
    return lo, hi


def level_table(spec, T_train: int, name: str, lo: Optional[float] = None, hi: Optional[float] = None) -> torch.Tensor:
    """A value per noise level as a CPU float32 [T_train] tensor (include/avdiff_hip.h, "slot CFG control": the kernels look a slot's
    guidance and rescale up at its t_now).  ``spec``: a number (every level), a sequence / array / tensor of T_train values, or a
    callable t -> value, evaluated here for t = 0 .. T_train - 1.  Refuses NaN, infinities and, where given, values outside
    [lo, hi]: the kernels trust the device values.  Host-side."""
    T_train = _whole(T_train, "T_train")
    if callable(spec):
        vals = [spec(t) for t in range(T_train)]
        for t, v in enumerate(vals):
            if isinstance(v, torch.Tensor) and v.numel() == 1:
                vals[t] = v = v.item()
            if isinstance(v, bool) or not isinstance(v, numbers.Real):
                raise ValueError(f"{name}: the callable must return a number per level, got {v!r} at t = {t}")
        t_ = torch.tensor(vals, dtype=torch.float32)
    elif isinstance(spec, (bool, str, bytes)) or spec is None:
        raise ValueError(f"{name} must be a number, {T_train} values or a callable t -> value, got {spec!r}")
    else:
        try:
            t_ = torch.as_tensor(spec.detach().cpu() if isinstance(spec, torch.Tensor) else spec, dtype=torch.float32)
        except (TypeError, ValueError, RuntimeError):
            raise ValueError(f"{name} must be a number, {T_train} values or a callable t -> value, got {spec!r}") from None
        if t_.dim() == 0:
            t_ = t_.reshape(1).expand(T_train)
        elif t_.dim() != 1 or t_.numel() != T_train:
            raise ValueError(f"{name} has shape {tuple(t_.shape)}, expected a number or {T_train} values (one per training timestep)")
    if not bool(torch.isfinite(t_).all()):
        raise ValueError(f"{name} must be finite at every level")
    if lo is not None and not bool(((t_ >= lo) & (t_ <= hi)).all()):
        raise ValueError(f"{name} must lie in [{lo:g}, {hi:g}] at every level, got [{float(t_.min()):g}, {float(t_.max()):g}]")
    return t_.contiguous().clone()


def guidance_interval_table(g: float, interval, T_train: int) -> torch.Tensor:
    """The slot form of a guidance interval as a ``level_table``: ``g`` at the levels t_lo <= t <= t_hi (``check_guidance_interval``;
    None: every level), 1.0 outside, where the CFG combine returns the conditional prediction.  A queue has no cond-only steps (some
    slot is always inside the interval), so the interval acts through the table.  Host-side."""
    if isinstance(g, bool) or not isinstance(g, numbers.Real) or not math.isfinite(g):
        raise ValueError(f"guidance must be a finite number, got {g!r}")
    iv = check_guidance_interval(interval)
    T_train = _whole(T_train, "T_train")
    tab = torch.ones(T_train, dtype=torch.float32)
    if iv is None:
        tab.fill_(float(g))
    else:
        tab[iv[0]:iv[1] + 1] = float(g)
    return tab


def guidance_segments(sched, interval) -> List[Tuple[int, int, bool]]:
    """Split the steps of a sampling schedule by kind: step i goes from sched[i] to sched[i + 1] and is a CFG step when
    t_lo <= sched[i] <= t_hi (``interval`` None: always), else a cond-only step.  Returns the maximal runs of equal kind as
    [(start, stop, cfg)] with steps start .. stop - 1, in order; together they partition range(len(sched) - 1).  Host-side."""
    iv = check_guidance_interval(interval)
    sc = torch.as_tensor(sched).reshape(-1).to("cpu", torch.long).tolist()
    segs: List[Tuple[int, int, bool]] = []
    for i, t in enumerate(sc[:-1]):
        cfg = iv is None or iv[0] <= t <= iv[1]
        if segs and segs[-1][2] == cfg:
            segs[-1] = (segs[-1][0], i + 1, cfg)
        else:
            segs.append((i, i + 1, cfg))
    return segs


def _whole(v, name: str) -> int:
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
        raise ValueError(f"{name} must be an integer >= 1, got {v!r}")
    return int(v)


def check_resample(resample) -> Optional[Tuple[int, int]]:
    """Validate a RePaint resampling setting: None (off), a pair (jump, resamples) or a dict {"jump":, "resamples":} (the config's
    ``sampling.resample``), both integers >= 1.  Returns None or the pair as Python ints.  Host-side."""
    if resample is None:
        return None
    if isinstance(resample, dict):
        if set(resample) != {"jump", "resamples"}:
            raise ValueError(f"resample as a dict holds exactly 'jump' and 'resamples', got {sorted(resample)}")
        resample = (resample["jump"], resample["resamples"])
    if isinstance(resample, (str, bytes)) or not hasattr(resample, "__len__") or len(resample) != 2:
        raise ValueError(f"resample must be None, a pair (jump, resamples) or a dict with those keys, got {resample!r}")
    return _whole(resample[0], "resample jump"), _whole(resample[1], "resamples")


def resample_schedule(sched, jump: int, resamples: int) -> torch.Tensor:
    """The RePaint time-travel schedule (Lugmayr et al. 2022; diffusers' ``RePaintScheduler``) of a decreasing sampling schedule
    s[0..n] that ends in -1.  The n steps are cut into blocks of ``jump`` steps, block k from a_k = k*jump to b_k = min(a_k + jump, n).
    A block with s[b_k] >= 0 is emitted ``resamples`` times, its passes joined by the up-jump s[b_k] -> s[a_k] (a renoise pair, see
    ``step_segments``); the block that ends in -1 is emitted once — a finished latent is never sent back.  n = 4, jump = 2,
    resamples = 2 gives [s0, s1, s2, s0, s1, s2, s3, s4].  ``resamples`` == 1 returns the schedule unchanged.  Host-side (int64 CPU
    tensor)."""
    jump, resamples = _whole(jump, "jump"), _whole(resamples, "resamples")
    sc = torch.as_tensor(sched).reshape(-1).to("cpu", torch.long)
    s = sc.tolist()
    if not s or s[-1] != -1:
        raise ValueError("resample_schedule needs a sampling schedule that ends in -1")
    if any(b >= a for a, b in zip(s[:-1], s[1:])):
        raise ValueError("resample_schedule needs a strictly decreasing schedule (resample once, from make_sampling_schedule / "
                         "truncate_schedule)")
    n = len(s) - 1
    if resamples == 1 or n == 0:
        return sc.clone()
    out = [s[0]]
    for a in range(0, n, jump):
        b = min(a + jump, n)
        for r in range(resamples if s[b] >= 0 else 1):
            if r:
                out.append(s[a])                 # the up-jump s[b] -> s[a]
            out.extend(s[a + 1:b + 1])
    return torch.tensor(out, dtype=torch.long)


def step_segments(sched, interval) -> List[Tuple[int, int, str]]:
    """``guidance_segments`` for a schedule that may hold up-jumps: pair i = (sched[i], sched[i + 1]) is a "renoise" when sched[i + 1] >
    sched[i] (the forward jump of a resampling schedule), else a denoising step — "cfg" when t_lo <= sched[i] <= t_hi (``interval``
    None: always), else "cond".  Equal neighbours are a ValueError.  Returns the maximal runs of equal kind as [(start, stop, kind)]
    with pairs start .. stop - 1, in order; together they partition range(len(sched) - 1).  Host-side."""
    iv = check_guidance_interval(interval)
    sc = torch.as_tensor(sched).reshape(-1).to("cpu", torch.long).tolist()
    segs: List[Tuple[int, int, str]] = []
    for i, (t, nxt) in enumerate(zip(sc[:-1], sc[1:])):
        if nxt == t:
            raise ValueError(f"schedule entries {i} and {i + 1} are both {t}: a pair is a denoising step (down) or a renoise (up)")
        kind = "renoise" if nxt > t else ("cfg" if iv is None or iv[0] <= t <= iv[1] else "cond")
        if segs and segs[-1][2] == kind:
            segs[-1] = (segs[-1][0], i + 1, kind)
        else:
            segs.append((i, i + 1, kind))
    return segs


def has_jumps(sched) -> bool:
    """Whether a schedule is a resampling schedule: it holds a time-travel jump, an up-pair that returns to a timestep the schedule
    has already passed (the only jumps ``resample_schedule`` emits).  ``DenoiseEngine.run`` and ``stream_generate`` read every
    up-pair of such a schedule as a renoise (``step_segments``).  An up-pair to a timestep not seen before is no time travel: the DDIM
    engine has always taken any schedule and steps through such a pair as before, the multistep solver refuses it as before."""
    seen = set()
    sc = torch.as_tensor(sched).reshape(-1).to("cpu", torch.long).tolist()
    for a, b in zip(sc[:-1], sc[1:]):
        seen.add(a)
        if b > a and b in seen:
            return True
    return False


def trajectory_segments(sched, interval) -> List[Tuple[int, int, str]]:
    """The pairs of any schedule by kind, [(start, stop, kind)] with kind in {"cfg", "cond", "renoise"}: what ``DenoiseEngine.run`` and
    ``stream_generate``'s lock-step loop iterate.  A resampling schedule (``has_jumps``) is split by ``step_segments``; any other by
    ``guidance_segments``, every pair a denoising step — an up-pair to a timestep not seen before and equal neighbours included."""
    if has_jumps(sched):
        return step_segments(sched, interval)
    return [(a, b, "cfg" if cfg else "cond") for a, b, cfg in guidance_segments(sched, interval)]


def fifo_plan(sched, S: int):
    """The timestep tables of FIFO diagonal denoising (Kim et al. 2024, with its latent partitioning) for ``DenoiseEngine.step_slots``.
    ``sched`` = s_0 > s_1 > ... > s_n = -1, strictly decreasing, n steps; ``S`` slots per sample, n % S == 0.  The queue has n slots,
    queue slot q in sample q // S at slot q % S of a batch of B = n // S samples; its head (q = 0) is the cleanest.

    steady state: slot q takes step n-1-q (t_now = s_{n-1-q}, t_prev = s_{n-q}) in every iteration: one model call moves every slot
      one level, the head leaves finished (t_prev = -1), the queue shifts and noise at s_0 enters at the tail;
    ramp: all n slots start as noise at s_0.  Ramp iteration r = 0 .. n-2 (no shift): slot q <= r takes step r-q, slot q > r holds at
      s_0 (t_prev == t_now).  After the ramp slot q stands at s_{n-1-q}: the steady state.

    Returns (ramp_now, ramp_prev, steady_now, steady_prev): int64 CPU tensors [n-1, B, S] x 2 and [B, S] x 2.  Clip slot c leaves in
    steady iteration c, having taken the pairs (s_i, s_{i+1}), i = 0 .. n-1, in order, and nothing else but holds at s_0.  Host-side."""
    S = _whole(S, "S")
    s = torch.as_tensor(sched).reshape(-1).to("cpu", torch.long).tolist()
    if len(s) < 2 or s[-1] != -1:
        raise ValueError("fifo_plan needs a sampling schedule of at least one step that ends in -1")
    if any(b >= a for a, b in zip(s[:-1], s[1:])):
        raise ValueError("fifo_plan needs a strictly decreasing schedule: every queue slot takes its steps in order (no jumps, no "
                         "equal neighbours)")
    n = len(s) - 1
    if n % S:
        raise ValueError(f"fifo_plan: the {n} steps of the schedule must be a multiple of the S = {S} slots of a sample (the queue is "
                         "n slots in n / S samples)")
    B = n // S
    q = torch.arange(n)
    sc = torch.tensor(s, dtype=torch.long)
    steady_now, steady_prev = sc[n - 1 - q], sc[n - q]
    r = torch.arange(n - 1)[:, None]
    live = q[None, :] <= r                                    # slot q steps in ramp iteration r
    i = (r - q[None, :]).clamp(min=0)
    hold = torch.full((n - 1, n), s[0], dtype=torch.long)
    ramp_now, ramp_prev = torch.where(live, sc[i], hold), torch.where(live, sc[i + 1], hold)
    return ramp_now.view(n - 1, B, S), ramp_prev.view(n - 1, B, S), steady_now.view(B, S).clone(), steady_prev.view(B, S).clone()


def fifo_plan_last(sched, S: int):
    """The third table of ``fifo_plan`` for a multistep solver (``DenoiseEngine.step_slots(t_last=)`` on solver "dpmpp_2m"): where a
    slot takes step i its t_last is s_{i-1}, the timestep its previous step started from and its history's; a slot taking step 0 has
    -1 (first order), and so has a held slot (it is not read there).  Returns (ramp_last [n-1, B, S], steady_last [B, S]), int64 CPU
    tensors in ``fifo_plan``'s layout, which also refuses what this refuses.  In the steady state the tail slot (step 0) is first
    order, so the history of a slot entering the queue is never read."""
    ramp_now, ramp_prev, steady_now, _ = fifo_plan(sched, S)
    n = ramp_now.shape[0] + 1
    s = torch.as_tensor(sched).reshape(-1).to("cpu", torch.long)
    last = torch.cat([torch.tensor([-1]), s[:n - 1]])                  # last[i] = s_{i-1}
    q = torch.arange(n)
    steady_last = last[n - 1 - q].view_as(steady_now).clone()
    r = torch.arange(n - 1)[:, None]
    live = q[None, :] <= r
    i = (r - q[None, :]).clamp(min=0)
    ramp_last = torch.where(live, last[i], torch.full((n - 1, n), -1, dtype=torch.long))
    return ramp_last.view_as(ramp_now).clone(), steady_last


def _lookahead_tables(sched, S: int, ctx: int, context: str):
    """(ramp, steady) of the lookahead plan per LOGICAL slot, each a (t_now, t_prev, t_last) triple of int64 tensors [n-1, Q] /
    [ctx+1, Q] with Q = ctx + n, and the window index map [B, S] of the logical slot every window position holds"""
    S = _whole(S, "S")
    if isinstance(ctx, bool) or not isinstance(ctx, int) or not 0 <= ctx < S:
        raise ValueError(f"fifo_lookahead_plan: the lookahead ctx must be an int in [0, S = {S}), got {ctx!r}")
    if context not in ("noise", "clean"):
        raise ValueError(f"fifo_lookahead_plan: context must be 'noise' or 'clean', got {context!r}")
    h = S - ctx
    fifo_plan(sched, 1)                                       # the schedule's own refusals
    s = torch.as_tensor(sched).reshape(-1).to("cpu", torch.long)
    n = s.numel() - 1
    if n % h:
        raise ValueError(f"fifo_lookahead_plan: the {n} steps of the schedule must be a multiple of the h = S - ctx = {h} slots a "
                         "window updates (the queue is n active slots in n / h windows)")
    B = n // h
    s0 = int(s[0])
    last = torch.cat([torch.tensor([-1]), s[:n - 1]])         # last[i] = s_{i-1}
    a = torch.arange(n)
    # ramp, active slots: fifo_plan's rows at one slot per sample, with fifo_plan_last's third table
    r = torch.arange(n - 1)[:, None]
    live = a[None, :] <= r
    i = (r - a[None, :]).clamp(min=0)
    hold = torch.full((n - 1, n), s0, dtype=torch.long)
    act = (torch.where(live, s[i], hold), torch.where(live, s[i + 1], hold), torch.where(live, last[i], torch.full_like(hold, -1)))
    c0 = torch.full((n - 1, ctx), 0 if context == "clean" else s0, dtype=torch.long)
    ramp = (torch.cat([c0, act[0]], 1), torch.cat([c0, act[1]], 1), torch.cat([torch.full_like(c0, -1), act[2]], 1))
    # steady, row min(m, ctx): context slot q is a finished slot once q >= ctx - m ("clean": always)
    m = torch.arange(ctx + 1)[:, None]
    done = (torch.arange(ctx)[None, :] >= ctx - m) | (context == "clean")
    cm = torch.where(done, torch.zeros((), dtype=torch.long), torch.full((), s0, dtype=torch.long)).expand(ctx + 1, ctx)
    rows = lambda t: t[None, :].expand(ctx + 1, n)
    steady = (torch.cat([cm, rows(s[n - 1 - a])], 1), torch.cat([cm, rows(s[n - a])], 1),
              torch.cat([torch.full_like(cm, -1), rows(last[n - 1 - a])], 1))
    q = torch.arange(B)[:, None] * h + torch.arange(S)[None, :]      # window k position s holds logical slot k*h + s
    return ramp, steady, q, ctx


def _lookahead_windows(tabs, q, ctx: int, which: int) -> torch.Tensor:
    """per-logical-slot triples -> the [rows, B, S] table `which` (0 t_now, 1 t_prev, 2 t_last): a stepping position (s >= ctx) takes
    its slot's entry, a held one (s < ctx) t_now for t_now and t_prev — the duplicate-label invariant — and -1 for t_last"""
    held = (torch.arange(q.shape[1]) < ctx)[None, None, :]
    now, own = tabs[0][:, q], tabs[which][:, q]
    if which == 2:
        return torch.where(held, torch.full_like(own, -1), own).contiguous()
    return torch.where(held, now, own).contiguous()


def fifo_lookahead_plan(sched, S: int, ctx: int, context: str = "noise"):
    """The timestep tables of FIFO lookahead denoising (Kim et al. 2024; layout in include/avdiff_hip.h, "FIFO lookahead") for
    ``DenoiseEngine.step_slots``.  ``sched`` = s_0 > ... > s_n = -1 as for ``fifo_plan``; ``S`` slots per sample, of which the first
    ``ctx`` (0 <= ctx < S) are held context and the last h = S - ctx step; n % h == 0 and the batch is B = n // h windows.  Window k
    holds logical slots k*h .. k*h + S - 1 of a queue of ctx context slots and n active ones (active slot a = logical slot ctx + a).

    The invariant of every row: a duplicate (a window's position s < ctx) is held at the timestep its slot's owner takes as t_now in
    the same call, so every copy of a slot embeds the same timestep.
    ramp, row r = 0 .. n-2: active slot a <= r takes step r-a, a > r holds at s_0; the context holds at s_0 (``context="noise"``: the
      initial context is seeded noise, labelled as noise like any slot waiting in the ramp) or at 0 (``"clean"``: supplied latents);
    steady, row min(m, ctx) for iteration m: active slot a takes (s_{n-1-a}, s_{n-a}); context slot q holds at 0 once it is a
      finished slot — "noise": q >= ctx - m, "clean": always — else at s_0.

    Returns (ramp_now, ramp_prev, steady_now, steady_prev): int64 CPU tensors [n-1, B, S] x 2 and [ctx+1, B, S] x 2.  ``ctx = 0`` gives
    ``fifo_plan``'s tables (the steady ones as one row).  Refuses what ``fifo_plan`` refuses.  Host-side."""
    ramp, steady, q, ctx = _lookahead_tables(sched, S, ctx, context)
    return (_lookahead_windows(ramp, q, ctx, 0), _lookahead_windows(ramp, q, ctx, 1), _lookahead_windows(steady, q, ctx, 0),
            _lookahead_windows(steady, q, ctx, 1))


def fifo_lookahead_plan_last(sched, S: int, ctx: int, context: str = "noise"):
    """The third table of ``fifo_lookahead_plan`` for solver "dpmpp_2m": ``fifo_plan_last``'s values on the stepping positions (s_{i-1}
    where the slot takes step i, -1 at step 0 and while it waits in the ramp) and -1 on every held position.  Returns (ramp_last
    [n-1, B, S], steady_last [ctx+1, B, S]), int64 CPU tensors."""
    ramp, steady, q, ctx = _lookahead_tables(sched, S, ctx, context)
    return _lookahead_windows(ramp, q, ctx, 2), _lookahead_windows(steady, q, ctx, 2)


def fifo_slot_keying(S: int, ctx: int = 0) -> Tuple[int, int]:
    """(first_offset, stride) = (-ctx, S - ctx): how a FIFO queue keys the step noise of an eta > 0 engine by clip position
    (include/avdiff_hip.h, "clip-keyed slot noise").  Before the step of steady iteration m (the ramp: m = 0) position s of sample k
    holds clip slot m + first_offset + k*stride + s, so the drivers pass ``step_slots(clip_first=m + first_offset,
    clip_stride=stride)``: a queue of samples (``ctx`` = 0) is S slots apart, lookahead windows h = S - ctx, their first ctx positions
    being the slots before the window's own.  Clip slot c then draws at the keys (c, s_i), i = 0 .. n-1, once each, in either queue."""
    S = _whole(S, "S")
    if isinstance(ctx, bool) or not isinstance(ctx, int) or not 0 <= ctx < S:
        raise ValueError(f"fifo_slot_keying: the lookahead ctx must be an int in [0, S = {S}), got {ctx!r}")
    return -ctx, S - ctx


def resample_from_config(scfg) -> Optional[Tuple[int, int]]:
    """``sampling.resample`` of a config: {jump:, resamples:}; a missing key or None means no resampling."""
    return check_resample(scfg.get("resample"))


def guidance_interval_from_config(scfg, modality: str) -> Optional[Tuple[int, int]]:
    """``sampling.guidance_interval`` of a config: a per-modality dict of [t_lo, t_hi] (like ``guidance_scale``); a missing key or
    modality, or None, means guidance on every step."""
    table = scfg.get("guidance_interval") or {}
    if not isinstance(table, dict):
        raise ValueError(f"sampling.guidance_interval must be a per-modality dict of [t_lo, t_hi], got {table!r}")
    return check_guidance_interval(table.get(modality))


def timestep_embedding(timesteps: torch.Tensor, dim: int, max_period: int = 10000) -> torch.Tensor:
    """[cos | sin] sinusoidal embedding [B, dim] on the device (schedule_utils.py:64-86)."""
    return Fn.timestep_embedding(timesteps, dim, max_period)


def ddim_step(x_t: torch.Tensor, t_now: torch.Tensor, t_prev: torch.Tensor, eps_hat: torch.Tensor,
              alpha_bar: torch.Tensor, eta: float = 0.0, noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One DDIM update x_{t_prev} from x_t (schedule_utils.py:146-200); t_prev = -1 means alpha_bar = 1.

    ``alpha_bar`` may live on the CPU (as it does in the reference sampler, sample_clip.py:274-275): it is
    uploaded.  ``noise`` (extension) lets the caller supply z for eta > 0; otherwise it is drawn like the reference.
    """
    return Fn.ddim_step(x_t, t_now, t_prev, eps_hat, alpha_bar, eta, noise)
