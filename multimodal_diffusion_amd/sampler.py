"""DDIM + CFG sampler — host-side mirror of ``avdiff/models/infer/sample_clip.py`` over the HIP C ABI.

Keeps the reference names (``LinearAdapter``, ``add_sinusoidal_timestep``, ``build_components``,
``latents_to_tokens_*``, ``tokens_to_latents_audio``, ``sample_one_direction``) and adds what the reference
lacks: ``DenoiseEngine`` — a *batched* (B >= 1) on-device loop where one denoising step (sample_clip.py:359-389
or :318-348) is a single ``avd_denoise_step_f32`` call with the cond/null branches stacked to 2B, the constant
prompt rows embedded once, the timestep schedule resident on the device and the step optionally replayed
from a captured HIP graph.

File I/O and the CLI (sample_clip.py:112-174, 399-461) are out of scope; ``VideoVAE`` / ``AudioCodec`` are the
loop *boundary*  and are taken as caller-supplied modules.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib as L
from . import _pipeline as P
from . import functional as Fn
from . import ops
from . import schedule_utils as su
from ._pipeline import tube_from_config      # noqa: F401  (its home is the pipeline front end)
from .mmdt import MMDiT
from .noise_heads import MultiModalNoiseHead


class LinearAdapter(nn.Module):
    """Per-modality linear projection to token width (sample_clip.py:48-56); PyTorch-default Linear init."""

    def __init__(self, d_in: int, d_out: int):
        super().__init__()
        self.proj = nn.Linear(d_in, d_out)     # parameter container only

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return Fn.linear(x, self.proj.weight, self.proj.bias)


def add_sinusoidal_timestep(tokens: torch.Tensor, t_scalar: torch.Tensor, dim: int) -> torch.Tensor:
    """[B,N,d] + t[B] -> [B,N,d+dim] by concatenation (sample_clip.py:59-70).  Stand-alone helper; the engine fuses
    this into the sequence-assembly kernel instead."""
    emb = su.timestep_embedding(L.dev_i64(t_scalar, tokens.device), dim)
    out = torch.empty(tokens.shape[0], tokens.shape[1], tokens.shape[2] + dim, device=tokens.device, dtype=tokens.dtype)
    out[..., :tokens.shape[2]] = tokens
    out[..., tokens.shape[2]:] = emb[:, None, :]
    return out


def build_components(cfg: Dict, device: torch.device, vid_vae: Optional[nn.Module] = None,
                     aud_codec: Optional[nn.Module] = None):
    """(vid_vae, aud_codec, adapt_v, adapt_a, core, head, tstep_dim) as sample_clip.py:75-109.

    The codec / VAE are built from ``cfg["video"]`` / ``cfg["audio"]`` like the reference unless the caller passes
    its own modules (anything with ``encode`` / ``decode``); they sit outside the per-step path.
    Extension over the reference config: ``cfg["runtime"]["matmul"]`` in {"auto", "f32", "bf16x3", "bf16x3_strict", "f16x2", "bf16"}
    selects the matrix-pipe mode of the MMDiT core, the noise head and the VAE (default "auto": the exact three-plane bf16x3 kernels
    where they engage, fp32 MFMA elsewhere — what ``bench.py`` times; same fp32-level error either way).
    """
    matmul = str(cfg.get("runtime", {}).get("matmul", "auto"))
    if matmul not in L.MATMUL_TERMS:
        raise ValueError(f"runtime.matmul must be one of {sorted(L.MATMUL_TERMS)}, got {matmul!r}")
    if vid_vae is None and "video" in cfg:
        from .vae_video3d import VideoVAE
        vid_vae = VideoVAE.from_config(cfg["video"]).to(device).eval()
        vid_vae.matmul = matmul if matmul in ("auto", "f32", "bf16x3", "f16x2") else "bf16x3"     # bf16 / strict: the exact three-plane convolutions
    if aud_codec is None and "audio" in cfg:
        from .audio_codec import AudioCodec
        aud_codec = AudioCodec.from_config(cfg["audio"]).to(device).eval()
    d = int(cfg["tokenizer"]["width"])
    out_v = int(cfg["model"]["heads"]["video"]["out_dim"])
    out_a = int(cfg["model"]["heads"]["audio"]["out_dim"])
    tstep_dim = int(cfg["embeddings"].get("timestep_dim", 256))
    adapt_v = LinearAdapter(out_v, d - tstep_dim).to(device)
    adapt_a = LinearAdapter(out_a, d - tstep_dim).to(device)
    core = MMDiT(**cfg["model"]["core"]).to(device).eval()
    core.matmul = matmul
    head = MultiModalNoiseHead(
        input_dims={"video": d, "audio": d}, output_dims={"video": out_v, "audio": out_a},
        hidden_dim=int(cfg["model"]["heads"]["video"]["hidden_dim"]), num_shared_layers=2,
        num_modality_specific_layers=1, dropout=float(cfg["model"]["core"].get("dropout", 0.1)),
        activation=cfg["model"]["heads"]["video"].get("activation", "gelu")).to(device).eval()
    head.matmul = matmul
    return vid_vae, aud_codec, adapt_v, adapt_a, core, head, tstep_dim


def latents_to_tokens_video(z_v: torch.Tensor, t_p: int, p: int) -> torch.Tensor:
    return ops.tube_patch_video(z_v, t=t_p, h=p, w=p)


def latents_to_tokens_audio(z_a: torch.Tensor, l_chunk: int, s_chunk: int) -> torch.Tensor:
    return Fn.audio_tokens(z_a, l_chunk, s_chunk)


def tokens_to_latents_audio(tokens: torch.Tensor, Ca: int, l_chunk: int, Fa: int, stride: int) -> torch.Tensor:
    """Overlap-add back to [B,Ca,Fa] (crop / zero-pad), sample_clip.py:191-215 — one kernel, no Python loops."""
    return Fn.audio_untokens(tokens, Ca, l_chunk, Fa, stride)


# ----------------------------------------------------------------------------------------------------------
# batched on-device loop
# ----------------------------------------------------------------------------------------------------------

class FifoQueue:
    """The state of one open FIFO queue (``DenoiseEngine.fifo_open``): the device cursors ``r`` (ramp iteration) and ``m`` (steady
    iteration), the uploaded tables (``ramp``: [n - 1, B*S] each; ``steady`` and the selected ``slot`` tables: [B, S] each; two, or
    three with t_last), the prompt canvas ``canvas_p`` and the prompt-latent buffer ``prompt``, the latent buffers ``z`` / ``other``,
    the clip canvas ``clip``, and what the launches take by value: ``seed``, ``s0``, ``n`` (= c0), ``n_slots``, ``hop``, ``frac``
    ((prompt_den, prompt_interp) of a fractional prompt hop ``hop / prompt_den``, None on a whole one) and ``clip_first`` (0 on an eta > 0 engine with a noise_seed, whose steps key their noise by clip slot off ``m``; else None)."""


class _CapturedPair:
    """A captured two-step HIP graph of one engine.  ``replay()`` first re-checks the engine's weight tables: parameters updated in
    place behind unchanged pointers are picked up (derived images are refreshed in place).  The graph holds every device pointer
    and every by-value scale of the tables it was captured with, so it carries the engine's table GENERATION of that moment: a
    re-allocated parameter, workspace or prompt buffer, or a changed by-value scale, moves the engine to a new generation and every
    pair captured before stays refused for good — also after the engine has captured again."""

    def __init__(self, engine: "DenoiseEngine", graph: "torch.cuda.CUDAGraph"):
        self.engine, self.graph, self.generation = engine, graph, engine._generation

    def replay(self) -> None:
        self.engine._sync_weights()
        if self.generation != self.engine._generation:
            raise L.AvdError(f"this captured graph is stale ({self.engine._stale_reason or 'the engine tables changed'} since "
                             "capture_pair()): replaying it would launch kernels that hold the old values; capture again")
        self.graph.replay()


class DenoiseEngine:
    """One direction (``target`` in {"video","audio"}) of the CFG + DDIM loop for a batch of independent samples.

    step(z, t_now, t_prev)   one step, explicit timesteps (int64 [B] on the device) — parity entry point
    run(z, sched)            whole trajectory with the schedule cursor on the device; ``graph=True`` replays a
                             captured HIP graph per step (no per-step host work beyond one graph launch)

    ``noise_seed`` (extension; default None = the reference's ``randn_like`` per step, schedule_utils.py:197): with eta > 0 the
    step draws its noise inside the fused CFG + DDIM kernel from the seeded normal stream (include/avdiff_hip.h, avd_noise_key),
    keyed by (noise_seed, sample_offset + b, t_now[b], element) — no noise buffer, and the graph replay of ``run`` applies as at
    eta == 0.  ``sample_offset`` is the global index of this batch's sample 0 (a batch that is one slice of a larger job draws the
    same noise as the whole job would).  Both are fixed at construction; a captured graph holds them by value.

    ``solver`` (extension; default "ddim" = the reference's sampler): "dpmpp_2m" ends every step in the DPM-Solver++(2M) update
    (include/avdiff_hip.h, avd_dpmpp_2m_step_f32) inside the same fused CFG kernel — second order, one model call per step.  With
    eta > 0 it is the solver's SDE form (SDE-DPM-Solver++(2M), avd_dpmpp_2m_sde_step_f32; k-diffusion's "DPM++ 2M SDE"): it needs
    ``noise_seed`` (seeded noise only — the stream the DDIM step draws, so both solvers see the same normals at a (sample, t,
    element)), and every kind of step — CFG, CFG-controlled, guided, cond-only, canvas-keyed — goes through one entry
    (avd_denoise_step_dpmpp_2m_sde_f32).  The engine owns the solver's history ``x0_hist`` (the previous step's x0, allocated once: a captured graph keeps its
    address); ``step(..., t_last=None)`` takes a first-order step, and ``run`` starts every trajectory first order.

    ``set_known(known, mask)`` (extension: latent inpainting / outpainting, SDEdit): while a known clean latent is set, every step
    ends in the latent guide's blend (include/avdiff_hip.h, avd_latent_guide) inside the same fused kernel — z_out = blend(mask,
    q(t_prev), step(z)) with q the known latent forward-noised to t_prev along the known-noise stream of (guide_seed,
    sample_offset + b).  ``start_latent`` builds the trajectory's start for a ``strength``; ``clear_known`` returns to the plain
    step.  The known latent and the mask live in engine-owned buffers, so a captured graph replays guided steps.

    ``guidance`` a number (today's scalar CFG) or B per-sample scales, ``guidance_rescale`` phi in [0, 1], a number or B values
    (extension: per-sample guidance and CFG rescale, include/avdiff_hip.h, avd_cfg_control; diffusers' ``rescale_noise_cfg`` per
    sample).  With either in use every step runs the controlled fused kernel — after a statistics pass over the eps when any phi is
    set; a scalar guidance with phi = 0 is the plain step, bit for bit and kernel for kernel.  ``set_cfg`` changes the values in
    engine-owned buffers (a captured graph follows them); switching between the plain and the controlled step starts a new graph
    generation.

    ``apg`` (extension: adaptive projected guidance, Sadat et al. 2024, diffusers' ``AdaptiveProjectedGuidance``; include/avdiff_hip.h,
    "adaptive projected guidance"; default None = off): a dict with any of ``norm_threshold`` (r >= 0, 0 = no cap on the norm of the
    guidance direction), ``eta_parallel`` (in [0, 1]: the kept share of the direction's component parallel to the conditional
    prediction) and ``momentum`` (beta, negative in the paper; 0 = none).  Every CFG step then runs a statistics pass over the eps and
    steps, inside the same fused kernel, on cond + (g - 1) s (d - k cond) instead of the CFG combine; per-sample ``guidance`` applies,
    ``guidance_rescale`` != 0 beside it is refused.  The engine owns the statistics scratch and, with momentum, the per-element
    momentum buffer (``apg_momentum``; zeroed by ``begin`` — so by every ``run`` — and by ``start_latent``; updated in place, so a
    captured pair leaves it at its address).  Cond-only steps of a guidance interval do not apply it and leave the buffer untouched;
    ``rewind`` and ``renoise`` (RePaint resampling) carry the buffer as it is: the direction's running average goes on across a jump.
    ``set_apg`` / ``clear_apg`` change it and start a new graph generation (the parameters are held by value).  ``step_slots`` and the
    FIFO queue refuse it, as they refuse every per-sample CFG control: their form is ``set_slot_cfg`` (guidance by noise level, per-slot
    rescale and APG, whose momentum is a per-slot buffer that travels with the slot; include/avdiff_hip.h, "slot CFG control" and
    "slot APG momentum").  What it does to sample quality at a given guidance
    scale is not measured here: that needs trained weights.

    ``guidance_interval`` (extension: guidance in a limited interval, Kynkaanniemi et al. 2024; default None = every step is a CFG
    step): (t_lo, t_hi) in training timesteps, both ends inclusive.  ``run`` takes a CFG step — today's step, whichever form the
    engine runs — where t_lo <= t_now <= t_hi, and a cond-only step elsewhere (include/avdiff_hip.h, "guidance interval"): eps =
    eps_cond, the null branch is not computed (B*N rows through the model instead of 2B*N), per-sample guidance and rescale do not
    apply; the seeded noise, the DPM history and the latent guide carry on across the two kinds.  ``step`` / ``advance`` take
    explicit device timesteps and do not read them: there the caller picks the kind with ``cond_only``.  ``set_guidance_interval``
    changes the interval for the next ``run``; it is a host-side decision and leaves captured graphs valid.

    ``set_window_consensus(hop, weights=None)`` (extension: latent window consensus, MultiDiffusion-style co-denoising, Bar-Tal et
    al. 2023; default off): the batch is N consecutive windows of one latent canvas, window k at positions k*hop .. k*hop + L - 1 of
    the sliding axis (T of a video latent, F of an audio latent).  While set, every kind of step ends with one more launch on the
    same stream (include/avdiff_hip.h, avd_window_consensus_f32) that replaces, in ``out``, every canvas position under several
    windows by their weighted mean, so the windows take the next step from latents that agree wherever they overlap.  It is part
    of ``step``: ``capture_pair`` captures it and ``run(graph=True)`` replays it.  With the default per-sample noise stream it is
    eta == 0 only (the mean of independent noise draws would shrink their variance); a canvas-keyed engine (below) lifts that for
    hop == canvas_hop.  DPM-Solver++(2M) needs nothing extra: all windows share the timesteps, so the update is the
    same linear map of (z, x0, x0_hist) for every window — at eta > 0 plus the canvas-keyed noise term the windows share — and the
    consensus of the outputs equals the output of the consensed inputs; ``x0_hist`` stays per window.

    ``noise_keying`` (extension; default "sample" = the stream above): "canvas" needs ``noise_seed`` and an integer ``canvas_hop`` >=
    1 and reads the batch as N consecutive windows of one canvas, ``canvas_hop`` latent positions apart, window 0 at global window
    index ``sample_offset``.  At eta > 0 every CFG, CFG-controlled, guided and cond-only step of either solver then draws its noise keyed by
    (noise_seed, canvas position, t_now, element of that position's slice) (include/avdiff_hip.h, "canvas-keyed noise";
    avd_denoise_step_canvas_f32): all windows over a canvas position draw the same normal there, so the noise term passes through
    the consensus mean unchanged for any weights, and ``set_window_consensus(hop)`` is allowed at eta > 0 when hop == canvas_hop.
    (sample_offset + N - 1) * canvas_hop + L <= 2**32 replaces the per-sample range check.  Both values are fixed at construction; a
    captured graph holds them by value.  ``noise=`` is refused as on any seeded engine.  At eta == 0 no noise is drawn and the keying
    changes nothing.

    ``set_known(..., keying="canvas", hop=...)`` (extension; default "sample" = the stream above): the same second keying for the
    latent guide's known noise (include/avdiff_hip.h, "canvas-keyed known noise"): the batch is N consecutive windows of one canvas
    ``hop`` positions apart and every window draws the same known normal at a shared canvas position, so a held region passes through
    the consensus mean on its forward path (keyed per sample, the mean over an overlap would shrink its noise term).  Every step of
    such an engine — either solver, eta == 0 or > 0, CFG, CFG-controlled, cond-only — goes through one entry
    (avd_denoise_step_canvas_guided_f32), and ``start_latent`` forward-noises with the same keying.  ``hop`` must equal ``canvas_hop``
    on a canvas-keyed engine and the consensus hop while a consensus is set; eta > 0 needs the canvas-keyed engine (a canvas guide
    with per-sample step noise is refused).  The known windows must agree on their overlaps (``functional.window_consensus`` once).

    RePaint resampling (extension; Lugmayr et al. 2022): ``run`` accepts a schedule with up-jumps (schedule_utils.resample_schedule).
    A pair sched[i] < sched[i + 1] is not a denoising step but a forward jump, ``renoise`` (include/avdiff_hip.h, "renoise"): the
    latent is noised from sched[i] to sched[i + 1] with fresh seeded normals named by visit = i, and under ``set_known`` the held
    region lands on its forward path there; the stretch below is then denoised again, so the free and the held region meet at a
    common noise level more than once.  It needs ``noise_seed`` (also at eta == 0); the keying is the engine's (by canvas position
    with ``canvas_hop`` or a canvas-keyed guide, which a window consensus requires).  Limit: at eta > 0 the step noise stays keyed by
    (sample, t_now, element), so a revisited timestep repeats its step normals; only the renoise normals are fresh per visit.

    ``step_slots(z, t_now, t_prev)`` (extension: slot timesteps, include/avdiff_hip.h): one (t_now, t_prev) pair per token position
    of the sliding axis ([B, S] tables, S = ``slots`` of ``slot_len`` latent positions) instead of one per sample; a slot with t_prev ==
    t_now is held.  The primitive of FIFO diagonal denoising (``stream_infer.fifo_denoise``, ``schedule_utils.fifo_plan``).  Either
    solver with the scalar guidance only: solver "dpmpp_2m" takes a third table ``t_last`` and keeps its history per
    element in ``x0_hist``, which ``fifo_shift`` moves along with the queue.  At eta > 0 it needs ``noise_seed`` and ``clip_first``,
    the clip slot the batch starts at: every stepping slot draws its noise keyed by (noise_seed, the clip position it holds, its
    t_now, element) under a domain tag of its own (include/avdiff_hip.h, "clip-keyed slot noise"), so a clip slot's draws do not
    depend on the queue layout, on which sample holds it or on eager / replayed launches.  ``step``, ``run`` and ``capture_pair`` do
    not change.

    ``fifo_open`` / ``fifo_ramp`` / ``fifo_steady`` / ``fifo_capture`` (extension: a FIFO queue whose iterations read the ramp row and
    the clip slot off device cursors, include/avdiff_hip.h, "FIFO device cursors"): what ``fifo_denoise(graph=True)`` replays.  An
    iteration is the same chain of launches eagerly and under capture; a captured pair belongs to the queue it was captured on.

    ``fifo_lookahead(z, ctx, shift, ...)`` (extension: overlapping queue windows with held context, include/avdiff_hip.h, "FIFO
    lookahead"): the queue step of ``fifo_denoise(lookahead=ctx)``; it moves ``x0_hist`` as ``fifo_shift`` does.

    ``fifo_shift_clips(z, queues, c, t, seeds, clips, m)`` (extension: K queues in lockstep in one batch, include/avdiff_hip.h, "FIFO
    clip batch"): the queue step of ``stream_infer.fifo_denoise_clips``; one launch moves every queue, ``x0_hist`` and the slot momentum.
    """

    SOLVERS = ("ddim", "dpmpp_2m")
    NOISE_KEYINGS = ("sample", "canvas")
    GUIDE_KEYINGS = ("sample", "canvas")

    def __init__(self, *, adapt_v: LinearAdapter, adapt_a: LinearAdapter, core: MMDiT, head: MultiModalNoiseHead,
                 tstep_dim: int, target: str, latent_shape: Tuple[int, ...], prompt_tokens: int, alpha_bar: torch.Tensor,
                 guidance: float, eta: float = 0.0, tube=(2, 4, 4), chunk=(4, 4), split_streams: Optional[bool] = None,
                 temb_mode: str = "concat", matmul: Optional[str] = None, attn: Optional[str] = None,
                 noise_seed: Optional[int] = None, sample_offset: int = 0, solver: str = "ddim", guidance_rescale=0.0,
                 guidance_interval=None, noise_keying: str = "sample", canvas_hop: Optional[int] = None, apg=None):
        if target not in ("video", "audio"):
            raise ValueError("target must be 'video' or 'audio'")
        if eta < 0:
            raise ValueError("eta must be >= 0")
        if solver not in self.SOLVERS:
            raise ValueError(f"solver must be one of {self.SOLVERS}, got {solver!r}")
        if solver == "dpmpp_2m" and eta > 0 and noise_seed is None:
            raise ValueError("solver 'dpmpp_2m' with eta > 0 (its SDE form) draws seeded noise only: pass noise_seed, or eta = 0 for the "
                             "deterministic (ODE) solver")
        self.solver = solver
        self.guidance_interval = su.check_guidance_interval(guidance_interval)
        self._last_cond_only = False      # the kind of the last step: what eps_tokens() finds in the workspace
        if temb_mode not in ("concat", "add"):
            raise ValueError("temb_mode must be 'concat' (sampler, sample_clip.py:59-70) or 'add' (trainer, trainer.py:45-49)")
        self.temb_mode = temb_mode
        self.target = target
        self.core, self.head = core, head
        self.adapt_t = adapt_v if target == "video" else adapt_a
        self.adapt_p = adapt_a if target == "video" else adapt_v
        self.d = core.cfg.d_model
        self.tdim = self.d if temb_mode == "add" else int(tstep_dim)     # the trainer embeds at token width
        self.tube, self.chunk = tuple(tube), tuple(chunk)
        self.eta = float(eta)
        self.device = next(core.final_norm.parameters()).device
        if not self.device.type == "cuda":
            raise L.AvdError("DenoiseEngine needs its modules on a ROCm device (no CPU fallback)")
        self.latent_shape = tuple(int(s) for s in latent_shape)      # with batch dim
        B = self.latent_shape[0]
        # CFG control (set_cfg): the values on the host, and the [B] device buffers + statistics scratch once a step needs them
        self._g_vals, self._g_per_sample = Fn.cfg_values(guidance, B, "guidance"), not _scalar_like(guidance)
        self._phi_vals = Fn.cfg_values(guidance_rescale, B, "guidance_rescale", 0.0, 1.0)
        self.guidance = float(self._g_vals[0])
        self._cfg_g = self._cfg_phi = self._cfg_stats = None
        self._ctl: Optional[L.CfgControl] = None
        self._cfg_sig = None          # what a captured graph holds of the control by value: its pointers
        # adaptive projected guidance (set_apg): the parameters on the host, the scratch and the momentum buffer once a step needs them
        self._apg_vals = self._check_apg(Fn.apg_from_dict(apg), self._phi_vals)
        self._apg: Optional[L.ApgControl] = None
        self._apg_stats: Optional[torch.Tensor] = None
        self.apg_momentum: Optional[torch.Tensor] = None
        self._apg_sig = None          # what a captured graph holds of it by value: the parameters and the two pointers
        self.noise_seed, self.sample_offset = noise_seed, int(sample_offset)
        self._key = None if noise_seed is None else Fn.noise_key(noise_seed, sample_offset)
        if self._key is None and sample_offset != 0:
            raise ValueError("sample_offset keys the seeded noise: it needs noise_seed")
        if noise_keying not in self.NOISE_KEYINGS:
            raise ValueError(f"noise_keying must be one of {self.NOISE_KEYINGS}, got {noise_keying!r}")
        self.noise_keying, self.canvas_hop = noise_keying, None
        if noise_keying == "canvas":
            if self._key is None:
                raise ValueError("noise_keying='canvas' keys the seeded noise stream by canvas position: it needs noise_seed")
            if canvas_hop is None:
                raise ValueError("noise_keying='canvas' needs canvas_hop: the latent positions from one window of the batch to the next")
            self.canvas_hop = Fn.check_canvas_keying(self.latent_shape, canvas_hop, self.sample_offset)
        elif canvas_hop is not None:
            raise ValueError("canvas_hop belongs to noise_keying='canvas'")
        elif self._key is not None and sample_offset + B > 2 ** 32:
            raise ValueError(f"sample_offset {sample_offset} + batch {B} exceeds the stream's 2**32 sample indices")
        e = L.EmbedDesc()
        e.B, e.d, e.tdim = B, self.d, self.tdim
        if target == "video":
            _, Cc, T, H, W = self.latent_shape
            t, h, w = self.tube
            assert T % t == 0 and H % h == 0 and W % w == 0, "tube sizes must divide latent dims"
            e.target_kind, e.target_first = 0, 1                     # sequence order is always [video ; audio]
            e.C, e.T, e.H, e.W = Cc, T, H, W
            e.p0, e.p1, e.p2 = t, h, w
            e.Nt = (T // t) * (H // h) * (W // w)
        else:
            _, Ca, Fa = self.latent_shape
            ln, st = self.chunk
            e.target_kind, e.target_first = 1, 0
            e.C, e.T, e.H, e.W = Ca, Fa, 1, 1
            e.p0, e.p1, e.p2 = ln, st, 1
            e.Nt = (Fa - ln) // st + 1
        e.Np = int(prompt_tokens)
        self._freqs = Fn.temb_freqs(self.tdim, 10000, self.device) if self.tdim >= 2 else None
        e.temb_freqs = L.ptr(self._freqs)
        e.temb_add = 1 if temb_mode == "add" else 0
        w_out = self.adapt_t.proj.weight.shape[0]
        if w_out != (self.d if temb_mode == "add" else self.d - self.tdim):
            raise ValueError(f"adapter width {w_out} does not match temb_mode='{temb_mode}' (d={self.d}, tdim={self.tdim})")
        self.embed = e
        self.N = e.Nt + e.Np
        self.alpha_bar = alpha_bar.to(self.device, torch.float32).contiguous()

        # matrix-pipe mode of this engine (a key of _lib.MATMUL_TERMS; default: the core's own setting, "auto" unless changed); the core
        # module keeps its setting
        self.matmul = core.matmul if matmul is None else matmul
        self.attn = core.attn if attn is None else attn
        # cond / null halves as two kernel chains on two HIP streams (bit-identical results).  Default: on where it was measured to
        # pay — the f16x2 mode, whose kernels alternate matrix-bound loops with memory-bound epilogues, with >= 6144 rows per half
        # (C3: 166 -> 174 steps/s, 512x512: 137 -> 144) — and the bf16x3 mode where the null half's short layout applies (audio ->
        # video in concat mode with two or more prompt tokens), as split_streams="short": the cond half on the caller's stream, the
        # null half with one prompt row per sample on the second (C3: 122.5 -> 128.9 steps/s, profiles/two_stream_dedup_e2e.txt), from
        # 24,321 stacked rows 2 B N: the size from which out_proj / fc2 run as one generation of one-block-per-CU launches, whose
        # launch, fill and epilogue phases the other chain covers, and the regime of the six-run record.  Smaller batches gained in
        # three-run sweeps too (same file); they keep the one-stream default, which tests/test_gpu_f16x2.py pins at 6,736 rows per half.
        # "short" where that layout does not apply is the one-stream step.  True keeps the full layout in both chains, which bf16x3
        # and the fp32 mode lose by.
        short_applies = (self.matmul == "bf16x3" and self.attn != "fp8" and temb_mode == "concat" and target == "video" and e.Np >= 2)
        if split_streams is None:
            if self.matmul == "f16x2":
                split_streams = B * self.N >= 6144
            else:
                split_streams = "short" if short_applies and 2 * B * self.N >= 24321 else False
        if isinstance(split_streams, str):
            if split_streams != "short":
                raise ValueError(f"split_streams must be None, a bool or 'short', got {split_streams!r}")
            self._split_short = self._split_streams = short_applies
        else:
            self._split_short, self._split_streams = False, bool(split_streams)
        # generation of the pointer / scalar tables: bumped whenever something a captured HIP graph holds by value changes
        # (see _CapturedPair); _stale_reason says what changed last
        self._generation = 0
        self._stale_reason = ""
        self.workspace: Optional[torch.Tensor] = None
        self.Xp: Optional[torch.Tensor] = None
        self._prompt_latent: Optional[torch.Tensor] = None
        # DPM-Solver++(2M) history: the previous step's x0, and the all -1 t_last of a first-order step (both at fixed addresses)
        self.x0_hist: Optional[torch.Tensor] = None
        if solver == "dpmpp_2m":
            self.x0_hist = torch.zeros(self.latent_shape, device=self.device, dtype=torch.float32)
            self._no_hist = torch.full((B,), -1, dtype=torch.long, device=self.device)
        self._hist_other: Optional[torch.Tensor] = None      # fifo_shift's second history buffer: the shift is out of place
        # latent guide (set_known): the known latent and the mask at fixed addresses, and the avd_latent_guide over them
        self._known: Optional[torch.Tensor] = None
        self._mask: Optional[torch.Tensor] = None
        self._guide: Optional[L.LatentGuide] = None
        self._guide_sig = None       # what a captured graph holds of the guide by value: pointers, stride, seed, offset, keying, hop
        self._guide_hop: Optional[int] = None      # the hop of a canvas-keyed guide (None: keyed per sample)
        # clip-keyed latent guide (set_clip_guide): (known canvas, mask canvas or None, seed), a state of its own beside set_known's
        self._clip = None
        # slot CFG control (set_slot_cfg): the avd_slot_cfg over engine-owned level tables and scratch, None = off
        self._scfg: Optional[L.SlotCfg] = None
        self._scfg_g = self._scfg_phi = self._scfg_stats = None
        # window consensus (set_window_consensus): the hop (None = off) and the [L] weight table at a fixed address
        self._cons_hop: Optional[int] = None
        self._cons_w: Optional[torch.Tensor] = None
        self._bind_weights()
        self._apply_cfg()
        self._apply_apg()

    # ---- pointer tables.  They hold derived copies (norm-folded / split3 weights), so they are re-derived whenever a
    # parameter's (address, version) changes: load_state_dict, EMA copy_to, an optimiser step or .to(device) after the
    # engine was built all show up here, at the next step, instead of mixing old and new weights silently.
    def _weights_key(self):
        mods = (self.core, self.head, self.adapt_t, self.adapt_p)
        return tuple((p.data_ptr(), p._version) for m in mods for p in m.parameters())

    def _bind_weights(self) -> None:
        core, head = self.core, self.head
        prev = core.matmul, core.attn
        core.matmul, core.attn = self.matmul, self.attn
        try:
            self._core_tab, self._keep_core = core.weight_table()
        finally:
            core.matmul, core.attn = prev
        # the head follows the engine's mode; its input rows are the core's final-norm output, bounded by that norm's parameters:
        # RMSNorm |y_i| <= sqrt(d) |g_i|, ||y|| <= sqrt(d) max|g|; LayerNorm adds |b_i| resp. ||b||
        hb = hn = None
        if self.matmul == "f16x2":
            fn_ = core.final_norm
            bias = getattr(fn_, "bias", None)
            g = fn_.weight if bias is not None else fn_.scale
            bd = Fn.weight_bounds([g] + ([bias] if bias is not None else []))
            gmax = bd[0][0] * core.cfg.d_model ** 0.5
            hb = gmax + (bd[1][0] if bias is not None else 0.0)
            hn = gmax + (bd[1][1] if bias is not None else 0.0)
        self._head_tab, self._keep_head = head.weight_table(self.target, matmul=self.matmul, in_bound=hb, in_norm=hn)
        self._aw = L.dev_f32(self.adapt_t.proj.weight.detach(), "adapter weight")
        self._ab = L.dev_f32(self.adapt_t.proj.bias.detach(), "adapter bias")
        if self._aw.device != self.device:
            raise L.AvdError("engine modules moved to another device after the engine was built")
        s = L.StepDesc()
        s.embed = self.embed
        s.core = C.pointer(self._core_tab)
        s.head = C.pointer(self._head_tab)
        s.adapt_w, s.adapt_b = self._aw.data_ptr(), self._ab.data_ptr()
        s.alpha_bar, s.T_train = self.alpha_bar.data_ptr(), self.alpha_bar.numel()
        s.guidance, s.eta = self.guidance, self.eta
        s.split_streams = 2 if self._split_short else 1 if self._split_streams else 0
        self.desc = s
        need = L.lib().avd_step_workspace_bytes(C.byref(s))
        if need < 0:
            raise ValueError(L.lib().avd_last_error().decode())
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        self._ptrs = self._table_ptrs()
        self._scalars = self._table_scalars()
        self._wkey = self._weights_key()

    def _table_ptrs(self):
        return tuple(t.data_ptr() for t in self._keep_core[1]) + tuple(t.data_ptr() for t in self._keep_head[1]) + \
            (self._aw.data_ptr(), self._ab.data_ptr(), self.workspace.data_ptr(), self.alpha_bar.data_ptr())

    def _table_scalars(self):
        """Every BY-VALUE number of the tables: a captured HIP graph bakes these into its kernel arguments (the f16x2 image scales
        become 1/(s_A s_W) factors and split scales of the launches), so unlike weights behind unchanged pointers they do not follow
        an in-place parameter update."""
        cw, hw = self._core_tab, self._head_tab
        blocks = self._keep_core[0]
        out = [cw.d, cw.n_layers, cw.n_heads, cw.mlp_hidden, cw.norm_eps, cw.norm_kind, cw.split_terms, cw.attn_mode,
               hw.d_in, hw.hidden, hw.d_out, hw.n_shared, hw.ln_eps, hw.act, hw.split_terms, self.guidance, self.eta]
        if cw.split_terms == 3:
            for i in range(cw.n_layers):
                out += list(blocks[i].f16x2_scale)
        if hw.split_terms == 3 and hw.f16x2_scale:
            out += [hw.f16x2_scale[i] for i in range(2 * (hw.n_shared + 2))]
        return tuple(float(v) for v in out)

    def _sync_weights(self) -> None:
        if self._weights_key() == self._wkey:
            return
        old, old_sc = self._ptrs, self._scalars
        self._bind_weights()             # derived copies are refreshed in place where shapes allow
        if self._ptrs != old:
            self._generation += 1
            self._stale_reason = "a parameter or the workspace was re-allocated"
        elif self._scalars != old_sc:
            self._generation += 1
            self._stale_reason = ("an in-place parameter update changed a scale that a captured HIP graph holds by value (f16x2 image "
                                  "scales follow max|w| and the norm gains)")
        if self._prompt_latent is not None:
            self.set_prompt(self._prompt_latent)     # the cached prompt rows depend on the prompt adapter (same buffer: in place)

    # ---- prompt rows: adapter(tokens(prompt latent)) | temb(0); constant over the trajectory ----
    def set_prompt(self, prompt_latent: torch.Tensor) -> torch.Tensor:
        z = L.dev_f32(prompt_latent, "prompt latent")
        self._prompt_latent = z
        B = self.embed.B
        if z.shape[0] != B:
            raise ValueError("prompt batch size must match the engine's")
        tok = self._prompt_tokens(z)
        if tok.shape[1] != self.embed.Np:
            raise ValueError(f"prompt yields {tok.shape[1]} tokens, engine was built for {self.embed.Np}")
        d = self.d
        # the prompt rows keep their buffer from call to call (a captured graph holds its address); a first call, or one after the
        # buffer was dropped, starts a new table generation
        Xp = self.Xp
        if Xp is None or tuple(Xp.shape) != (B, tok.shape[1], d) or Xp.device != self.device:
            Xp = torch.empty(B, tok.shape[1], d, device=self.device, dtype=torch.float32)
            self._generation += 1
            self._stale_reason = "the prompt rows were (re-)allocated by set_prompt()"
        self._prompt_rows(tok, Xp)
        self.Xp = Xp
        return Xp

    def _prompt_tokens(self, z: torch.Tensor) -> torch.Tensor:
        return latents_to_tokens_audio(z, *self.chunk) if self.target == "video" else ops.tube_patch_video(z, *self.tube)

    def _prompt_rows(self, tok: torch.Tensor, Xp: torch.Tensor, temb: bool = True) -> None:
        """``set_prompt``'s device work behind the tokens: the adapter GEMM into ``Xp`` and, with ``temb``, the timestep-0 embedding.
        ``temb=False`` (concat mode only) leaves Xp's timestep columns as they are: they are constant, so a FIFO queue writes them once
        when it is opened and every steady iteration renews the adapter columns alone — launches only, no host synchronisation."""
        B, d, td = self.embed.B, self.d, self.tdim
        w, b = self.adapt_p.proj.weight.detach(), self.adapt_p.proj.bias.detach()
        t0 = su.timestep_embedding(torch.zeros(B, dtype=torch.long, device=self.device), td) if td and temb else None
        if self.temb_mode == "add":
            # adapter(tok) + temb(0): the broadcast embedding rides in as the GEMM's residual operand
            res = t0[:, None, :].expand(B, tok.shape[1], d).contiguous()
            L.check(L.lib().avd_gemm_bias_act_f32(tok.data_ptr(), tok.shape[2], L.dev_f32(w).data_ptr(), L.dev_f32(b).data_ptr(),
                                                  res.data_ptr(), d, Xp.data_ptr(), d, B * tok.shape[1], d, tok.shape[2],
                                                  L.ACT_NONE, L.stream_ptr(self.device)))
        else:
            # GEMM writes straight into the first d-tdim columns (ldc = d)
            L.check(L.lib().avd_gemm_bias_act_f32(tok.data_ptr(), tok.shape[2], L.dev_f32(w).data_ptr(), L.dev_f32(b).data_ptr(),
                                                  None, 0, Xp.data_ptr(), d, B * tok.shape[1], d - td, tok.shape[2],
                                                  L.ACT_NONE, L.stream_ptr(self.device)))
            if t0 is not None:
                Xp[..., d - td:] = t0[:, None, :]

    # ---- latent guide: a known clean latent the trajectory is held to (inpainting / outpainting) or starts from (SDEdit) ----
    def set_known(self, known: torch.Tensor, mask: Optional[torch.Tensor] = None, *, guide_seed: int = 0, keying: str = "sample",
                  hop: Optional[int] = None, sample_offset: Optional[int] = None) -> None:
        """Hold the trajectory to ``known`` (the clean latent, the engine's latent shape) where ``mask`` is 1, blend where it is
        fractional, leave it free where it is 0.  ``mask``: None = 1 everywhere, else values in [0, 1] broadcastable to one
        sample's latent shape (shared by the batch) or to the batch's.  ``guide_seed`` keys the known-noise stream with
        ``sample_offset`` (default: the engine's; the global index of this batch's sample — or window — 0 in that stream).
        ``keying``: "sample" (the stream of (guide_seed, sample_offset + b)) or "canvas" with ``hop`` (class docstring: the batch as
        windows of one canvas, the known noise keyed by canvas position).  Everything is checked before anything changes.  Known
        latent and mask are copied into engine-owned buffers: a later call with the same shapes, mask presence, seed, offset, keying
        and hop keeps every captured graph valid."""
        if keying not in self.GUIDE_KEYINGS:
            raise ValueError(f"keying must be one of {self.GUIDE_KEYINGS}, got {keying!r}")
        offset = self.sample_offset if sample_offset is None else sample_offset
        Fn.noise_key(guide_seed, offset)                     # validates the seed and the offset
        if keying == "canvas":
            if hop is None:
                raise ValueError("keying='canvas' needs hop: the latent positions from one window of the batch to the next")
            hop = Fn.check_canvas_keying(self.latent_shape, hop, offset)
            if self.canvas_hop is not None and hop != self.canvas_hop:
                raise ValueError(f"a canvas-keyed guide needs hop == canvas_hop (the engine's noise is keyed for windows {self.canvas_hop} "
                                 f"positions apart), got hop {hop}")
            if self._cons_hop is not None and hop != self._cons_hop:
                raise ValueError(f"a canvas-keyed guide needs hop == the window consensus hop {self._cons_hop}, got hop {hop}")
            if self.eta > 0 and self.canvas_hop is None:
                raise ValueError("a canvas-keyed guide at eta > 0 needs the step's noise keyed by canvas position as well: build the "
                                 "engine with noise_keying='canvas', canvas_hop=hop (per-sample step noise is refused)")
        elif hop is not None:
            raise ValueError("hop belongs to keying='canvas'")
        elif offset + self.latent_shape[0] > 2 ** 32:
            raise ValueError(f"sample_offset {offset} + batch {self.latent_shape[0]} exceeds the stream's 2**32 sample indices")
        known = L.dev_f32(known, "known")
        if tuple(known.shape) != self.latent_shape:
            raise ValueError(f"known latent shape {tuple(known.shape)} != engine shape {self.latent_shape}")
        m = None
        if mask is not None:
            m = torch.as_tensor(mask).to(self.device, torch.float32)
            shape = self.latent_shape[1:] if m.dim() < len(self.latent_shape) else self.latent_shape
            try:
                m = m.expand(shape)
            except RuntimeError:
                raise ValueError(f"mask shape {tuple(m.shape)} does not broadcast to {self.latent_shape[1:]} or "
                                 f"{self.latent_shape}") from None
            if not bool(((m >= 0) & (m <= 1)).all()):
                raise ValueError("mask values must lie in [0, 1]")
        if self._known is None:
            self._known = torch.empty(self.latent_shape, device=self.device, dtype=torch.float32)
        self._known.copy_(known)
        if m is not None:
            if self._mask is None or tuple(self._mask.shape) != tuple(m.shape):
                self._mask = torch.empty(tuple(m.shape), device=self.device, dtype=torch.float32)
            self._mask.copy_(m)
        self._guide = Fn.latent_guide_desc(self._known, self._mask if m is not None else None, guide_seed, offset)
        self._guide_hop = hop
        self._touch_guide()

    def clear_known(self) -> None:
        """Back to the plain step (the buffers are kept for a later set_known)."""
        self._guide = None
        self._touch_guide()

    # ---- clip-keyed latent guide: a known clean clip canvas that ``step_slots`` holds every slot to, by the clip position it holds ----
    def set_clip_guide(self, known_canvas: torch.Tensor, mask: Optional[torch.Tensor] = None, *, guide_seed: int = 0) -> None:
        """Guide ``step_slots`` by a clean clip canvas (extension; include/avdiff_hip.h, "clip-keyed latent guide"):
        ``known_canvas`` [C, P, H, W] (video target) or [Ca, P] (audio target) is the whole clip along the sliding axis, ``mask`` None
        (1 everywhere) or values in [0, 1] broadcastable to the canvas (``canvas_frame_mask`` gives one): after every stepping slot's
        update the slot is blended, by the clip positions it holds (``step_slots``'s ``clip_first``, required while the guide is set),
        with the known canvas forward-noised to the slot's own t_prev — 1 keeps the clip, 0 leaves the trajectory free, positions
        outside the canvas are unguided.  The known noise is keyed by ``guide_seed`` and clip position (the stream of
        ``set_known(keying="canvas")``).  Both canvases are copied into engine-owned buffers.  It is a state of its own: ``set_known``
        stays the guide of ``step`` / ``run``, which refuse a clip guide, as do ``fifo_open`` and ``fifo_lookahead``."""
        Fn.noise_key(guide_seed, 0)
        want = self.latent_shape[1:2] + self.latent_shape[3:]
        k = torch.as_tensor(known_canvas)
        if k.dim() != len(self.latent_shape) - 1 or tuple(k.shape[:1]) + tuple(k.shape[2:]) != want or k.shape[1] < 1:
            raise ValueError(f"known canvas shape {tuple(k.shape)} must be {want[:1] + ('P',) + want[1:]}: the engine's latent without "
                             "its batch axis, any P >= 1 along the sliding axis")
        if not k.is_floating_point():
            raise TypeError(f"known canvas must be a float tensor, got {k.dtype}")
        m = None
        if mask is not None:
            m = torch.as_tensor(mask).to(torch.float32)
            try:
                m = m.expand(tuple(k.shape))
            except RuntimeError:
                raise ValueError(f"mask shape {tuple(m.shape)} does not broadcast to the known canvas's {tuple(k.shape)}") from None
            if not bool(((m >= 0) & (m <= 1)).all()):
                raise ValueError("mask values must lie in [0, 1]")
            m = m.to(self.device).contiguous()
        self._clip = (k.to(self.device, torch.float32).contiguous().clone(), m, guide_seed)

    def clear_clip_guide(self) -> None:
        """Back to the unguided ``step_slots``."""
        self._clip = None

    def _clip_refusal(self, what: str, why: str) -> None:
        if self._clip is not None:
            raise ValueError(f"{what} takes no clip guide ({why}): clear_clip_guide() first")

    # ---- the K clip guides of a FIFO clip batch: one canvas, mask and seed per queue ("clip batch keying"); class-level None, so that
    # an engine that never sets them (or a shell built without __init__) reads "none"
    _clips: Optional[tuple] = None

    def set_clip_guides(self, known_canvases, masks=None, *, guide_seeds) -> None:
        """Guide ``step_slots(clip_queues=K)`` by K clean clip canvases, one per queue of a FIFO clip batch (extension;
        include/avdiff_hip.h, "clip batch keying"): ``known_canvases`` is K canvases of one shape as ``set_clip_guide`` takes one — a
        sequence, or a stacked tensor [K, C, P, H, W] / [K, Ca, P]; ``masks`` None (1 everywhere) or K masks, each broadcastable to a
        canvas (a stacked tensor broadcastable to the stack); ``guide_seeds`` K ints, the seeds of the queues' known-noise streams.
        Queue k's stepping slots end in the blend with canvas k at the clip positions they hold inside their own queue.  A state of its
        own: ``set_clip_guide`` stays one canvas for one queue, and ``step``, ``run``, ``fifo_open`` and ``fifo_lookahead`` refuse
        this one as they refuse that."""
        k = Fn.stack_clip_canvases(known_canvases)
        K = k.shape[0]
        want = self.latent_shape[1:2] + self.latent_shape[3:]
        if k.dim() != len(self.latent_shape) or tuple(k.shape[1:2]) + tuple(k.shape[3:]) != want or k.shape[2] < 1:
            raise ValueError(f"known canvases shape {tuple(k.shape)} must be {('K',) + want[:1] + ('P',) + want[1:]}: K times the engine's "
                             "latent without its batch axis, any P >= 1 along the sliding axis")
        if not k.is_floating_point():
            raise TypeError(f"known canvases must be float tensors, got {k.dtype}")
        if self.embed.B % K:
            raise ValueError(f"{K} canvases for an engine of batch {self.embed.B}: the queues must divide the batch")
        seeds = Fn.queue_seeds(guide_seeds, K)
        m = None
        if masks is not None:
            m = masks if isinstance(masks, torch.Tensor) else torch.stack([torch.as_tensor(x).to(torch.float32).expand(tuple(k.shape[1:]))
                                                                          for x in masks])
            try:
                m = m.to(torch.float32).expand(tuple(k.shape))
            except RuntimeError:
                raise ValueError(f"masks shape {tuple(m.shape)} does not broadcast to the known canvases' {tuple(k.shape)}") from None
            if not bool(((m >= 0) & (m <= 1)).all()):
                raise ValueError("mask values must lie in [0, 1]")
            m = m.to(self.device).contiguous()
        self._clips = (k.to(self.device, torch.float32).contiguous().clone(), m, seeds.to(self.device))

    def clear_clip_guides(self) -> None:
        """Back to the unguided ``step_slots(clip_queues=K)``."""
        self._clips = None

    def _clips_refusal(self, what: str) -> None:
        if self._clips is not None:
            raise ValueError(f"{what} takes no clip guides (they are the K canvases of step_slots(clip_queues=K)): clear_clip_guides() first")

    # ---- slot CFG control: guidance by noise level, per-slot guidance rescale and per-slot APG for ``step_slots`` ----
    # slot APG momentum (set_slot_cfg(apg_momentum=)): beta and the two engine-owned [B, per] buffers; class-level, so that an engine
    # that never sets one (or a shell built without __init__) reads "none"
    _smom_beta = 0.0
    _smom: Optional[torch.Tensor] = None
    _smom_other: Optional[torch.Tensor] = None

    def set_slot_cfg(self, guidance=None, rescale=None, apg=None, apg_momentum=None) -> None:
        """Control the CFG combine of ``step_slots`` per slot (extension; include/avdiff_hip.h, "slot CFG control"): ``guidance`` and
        ``rescale`` are ``schedule_utils.level_table`` specs — a number, T_train values or a callable t -> value — looked up inside the
        kernels at each slot's own t_now (``schedule_utils.guidance_interval_table`` gives the slot form of a guidance interval);
        ``rescale`` phi in [0, 1] rescales every stepping slot's combined eps to the std of its conditional eps, over the slot's own
        elements; ``apg`` {"norm_threshold":, "eta_parallel":} steps every slot on the adaptive projected guidance eps, its moments
        and its norm cap taken per slot (a threshold chosen for a whole sample of S slots corresponds to r / sqrt(S)).  None leaves a
        part off: the scalar guidance, no rescale, the plain combine.  Everything is checked before anything changes; the tables and
        the scratch are engine-owned, so a later call with new values reaches a captured step.  A ``rescale`` that is zero at every
        level launches no statistics pass.  It is a state of its own: ``set_cfg`` / ``set_apg`` stay the controls of ``step`` /
        ``run``, which refuse a slot control, as ``step_slots`` refuses theirs.
        ``apg_momentum`` (a finite number; needs ``apg``; None or 0 = none) is APG's momentum per slot (include/avdiff_hip.h, "slot APG
        momentum"): every stepping slot's direction becomes d = (cond - null) + apg_momentum * m_prev and is stored back, in two
        engine-owned zeroed [B, per] buffers in latent layout.  ``fifo_shift`` / ``fifo_lookahead`` / ``fifo_steady`` carry the live
        one into the other behind their move and the two swap, as the solver histories do, so a slot's momentum travels with it up
        the queue and an entering slot starts from zero; ``slot_momentum`` is the live buffer.  A call with a momentum keeps the
        buffers' contents when one was already set (zero them with ``slot_momentum.zero_()``)."""
        self._apply_slot_cfg(*self._check_slot_cfg(guidance, rescale, apg, apg_momentum))

    def _check_slot_cfg(self, guidance, rescale, apg, apg_momentum=None):
        """set_slot_cfg's checks alone, on the host: (guidance table or None, rescale table or None, (r, eta_p) or None, scratch bytes,
        the slot momentum beta)"""
        if apg_momentum is not None and apg is None:
            raise ValueError(f"apg_momentum {apg_momentum!r} needs apg: the momentum is adaptive projected guidance's")
        if guidance is None and rescale is None and apg is None:
            raise ValueError("set_slot_cfg needs guidance, rescale or apg (clear_slot_cfg() switches the control off)")
        T = int(self.alpha_bar.numel())
        g = None if guidance is None else su.level_table(guidance, T, "guidance")
        phi = None if rescale is None else su.level_table(rescale, T, "guidance_rescale", 0.0, 1.0)
        vals = Fn.apg_from_dict(apg)
        if vals is not None and vals[2] != 0.0:
            raise ValueError("the slot APG's dict takes no momentum: that key is the per-sample buffer of set_apg, which does not travel "
                             "with it through the queue's shift; a slot's momentum is set_slot_cfg(apg_momentum=) / "
                             "fifo_denoise(apg_momentum=) (the dict's momentum must be 0)")
        beta = 0.0
        if apg_momentum is not None:
            beta = Fn.apg_params(momentum=apg_momentum)[2]      # a number (not a bool), finite
        self._check_apg(vals, torch.zeros(1) if phi is None else phi)
        rescale_on = phi is not None and bool((phi != 0).any())      # phi = 0 at every level: no statistics pass (rescale_t NULL)
        nb = 0
        if rescale_on or vals is not None:
            per_slot = int(np.prod(self.latent_shape[1:])) // self.latent_shape[2] * self.slot_len
            nb = L.lib().avd_slot_cfg_stats_bytes(self.latent_shape[0], self.slots, per_slot)
            if nb < 0:
                raise ValueError(f"the slot CFG control needs >= 2 latent elements per slot and B * S <= 65535 (latent "
                                 f"{self.latent_shape}, {self.slots} slots)")
        return g, phi if rescale_on else None, None if vals is None else vals[:2], nb, beta

    def _apply_slot_cfg(self, g, phi, apg, nb, beta=0.0) -> None:
        dev, rescale_on, vals = self.device, phi is not None, apg
        if beta != 0.0 and self._smom is None:      # zeroed once: a slot that has not stepped has no momentum
            self._smom = torch.zeros(self.latent_shape, device=dev, dtype=torch.float32)
            self._smom_other = torch.zeros(self.latent_shape, device=dev, dtype=torch.float32)
        self._smom_beta = beta
        if g is not None:
            self._scfg_g = g.to(dev) if self._scfg_g is None else self._scfg_g.copy_(g)
        if rescale_on:
            self._scfg_phi = phi.to(dev) if self._scfg_phi is None else self._scfg_phi.copy_(phi)
        if nb and (self._scfg_stats is None or self._scfg_stats.numel() < nb):
            self._scfg_stats = torch.empty(nb, dtype=torch.uint8, device=dev)
        r, eta_p = (0.0, 0.0) if vals is None else vals
        base = (None if g is None else self._scfg_g.data_ptr(), self._scfg_phi.data_ptr() if rescale_on else None,
                0 if vals is None else 1, r, eta_p, self._scfg_stats.data_ptr() if nb else None, nb)
        if beta != 0.0:      # the control with its two trailing fields: apg says that they follow
            self._scfg = L.SlotCfgMomentum(*base[:2], L.SLOT_APG_MOMENTUM, *base[3:], beta, self._smom.data_ptr())
        else:
            self._scfg = L.SlotCfg(*base)

    def clear_slot_cfg(self) -> None:
        """Back to the scalar guidance and the plain combine in ``step_slots`` (the tables and the scratch are kept for a later
        set_slot_cfg; a slot momentum's state is dropped: its beta and both buffers)."""
        self._scfg = None
        self._smom_beta, self._smom, self._smom_other = 0.0, None, None

    @property
    def slot_momentum(self) -> Optional[torch.Tensor]:
        """the live slot APG momentum buffer, float32 of the latent's shape (None without ``set_slot_cfg(apg_momentum=)``): what the
        next ``step_slots`` reads and overwrites under its stepping slots"""
        return self._smom if self._smom_beta != 0.0 else None

    def _carry_slot_momentum(self, ctx: int, shift: int) -> None:
        """behind a queue move: the live momentum buffer through the same move into the other one (``functional.fifo_carry``), and the
        two swap; the control follows the live address.  Nothing without a slot momentum."""
        if self._smom_beta == 0.0:
            return
        Fn.fifo_carry(self._smom, self.slots, self.slot_len, ctx=ctx, shift=shift, out=self._smom_other)
        self._swap_slot_momentum()

    def _swap_slot_momentum(self) -> None:
        """behind a launch that moved the live momentum buffer into the other one: the two swap, the control follows the live address"""
        self._smom, self._smom_other = self._smom_other, self._smom
        self._scfg.momentum_buf = self._smom.data_ptr()

    def _move_hist(self, what: str, move, bump: bool = True):
        """An out-of-place queue move of the solver history: ``move(hist, hist_out)`` launches it from ``x0_hist`` into the engine's
        other history buffer (allocated on first use), then the two swap.  That changes an address a captured graph holds, so a new
        graph generation starts (``bump`` False inside a captured pair, whose two swaps put the address back).  Returns move's result."""
        if self._hist_other is None:
            self._hist_other = torch.empty_like(self.x0_hist)
        res = move(self.x0_hist, self._hist_other)
        self.x0_hist, self._hist_other = self._hist_other, self.x0_hist
        if bump:
            self._generation += 1
            self._stale_reason = f"{what} moved the solver history into the engine's other history buffer (x0_hist changed its address)"
        return res

    def slot_cfg_coef(self) -> torch.Tensor:
        """The per-slot coefficients the last controlled ``step_slots`` left in the scratch, float32 [B, S, 4] on the device:
        (s, g, phi, 0) under a rescale, (s, k, w, g) under APG (held slots: (1, 0, 0, 0)).  A view, overwritten by the next step."""
        if self._scfg is None or not self._scfg.stats:
            raise ValueError("no statistics pass is set: set_slot_cfg(rescale=...) or set_slot_cfg(apg=...) first")
        n = self.latent_shape[0] * self.slots
        return self._scfg_stats[self._scfg.stats_bytes - 16 * n:self._scfg.stats_bytes].view(torch.float32).view(-1, self.slots, 4)

    def _slot_cfg_refusal(self, what: str) -> None:
        if self._scfg is not None:
            raise ValueError(f"{what} takes no slot CFG control (its guidance and statistics are per slot of step_slots; a per-sample "
                             "step is controlled by set_cfg / set_apg): clear_slot_cfg() first")

    def _touch_guide(self) -> None:
        g = self._guide
        sig = None if g is None else (g.known, g.mask, g.mask_batch_stride, g.key.seed, g.key.sample_offset, self._guide_hop)
        if sig != self._guide_sig:
            self._generation += 1
            self._stale_reason = "the latent guide's buffers, mask presence, seed, sample offset, keying or hop changed (set_known / " \
                                 "clear_known)"
        self._guide_sig = sig

    # ---- CFG control: per-sample guidance scales and guidance rescale ----
    def set_cfg(self, guidance=None, rescale=None) -> None:
        """New CFG values: ``guidance`` a number (every sample) or B per-sample scales, ``rescale`` phi in [0, 1] (a number or B
        values); None keeps the current one.  Both are checked before anything changes.  They are copied into engine-owned buffers, so
        a captured graph replays with the new values — unless the step switches between the plain one (a scalar guidance, phi = 0
        everywhere) and the controlled one, phi goes from all zero to not (the statistics pass is launched only when some phi is set)
        or back, or a new scalar reaches the plain step (held by value): that starts a new generation."""
        B = self.embed.B
        g = None if guidance is None else Fn.cfg_values(guidance, B, "guidance")
        phi = None if rescale is None else Fn.cfg_values(rescale, B, "guidance_rescale", 0.0, 1.0)
        if phi is not None:
            self._check_apg(self._apg_vals, phi)
        if g is not None:
            self._g_vals, self._g_per_sample = g, not _scalar_like(guidance)
        if phi is not None:
            self._phi_vals = phi
        self._apply_cfg()

    def _apply_cfg(self) -> None:
        rescale = bool((self._phi_vals != 0).any())        # phi = 0 everywhere: no statistics pass (rescale pointer NULL)
        reason = None
        if self._g_per_sample or rescale:
            if self._cfg_g is None:
                B = self.embed.B
                nb = L.lib().avd_cfg_stats_bytes(B, int(np.prod(self.latent_shape[1:])))
                if nb < 0:
                    raise ValueError(f"the CFG control needs >= 2 latent elements per sample and B <= 65535 (latent {self.latent_shape})")
                self._cfg_g = torch.empty(B, dtype=torch.float32, device=self.device)
                self._cfg_phi = torch.empty(B, dtype=torch.float32, device=self.device)
                self._cfg_stats = torch.empty(nb, dtype=torch.uint8, device=self.device)
            self._cfg_g.copy_(self._g_vals)
            self._cfg_phi.copy_(self._phi_vals)
            self._ctl = L.CfgControl(self._cfg_g.data_ptr(), self._cfg_phi.data_ptr() if rescale else None, self._cfg_stats.data_ptr(),
                                     self._cfg_stats.numel())
            sig = (self._ctl.guidance, self._ctl.rescale, self._ctl.stats)
        else:
            self._ctl, sig = None, None
            g = float(self._g_vals[0])
            if g != self.guidance:
                self.guidance = self.desc.guidance = g
                reason = "the scalar guidance of the plain step changed (set_cfg)"
        if sig != self._cfg_sig:
            reason = "the CFG control was switched on or off, or its rescale (statistics pass) was (set_cfg)"
        self._cfg_sig = sig
        if reason:
            self._generation += 1
            self._stale_reason = reason

    # ---- adaptive projected guidance ----
    @staticmethod
    def _check_apg(vals, phi):
        """APG beside guidance rescale is refused: the rescale's statistics would need the APG output"""
        if vals is not None and bool((phi != 0).any()):
            raise ValueError("adaptive projected guidance (apg) cannot be combined with guidance_rescale != 0: the rescale's statistics "
                             "would need the APG output")
        return vals

    def set_apg(self, norm_threshold: float = 0.0, eta_parallel: float = 0.0, momentum: float = 0.0) -> None:
        """Switch adaptive projected guidance on, or change its parameters (class docstring).  Checked before anything changes.  The
        parameters ride in the launches by value, so a change starts a new graph generation; the momentum buffer keeps its contents
        (``begin`` / ``start_latent`` zero it)."""
        self._apg_vals = self._check_apg(Fn.apg_params(norm_threshold, eta_parallel, momentum), self._phi_vals)
        self._apply_apg()

    def clear_apg(self) -> None:
        """Back to the CFG combine (the buffers are kept for a later set_apg)."""
        self._apg_vals = None
        self._apply_apg()

    def _apply_apg(self) -> None:
        if self._apg_vals is None:
            self._apg, sig = None, None
        else:
            r, eta_p, beta = self._apg_vals
            if self._apg_stats is None:
                nb = L.lib().avd_apg_stats_bytes(self.embed.B, int(np.prod(self.latent_shape[1:])))
                if nb < 0:
                    raise ValueError(f"apg needs >= 2 latent elements per sample and B <= 65535 (latent {self.latent_shape})")
                self._apg_stats = torch.empty(nb, dtype=torch.uint8, device=self.device)
            if beta != 0.0 and self.apg_momentum is None:
                self.apg_momentum = torch.zeros(self.latent_shape, device=self.device, dtype=torch.float32)
            mom = self.apg_momentum if beta != 0.0 else None
            self._apg = L.ApgControl(r, eta_p, beta, L.ptr(mom), self._apg_stats.data_ptr(), self._apg_stats.numel())
            sig = (r, eta_p, beta, L.ptr(mom), self._apg_stats.data_ptr())
        if sig != self._apg_sig:
            self._generation += 1
            self._stale_reason = "adaptive projected guidance was switched on or off, or its parameters changed (set_apg / clear_apg)"
        self._apg_sig = sig

    def _zero_apg_momentum(self) -> None:
        """a trajectory starts without momentum"""
        if self.apg_momentum is not None:
            self.apg_momentum.zero_()

    # ---- window consensus: the batch as N consecutive windows of one latent canvas ----
    def set_window_consensus(self, hop: int, weights=None) -> None:
        """This batch is N consecutive windows of one canvas, ``hop`` latent positions apart: every step from now on ends with the
        consensus launch on its ``out`` (class docstring).  ``weights``: [L] per-position weights > 0, None = uniform.  Checked
        before anything changes.  The weights are copied into an engine-owned buffer, so new weights reach a captured graph;
        switching the consensus on, or changing ``hop`` (held by value), starts a new graph generation."""
        if self.eta > 0 and self.noise_keying != "canvas":
            raise ValueError("window consensus needs eta == 0 with the per-sample noise stream: the mean of the windows' independent "
                             "noise draws would shrink their variance (build the engine with noise_keying='canvas', canvas_hop=hop "
                             "to key the noise by canvas position)")
        if int(hop) != hop or int(hop) <= 0:
            raise ValueError(f"hop must be a positive whole number of latent positions, got {hop!r}")
        if self.eta > 0 and int(hop) != self.canvas_hop:
            raise ValueError(f"window consensus at eta > 0 needs hop == canvas_hop (the noise is keyed for windows {self.canvas_hop} "
                             f"positions apart), got hop {hop}")
        if self._guide is not None and self._guide_hop is not None and int(hop) != self._guide_hop:
            raise ValueError(f"window consensus under a canvas-keyed guide needs hop == the guide's hop {self._guide_hop}, got hop {hop}")
        L_ = Fn.window_dims(self.latent_shape)[1]
        w = Fn.consensus_weights(weights, L_)
        if self._cons_w is None:
            self._cons_w = torch.empty(L_, dtype=torch.float32, device=self.device)
        self._cons_w.copy_(w)
        self._touch_consensus(int(hop))

    def clear_window_consensus(self) -> None:
        """Back to independent samples (the weight buffer is kept for a later set_window_consensus)."""
        self._touch_consensus(None)

    def _touch_consensus(self, hop: Optional[int]) -> None:
        if hop != self._cons_hop:
            self._generation += 1
            self._stale_reason = "the window consensus was switched on or off, or its hop changed (set_window_consensus / " \
                                 "clear_window_consensus)"
        self._cons_hop = hop

    # ---- guidance interval ----
    def set_guidance_interval(self, interval) -> None:
        """None (every step is a CFG step) or (t_lo, t_hi), ends inclusive: which steps of the next ``run`` apply guidance.  Checked
        before anything changes.  The two kinds of step are separate launches and ``run`` picks between them on the host, so no
        captured graph goes stale."""
        self.guidance_interval = su.check_guidance_interval(interval)

    def start_latent(self, z_init: torch.Tensor, sched: torch.Tensor, strength: float = 1.0):
        """(z_start, sched_k): the start of a guided trajectory at ``strength`` (schedule_utils.truncate_schedule: k of the n steps
        of ``sched`` are run, from t_s = sched_k[0]).  k = n (strength 1): blend(mask, q(t_s), z_init) — the masked region starts on
        the known clip's forward path, the rest is the caller's noise.  k < n: q(t_s) everywhere (SDEdit: the unmasked region becomes
        a variation of the known clip); k = 0 returns the known latent itself.  Without a known latent only strength 1 is allowed and
        z_start is z_init.  Computed on the device with the guide's keying (avd_latent_guide_f32 / avd_latent_guide_canvas_f32)."""
        sched_k = su.truncate_schedule(sched, strength)
        n = torch.as_tensor(sched).numel() - 1
        self._zero_apg_momentum()
        z_init = L.dev_f32(z_init, "z_init")
        if tuple(z_init.shape) != self.latent_shape:
            raise ValueError(f"latent shape {tuple(z_init.shape)} != engine shape {self.latent_shape}")
        if self._guide is None:
            if sched_k.numel() - 1 != n:
                raise ValueError("strength < 1 starts from the known latent: call set_known() first")
            return z_init, sched_k
        B = self.embed.B
        tau = torch.full((B,), int(sched_k[0]), dtype=torch.long, device=self.device)
        z = z_init if sched_k.numel() - 1 == n else None
        return Fn.latent_guide_launch(self._guide, self._guide_hop, tau, self.alpha_bar, z, torch.empty_like(z_init)), sched_k

    def step(self, z: torch.Tensor, t_now: torch.Tensor, t_prev: torch.Tensor,
             noise: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None,
             t_last: Optional[torch.Tensor] = None, cond_only: bool = False) -> torch.Tensor:
        """One step t_now -> t_prev.  ``t_last`` (solver "dpmpp_2m" only): the timesteps the previous step started from, whose x0
        ``x0_hist`` holds; None (or entries < 0) takes a first-order step.  Either way x0_hist then holds this step's x0.
        ``cond_only``: take the single-branch step of a guidance interval (eps = eps_cond, no null branch) instead of the CFG step;
        the timesteps live on the device and are not read here, so the engine's ``guidance_interval`` does not enter: the caller
        says which kind it wants (``run`` does, from the host copy of the schedule)."""
        if self.Xp is None:
            raise RuntimeError("call set_prompt() first")
        self._clip_refusal("step", "a clip guide is keyed by the clip positions of step_slots' slots; a per-sample step is guided by set_known")
        self._clips_refusal("step")
        self._slot_cfg_refusal("step")
        z = L.dev_f32(z, "z")
        if tuple(z.shape) != self.latent_shape:
            raise ValueError(f"latent shape {tuple(z.shape)} != engine shape {self.latent_shape}")
        tn, tp = L.dev_i64(t_now, self.device), L.dev_i64(t_prev, self.device)
        if not torch.cuda.is_current_stream_capturing():
            self._sync_weights()
        out = torch.empty_like(z) if out is None else out
        self._last_cond_only = bool(cond_only)
        out = self._step_kind(z, tn, tp, noise, out, t_last, cond_only)
        if self._cons_hop is not None:
            outer, L_, inner = Fn.window_dims(self.latent_shape)
            L.check(L.lib().avd_window_consensus_f32(out.data_ptr(), self._cons_w.data_ptr(), self.latent_shape[0], outer, L_,
                                                     self._cons_hop, inner, L.stream_ptr(self.device)))
        return out

    def _step_args(self, z, out, noise, t_last, guided):
        """(t_last, x0_hist, noise) as the step entries take them.  ``guided``: the step ends in the latent guide's blend or the CFG
        control, which draw eta > 0 noise from noise_seed only."""
        if noise is not None:
            if self._key is not None:
                raise ValueError("this engine draws its noise from noise_seed: do not pass `noise` as well")
            if guided:
                raise ValueError("a guided or CFG-controlled step draws its noise from noise_seed: it takes no `noise`")
            if self.solver == "dpmpp_2m":
                raise ValueError("solver 'dpmpp_2m' takes no noise: it is deterministic at eta == 0 and draws from noise_seed at eta > 0")
        if guided and self.eta > 0 and self._key is None:
            raise ValueError("with a known latent or a CFG control, eta > 0 needs noise_seed (unseeded noise is not supported there)")
        tl = h = None
        if self.solver == "dpmpp_2m":
            h = self.x0_hist
            for name, t in (("z", z), ("out", out)):
                if t.untyped_storage().data_ptr() == h.untyped_storage().data_ptr():
                    raise L.AvdError(f"{name} must not alias the engine's x0_hist (the solver history)")
            tl = self._no_hist if t_last is None else L.dev_i64(t_last, self.device)
        elif t_last is not None:
            raise ValueError("t_last is the multistep solver's history: this engine runs solver 'ddim'")
        if self.eta == 0:
            noise = None
        elif self._key is None and noise is None:
            noise = torch.randn_like(z)
        return tl, h, noise

    def _step_kind(self, z, tn, tp, noise, out, t_last, cond_only) -> torch.Tensor:
        """the step proper: under a canvas-keyed latent guide one entry for every kind of step of either solver; else the SDE form
        of DPM-Solver++(2M) (one entry for every kind of eta > 0 step of that solver), canvas-keyed
        (one entry for every kind of eta > 0 DDIM step of a canvas-keyed engine), cond-only (one entry for every solver state, with
        or without a latent guide; the CFG control does not apply there), CFG-controlled, guided, DPM-Solver++(2M), seeded or plain
        DDIM"""
        apg = None if self._apg is None or cond_only else C.byref(self._apg)      # as the CFG control: not on a cond-only step
        guided = self._guide is not None or ((self._ctl is not None or apg is not None) and not cond_only)
        tl, h, noise = self._step_args(z, out, noise, t_last, guided)
        lib, desc = L.lib(), C.byref(self.desc)
        key = None if self._key is None else C.byref(self._key)
        guide = None if self._guide is None else C.byref(self._guide)
        zx, ts = (z.data_ptr(), self.Xp.data_ptr()), (tn.data_ptr(), tp.data_ptr())
        tail = (out.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), L.stream_ptr(self.device))
        ctl = None if self._ctl is None or cond_only else C.byref(self._ctl)      # the CFG control does not apply to a cond-only step
        cond = 1 if cond_only else 0
        if apg is not None:      # one entry for every solver state and keying of the APG step
            hop = (self.canvas_hop or 0) if self.eta > 0 else 0
            rc = lib.avd_denoise_step_apg_f32(desc, apg, ctl, guide, key if self.eta > 0 else None, hop,
                                              (self._guide_hop or 0) if guide is not None else 0, L.ptr(tl), L.ptr(h), *zx, *ts, *tail)
        elif guide is not None and self._guide_hop is not None:
            rc = lib.avd_denoise_step_canvas_guided_f32(desc, guide, self._guide_hop, key if self.eta > 0 else None, ctl, cond,
                                                        L.ptr(tl), L.ptr(h), *zx, *ts, *tail)
        elif self.solver == "dpmpp_2m" and self.eta > 0:
            rc = lib.avd_denoise_step_dpmpp_2m_sde_f32(desc, key, self.canvas_hop or 0, ctl, guide, cond, tl.data_ptr(), h.data_ptr(),
                                                       *zx, *ts, *tail)
        elif self.canvas_hop is not None and self.eta > 0:
            rc = lib.avd_denoise_step_canvas_f32(desc, key, self.canvas_hop, ctl, guide, cond, *zx, *ts, *tail)
        elif cond_only:
            rc = lib.avd_denoise_step_cond_f32(desc, guide, key, L.ptr(tl), L.ptr(h), *zx, *ts, L.ptr(noise), *tail)
        elif ctl is not None:
            rc = lib.avd_denoise_step_cfg_f32(desc, ctl, guide, key, L.ptr(tl), L.ptr(h), *zx, *ts, *tail)
        elif guided:
            rc = lib.avd_denoise_step_guided_f32(desc, guide, key, L.ptr(tl), L.ptr(h), *zx, *ts, *tail)
        elif h is not None:
            rc = lib.avd_denoise_step_dpmpp_2m_f32(desc, *zx, tl.data_ptr(), *ts, h.data_ptr(), *tail)
        elif key is not None:
            rc = lib.avd_denoise_step_seeded_f32(desc, key, *zx, *ts, *tail)
        else:
            rc = lib.avd_denoise_step_f32(desc, *zx, *ts, L.ptr(noise), *tail)
        L.check(rc)
        return out

    # ---- slot timesteps: one (t_now, t_prev) pair per position of the sliding axis ----
    @property
    def slot_len(self) -> int:
        """latent positions of one slot along the sliding axis: the tube's t (video target) or the chunk length (audio target)"""
        return self.tube[0] if self.target == "video" else self.chunk[0]

    @property
    def slots(self) -> int:
        """S, the slots of one sample (include/avdiff_hip.h, "slot timesteps"): T // tube t (video) or the Na chunks (audio)"""
        return self.latent_shape[2] // self.tube[0] if self.target == "video" else self.embed.Nt

    def step_slots(self, z: torch.Tensor, t_now: torch.Tensor, t_prev: torch.Tensor, out: Optional[torch.Tensor] = None,
                   t_last: Optional[torch.Tensor] = None, clip_first: Optional[int] = None, clip_stride: Optional[int] = None,
                   clip_cursor: Optional[torch.Tensor] = None, clip_queues: Optional[int] = None, clip_seeds=None) -> torch.Tensor:
        """One CFG step on slot timesteps (extension; include/avdiff_hip.h, "slot timesteps"; avd_denoise_step_slots_f32):
        ``t_now`` / ``t_prev`` are int [B, S] tables, S = ``slots``, one pair per slot of ``slot_len`` latent positions along the
        sliding axis.  Every slot's tokens embed its t_now and its latent takes the DDIM update of its pair; a slot with t_prev ==
        t_now is held (``out`` equals ``z`` there bit for bit) while its tokens still take part in attention.  A table that repeats
        one pair per sample gives ``step``'s bits.  The primitive of FIFO diagonal denoising (stream_infer.fifo_denoise) and of
        continuing from held clean context.
        Solver "dpmpp_2m" (avd_denoise_step_slots_dpmpp_2m_f32) needs ``t_last``, a third int [B, S] table: the timestep each slot's
        previous step started from, < 0 for a first-order step.  A slot's history is the elements of ``x0_hist`` under it: read by its
        second-order steps, overwritten with its x0, and neither read nor written while the slot is held.
        On an eta > 0 engine ``clip_first`` selects the stochastic step (avd_denoise_step_slots_seeded_f32; include/avdiff_hip.h,
        "clip-keyed slot noise"): an int, the clip slot that slot 0 of sample 0 holds (negative slots wrap).  Every stepping slot then
        draws its noise term — DDIM's sigma(eta), or the SDE form of "dpmpp_2m" — by the clip position it holds, keyed by the engine's
        ``noise_seed`` (required): sample k holds clip slots clip_first + k * ``clip_stride`` .. (``clip_stride`` None = S), and
        ``clip_cursor`` (one int32 in device memory, or None) is read at every launch and added, clamped at 0, to ``clip_first``, so a
        captured step follows a moving queue.  A held slot draws nothing.  Without ``clip_first`` an eta > 0 engine is refused, and
        on an eta == 0 engine the three arguments change nothing: the same launches, the same bits.
        Under ``set_clip_guide`` (avd_denoise_step_slots_guided_f32; "clip-keyed latent guide") ``clip_first`` is required at any eta:
        every stepping slot ends in the blend with the known clip canvas at the clip positions it holds, forward-noised to the slot's
        own t_prev; a held slot stays ``z`` and ``x0_hist`` keeps the model's x0.
        Under ``set_slot_cfg`` (avd_denoise_step_slots_cfg_f32; "slot CFG control") every stepping slot's eps is combined with the
        guidance of its own noise level and rescaled, or projected (APG), with statistics over the slot's own elements, before the
        solver update; any solver, any eta, with or without the clip guide.
        ``clip_queues`` = K (avd_denoise_step_slots_clips_f32; "clip batch keying") steps a FIFO clip batch: the batch is K queues of
        B / K samples, the walk ``clip_first + k * clip_stride`` restarts in every queue, and at eta > 0 queue k draws its step noise
        under ``clip_seeds[k]`` — K ints, or the int64 device tensor ``functional.queue_seeds`` makes of them — which stand in for the
        engine's ``noise_seed`` (not read, and not required); an eta > 0 engine without ``clip_seeds`` is refused.  Under
        ``set_clip_guides`` (which requires ``clip_queues``, with its K) queue k is guided by its own canvas, mask and seed.  The bits
        are those of K separate calls on the K slices; ``set_clip_guide``'s one canvas is refused here, and ``clip_seeds`` without
        ``clip_queues`` is.
        Scope: the scalar guidance or a slot CFG control; a per-sample latent guide (``set_known``), a per-sample CFG control, a window
        consensus, temb_mode "add" and overlapping audio chunks are refused before anything is launched, as is ``t_last`` on a "ddim"
        engine; no unseeded or explicit noise."""
        if self.Xp is None:
            raise RuntimeError("call set_prompt() first")
        if clip_queues is None:
            if clip_seeds is not None:
                raise ValueError("clip_seeds are the step seeds of a clip batch's queues: they need clip_queues")
            if self._clips is not None:
                raise ValueError("step_slots under set_clip_guides needs clip_queues: the K canvases guide the K queues of a clip batch")
        else:
            if isinstance(clip_queues, bool) or not isinstance(clip_queues, int) or clip_queues < 1 or self.embed.B % clip_queues:
                raise ValueError(f"clip_queues {clip_queues!r} must be an int >= 1 that divides the batch {self.embed.B}")
            self._clip_refusal("step_slots(clip_queues=)", "a clip guide is one canvas walked by one queue, and a clip batch holds several: "
                               "set_clip_guides")
            if self._clips is not None and self._clips[0].shape[0] != clip_queues:
                raise ValueError(f"clip_queues {clip_queues} against the {self._clips[0].shape[0]} canvases of set_clip_guides")
            if self.eta > 0 and clip_seeds is None:
                raise ValueError("step_slots(clip_queues=K) at eta > 0 draws every queue's step noise under its own seed: pass clip_seeds, "
                                 "one per queue")
        self._slot_refusals(t_last is not None, clip_first, seeded=clip_seeds is not None, guided=self._clips is not None)
        S = self.slots
        key = guide = None
        if self.eta > 0:      # _slot_refusals has asked for clip_first and noise_seed (a clip batch: the queues' seeds stand in for it)
            key = Fn.slot_key(0 if clip_queues is not None else self.noise_seed, clip_first, S if clip_stride is None else clip_stride,
                              clip_cursor, self.device)
        if self._clips is not None:      # canvas 0 carries the checks and the addresses; the queues' seeds ride in the descriptor
            guide = Fn.clip_guide(self._clips[0][0], None if self._clips[1] is None else self._clips[1][0], 0, clip_first,
                                  S if clip_stride is None else clip_stride, clip_cursor, self.latent_shape)
        if self._clip is not None:      # _slot_refusals has asked for clip_first; the guide shares the key's geometry
            guide = Fn.clip_guide(self._clip[0], self._clip[1], self._clip[2], clip_first, S if clip_stride is None else clip_stride,
                                  clip_cursor, self.latent_shape)
        z = L.dev_f32(z, "z")
        if tuple(z.shape) != self.latent_shape:
            raise ValueError(f"latent shape {tuple(z.shape)} != engine shape {self.latent_shape}")
        tn, tp, *tl = Fn.slot_tables(t_now, t_prev, self.embed.B, S, self.device, t_last)
        if out is None:
            out = torch.empty_like(z)
        elif not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and out.shape == z.shape and out.device == z.device):
            raise ValueError(f"out must be a contiguous float32 tensor of shape {tuple(z.shape)} on z's device")
        if tl:
            for name, t in (("z", z), ("out", out)):
                if t.untyped_storage().data_ptr() == self.x0_hist.untyped_storage().data_ptr():
                    raise L.AvdError(f"{name} must not alias the engine's x0_hist (the solver history)")
        if not torch.cuda.is_current_stream_capturing():
            self._sync_weights()
        self._last_cond_only = False
        head = (C.byref(self.desc), z.data_ptr(), self.Xp.data_ptr())
        tail = (out.data_ptr(), self.workspace.data_ptr(), self.workspace.numel(), L.stream_ptr(self.device))
        if clip_queues is not None:      # a clip batch: any solver, any eta, with or without the control and the guides
            seeds = Fn.queue_seeds(clip_seeds, clip_queues, self.device) if key is not None else None
            cq = Fn.clip_queues(clip_queues, self.embed.B, seeds, None if guide is None else self._clips[2])
            L.check(L.lib().avd_denoise_step_slots_clips_f32(head[0], None if self._scfg is None else C.byref(self._scfg),
                                                             None if key is None else C.byref(key),
                                                             None if guide is None else C.byref(guide), C.byref(cq),
                                                             tl[0].data_ptr() if tl else None, self.x0_hist.data_ptr() if tl else None,
                                                             *head[1:], tn.data_ptr(), tp.data_ptr(), S, *tail))
        elif self._scfg is not None:      # any solver, any eta, with or without the clip guide
            L.check(L.lib().avd_denoise_step_slots_cfg_f32(head[0], C.byref(self._scfg), None if key is None else C.byref(key),
                                                           None if guide is None else C.byref(guide),
                                                           tl[0].data_ptr() if tl else None, self.x0_hist.data_ptr() if tl else None,
                                                           *head[1:], tn.data_ptr(), tp.data_ptr(), S, *tail))
        elif guide is not None:
            L.check(L.lib().avd_denoise_step_slots_guided_f32(head[0], None if key is None else C.byref(key), C.byref(guide),
                                                              tl[0].data_ptr() if tl else None, self.x0_hist.data_ptr() if tl else None,
                                                              *head[1:], tn.data_ptr(), tp.data_ptr(), S, *tail))
        elif key is not None:
            L.check(L.lib().avd_denoise_step_slots_seeded_f32(head[0], C.byref(key), tl[0].data_ptr() if tl else None,
                                                              self.x0_hist.data_ptr() if tl else None, *head[1:], tn.data_ptr(),
                                                              tp.data_ptr(), S, *tail))
        elif tl:
            L.check(L.lib().avd_denoise_step_slots_dpmpp_2m_f32(*head, tl[0].data_ptr(), tn.data_ptr(), tp.data_ptr(), S,
                                                                self.x0_hist.data_ptr(), *tail))
        else:
            L.check(L.lib().avd_denoise_step_slots_f32(*head, tn.data_ptr(), tp.data_ptr(), S, *tail))
        return out

    def _slot_refusals(self, has_t_last: bool, clip_first: Optional[int] = None, seeded: bool = False, guided: bool = False) -> None:
        """what ``step_slots`` refuses of the engine's state, before anything is launched (``fifo_open`` asks the same before it
        allocates, so a graph-replayed queue refuses what the eager one does, in the same words, before any capture).
        ``clip_first``: as ``step_slots`` takes it; an eta > 0 engine steps only with it and a ``noise_seed``.  ``seeded``: the step of
        a clip batch, whose queues' ``clip_seeds`` stand in for the ``noise_seed``; ``guided``: it runs under ``set_clip_guides``"""
        if (self._clip is not None or guided) and clip_first is None:
            raise ValueError("step_slots under a clip guide needs clip_first, at any eta: the guide reads the clip canvas at the clip "
                             "positions the slots hold")
        if self.eta > 0 and clip_first is None:
            raise ValueError("step_slots needs eta == 0, or clip_first on an engine with noise_seed: slots at different timesteps draw "
                             "their eta > 0 noise by the clip position they hold (unkeyed noise is out of scope)")
        if self.eta > 0 and self.noise_seed is None and not seeded:
            raise ValueError("step_slots(clip_first=...) at eta > 0 draws its noise from the engine's noise_seed: build the engine with "
                             "one (unseeded and explicit noise are not supported there)")
        if self.solver == "ddim" and has_t_last:
            raise ValueError("t_last is the multistep solver's history: this engine runs solver 'ddim'")
        if self.solver != "ddim" and not has_t_last:
            raise ValueError(f"step_slots on solver {self.solver!r} needs t_last, the [B, S] table of the timesteps each slot's history "
                             "comes from (-1: none)")
        if self._guide is not None:
            raise ValueError("step_slots takes no latent guide (its forward path is keyed by one t_prev per sample): clear_known() first")
        if self._ctl is not None:
            raise ValueError("step_slots takes the scalar guidance: per-sample guidance and guidance rescale (the CFG control) are not "
                             "supported there")
        if self._apg is not None:
            raise ValueError("step_slots takes the plain CFG combine: adaptive projected guidance (a CFG control) is not supported "
                             "there: clear_apg() first")
        if self._cons_hop is not None:
            raise ValueError("step_slots takes no window consensus (the windows of a canvas share their timesteps): "
                             "clear_window_consensus() first")
        if self.temb_mode == "add":
            raise ValueError("step_slots needs temb_mode='concat': the added embedding is one row per sample")
        if self.target == "audio" and self.chunk[0] != self.chunk[1]:
            raise ValueError(f"step_slots needs non-overlapping audio chunks (stride == length), got chunk {self.chunk}")

    def fifo_shift(self, z: torch.Tensor, c: int, t: int, seed: Optional[int] = None, guided: Optional[str] = None):
        """The queue step of FIFO diagonal denoising on this engine's queue (``functional.fifo_shift`` with the engine's ``slot_len``;
        ``seed``: the seed of the entering slot's noise, None = the engine's ``noise_seed``): returns (z_out, popped).  Solver "dpmpp_2m": the same launch shifts the history into a
        second engine-owned buffer, which becomes ``x0_hist`` (the head's history is dropped, the entering slot's is zero): a slot
        keeps its history as it moves up the queue.  That changes an address a captured graph holds, so it starts a new graph
        generation.  Under ``set_slot_cfg(apg_momentum=)`` one more launch (``functional.fifo_carry``) carries the slot momentum into
        the engine's other momentum buffer in the same way, on either solver, and the two swap.
        ``guided`` (None = the plain shift, also under a clip guide): "mask" or "everywhere" needs ``set_clip_guide`` and puts the
        entering slot, clip slot ``c``, on the guide's forward path at ``t`` inside the same launch (avd_fifo_shift_guided_f32) —
        through the guide's mask, or with the mask read as 1 on every in-canvas position (SDEdit's start)."""
        seed = self.noise_seed if seed is None else seed
        if seed is None:
            raise ValueError("fifo_shift draws the entering slot's noise from a seed: pass one, or build the engine with noise_seed")
        guide = None
        if guided is not None:
            if guided not in ("mask", "everywhere"):
                raise ValueError(f"guided must be None, 'mask' or 'everywhere', got {guided!r}")
            if self._clip is None:
                raise ValueError("fifo_shift(guided=...) guides the entering slot by the clip guide: set_clip_guide() first")
            guide = dict(known=self._clip[0], mask=self._clip[1], seed=self._clip[2], alpha_bar=self.alpha_bar,
                         everywhere=guided == "everywhere")
        if self.solver != "dpmpp_2m":
            out = Fn.fifo_shift(z, c, seed, t, self.slot_len, guide=guide)
            self._carry_slot_momentum(0, 1)      # a slot momentum follows its slot: a launch of its own behind the move
            return out
        z_out, popped, _ = self._move_hist("fifo_shift", lambda h, h_out: Fn.fifo_shift(z, c, seed, t, self.slot_len, hist=h, hist_out=h_out,
                                                                                        guide=guide))
        self._carry_slot_momentum(0, 1)
        return z_out, popped

    def fifo_shift_clips(self, z: torch.Tensor, queues: int, c: int, t: int, seeds, clips: torch.Tensor, m: int) -> torch.Tensor:
        """The multi-queue form of ``fifo_shift`` (``functional.fifo_shift_clips`` with the engine's ``slot_len``; include/avdiff_hip.h,
        "FIFO clip batch"): the batch is ``queues`` independent queues in lockstep, queue k under ``seeds[k]``; every queue shifts, its
        head goes into slot ``m`` of ``clips[k]`` and noise of clip slot ``c`` at ``t`` enters its tail.  Returns z_out.  Solver
        "dpmpp_2m": the same launch moves ``x0_hist`` into the engine's second buffer and the two swap, which starts a new graph
        generation, exactly as ``fifo_shift`` does.  Under ``set_slot_cfg(apg_momentum=)`` the same launch carries the slot momentum into
        the other momentum buffer too: no ``functional.fifo_carry`` launch.  A clip guide refuses the call."""
        self._clip_refusal("fifo_shift_clips", "a clip guide is one canvas walked by one queue, and a clip batch holds several")
        multistep, mom = self.solver == "dpmpp_2m", self._smom_beta != 0.0

        def move(h, h_out):
            return Fn.fifo_shift_clips(z, queues, c, seeds, t, self.slot_len, clips, m, hist=h, hist_out=h_out,
                                       carry=self._smom if mom else None, carry_out=self._smom_other if mom else None)

        out = self._move_hist("fifo_shift_clips", move) if multistep else move(None, None)
        if mom:
            self._swap_slot_momentum()
        return out[0] if isinstance(out, tuple) else out

    def fifo_lookahead(self, z: torch.Tensor, ctx: int, shift: int, c: Optional[int] = None, t: Optional[int] = None,
                       seed: Optional[int] = None):
        """The queue step of FIFO lookahead denoising on this engine's queue (``functional.fifo_lookahead`` with the engine's
        ``slot_len``; include/avdiff_hip.h, "FIFO lookahead"): returns (z_out, popped), popped None at ``shift=0`` (the refresh of the
        duplicates, which takes no ``c`` / ``t`` / ``seed``).  At ``shift=1`` ``seed`` None is the engine's ``noise_seed``.  Solver
        "dpmpp_2m": as in ``fifo_shift`` the same launch moves the history into the engine's second buffer, which becomes ``x0_hist``,
        and a new graph generation starts — at either ``shift``, the launch being out of place.  A slot momentum
        (``set_slot_cfg(apg_momentum=)``) follows the history's map in a ``functional.fifo_carry`` launch behind it, at either ``shift``."""
        self._clip_refusal("fifo_lookahead", "the duplicated slots of overlapping windows are refreshed from their owner copies, and the guide's "
                           "tail pass has no lookahead form yet")
        self._clips_refusal("fifo_lookahead")
        if shift == 1:
            seed = self.noise_seed if seed is None else seed
            if seed is None:
                raise ValueError("fifo_lookahead draws the entering slot's noise from a seed: pass one, or build the engine with noise_seed")
        if self.solver != "dpmpp_2m":
            out = Fn.fifo_lookahead(z, ctx, shift, self.slot_len, c=c, seed=seed, t=t)
            self._carry_slot_momentum(ctx, shift)
            return out
        z_out, popped, _ = self._move_hist("fifo_lookahead", lambda h, h_out: Fn.fifo_lookahead(z, ctx, shift, self.slot_len, c=c, seed=seed,
                                                                                                t=t, hist=h, hist_out=h_out))
        self._carry_slot_momentum(ctx, shift)
        return z_out, popped

    # ---- FIFO queue with device cursors: an iteration as a fixed chain of launches (include/avdiff_hip.h, "FIFO device cursors") ----
    def fifo_open(self, prompt_canvas: torch.Tensor, prompt_hop: int, prompt_len: int, sched, n_slots: int,
                  noise_seed: int, prompt_den: int = 1, prompt_interp: Optional[str] = None) -> "FifoQueue":
        """Open a FIFO queue (``stream_infer.fifo_denoise(graph=True)`` drives it) whose iterations read the ramp row r and the steady
        iteration m off two int32 device cursors, so that ``fifo_ramp`` and ``fifo_steady`` are fixed chains of launches on the
        current stream, the same eagerly and under ``fifo_capture``.  Uploads the plan's tables (``schedule_utils.fifo_plan``, with
        ``fifo_plan_last`` on solver "dpmpp_2m"; the ramp rows stacked [n - 1, B*S]) and the prompt canvas; allocates the cursors (both
        0), the [B, S] table buffers, the prompt-latent buffer, the two latent buffers (``q.z`` holds the seeded start), a clip canvas
        of ``n_slots`` slots (fresh per call: it is what the driver returns) and, on "dpmpp_2m", the second history buffer; embeds the
        prompt of m = 0, which also writes Xp's constant timestep columns.  ``prompt_len``: the prompt latent's length along its
        sliding axis (``stream_infer.fifo_prompt_len``).  Refuses what ``step_slots`` refuses, before it allocates.
        On an eta > 0 engine with a ``noise_seed`` the queue is stochastic: its steps pass ``clip_first=0, clip_cursor=q.m`` (m is 0
        through the ramp), the step noise keyed by ``engine.noise_seed``; ``noise_seed`` here seeds the start and the entering noise.
        The queue holds ``noise_seed``, c0 = n, ``n_slots``, the hops and every address: a captured pair is good for this queue only.
        ``prompt_den`` > 1 with a ``prompt_interp`` (include/avdiff_hip.h, "fractional prompt hop") makes the hop ``prompt_hop /
        prompt_den``: the prompt of m = 0 and ``fifo_steady``'s come from ``functional.fifo_prompt_gather_frac`` off the same cursor
        (first = 0, stride = S).  ``prompt_den`` == 1 is the integer gather, launch for launch."""
        self._clip_refusal("fifo_open", "the replayed queue's chain of launches has no guided tail pass: the guided queue runs eagerly")
        self._clips_refusal("fifo_open")
        B, S, sl = self.embed.B, self.slots, self.slot_len
        ramp_now, ramp_prev, steady_now, steady_prev = su.fifo_plan(sched, S)
        n = ramp_now.shape[0] + 1
        if n != B * S:
            raise ValueError(f"the schedule has {n} steps, the engine's queue {B} samples x {S} slots = {B * S}: fifo_denoise needs them equal")
        outer, L_, _ = Fn.window_dims(self.latent_shape)
        if L_ != S * sl:
            raise ValueError(f"the engine's sliding length {L_} is not {S} slots of {sl} positions (an uncovered audio tail cannot queue)")
        Fn.noise_key(noise_seed, 0)
        for name, v in (("n_slots", n_slots), ("prompt_hop", prompt_hop), ("prompt_len", prompt_len)):
            if isinstance(v, bool) or not isinstance(v, int) or v < 1:
                raise ValueError(f"{name} must be an int >= 1, got {v!r}")
        Fn.check_prompt_frac(prompt_hop, prompt_den, prompt_interp)
        stochastic = self.eta > 0 and self.noise_seed is not None
        self._slot_refusals(self.solver == "dpmpp_2m", 0 if stochastic else None)
        dev = self.device
        q = FifoQueue()
        q.clip_first = 0 if stochastic else None      # eta > 0: the steps key their noise by clip slot, read off the cursor m
        q.n, q.n_slots, q.seed, q.hop, q.s0 = n, n_slots, noise_seed, prompt_hop, int(torch.as_tensor(sched).reshape(-1)[0])
        q.frac = (prompt_den, prompt_interp) if prompt_den > 1 else None      # None: the integer gather
        if (n + n_slots) * sl > 2 ** 32:
            raise ValueError(f"(n {n} + n_slots {n_slots}) * slot_len {sl} exceeds the stream's 2**32 canvas positions")
        q.canvas_p = L.dev_f32(prompt_canvas.to(dev), "prompt canvas")
        multistep = self.solver == "dpmpp_2m"
        ramp = [ramp_now, ramp_prev]
        steady = [steady_now, steady_prev]
        if multistep:
            ramp_last, steady_last = su.fifo_plan_last(sched, S)
            ramp.append(ramp_last)
            steady.append(steady_last)
        q.ramp = [Fn.stack_slot_tables(t).to(dev) for t in ramp] if n > 1 else []
        q.steady = [L.dev_i64(t, dev) for t in steady]
        q.slot = [torch.empty(B, S, dtype=torch.long, device=dev) for _ in ramp]
        q.r = torch.zeros(1, dtype=torch.int32, device=dev)
        q.m = torch.zeros(1, dtype=torch.int32, device=dev)
        q.clip = torch.empty((outer, n_slots * sl) + tuple(self.latent_shape[3:]), device=dev, dtype=torch.float32)
        q.z = Fn.canvas_noise(noise_seed, torch.full((B,), q.s0, dtype=torch.long, device=dev), self.latent_shape, L_)
        q.other = torch.empty_like(q.z)
        if multistep and self._hist_other is None:
            self._hist_other = torch.empty_like(self.x0_hist)
        q.prompt = self._fifo_gather(q, torch.empty((B, q.canvas_p.shape[0], prompt_len) + tuple(q.canvas_p.shape[2:]), device=dev,
                                                    dtype=torch.float32))
        self.set_prompt(q.prompt)
        return q

    def _fifo_gather(self, q: "FifoQueue", out: torch.Tensor) -> torch.Tensor:
        """the prompt batch of the open queue's iteration *m into ``out``: one launch, the integer gather or the fractional one"""
        B, S = self.embed.B, self.slots
        if q.frac is None:
            return Fn.fifo_prompt_gather(q.canvas_p, q.m, B, S, q.hop, out.shape[2], out=out)
        return Fn.fifo_prompt_gather_frac(q.canvas_p, q.m, B, 0, S, q.hop, q.frac[0], q.frac[1], out.shape[2], out=out)

    def fifo_ramp(self, q: "FifoQueue", src: torch.Tensor, dst: torch.Tensor) -> None:
        """One ramp iteration of an open queue: select row *r of the ramp tables -> ``step_slots`` src -> dst (on a stochastic queue
        keyed by the clip slots the queue holds at m = 0) -> r += 1."""
        Fn.slot_tables_select(q.ramp, q.r, q.slot)
        self.step_slots(src, q.slot[0], q.slot[1], out=dst, t_last=q.slot[2] if len(q.slot) == 3 else None, clip_first=q.clip_first,
                        clip_cursor=q.m)
        Fn.cursor_add(q.r)

    def fifo_steady(self, q: "FifoQueue", z: torch.Tensor, tmp: torch.Tensor) -> None:
        """One steady iteration of an open queue, with m = *m: gather the prompt of iteration m -> embed it into Xp (same address) ->
        ``step_slots`` z -> tmp on the constant steady tables -> shift tmp -> z, the finished head into slot m of the clip canvas and
        clip slot n + m entering at the tail -> m += 1.  The latent is back in ``z``.  On a stochastic queue the step draws its noise
        for clip slots m .., read off the same cursor.  On "dpmpp_2m" the shift carries the history
        into the engine's other history buffer and the two swap, as in ``fifo_shift``: two iterations put ``x0_hist`` back.  A slot
        momentum is carried by one more launch behind the shift and its two buffers swap likewise (``fifo_ramp`` moves nothing)."""
        B, S = self.embed.B, self.slots
        self._fifo_gather(q, q.prompt)
        self._prompt_rows(self._prompt_tokens(q.prompt), self.Xp, temb=False)
        multistep = len(q.steady) == 3
        self.step_slots(z, q.steady[0], q.steady[1], out=tmp, t_last=q.steady[2] if multistep else None, clip_first=q.clip_first,
                        clip_cursor=q.m)
        if not multistep:
            Fn.fifo_shift_cursor(tmp, q.n, q.m, q.clip, q.seed, q.s0, self.slot_len, out=z)
        else:
            self._move_hist("fifo_steady", lambda h, h_out: Fn.fifo_shift_cursor(tmp, q.n, q.m, q.clip, q.seed, q.s0, self.slot_len, out=z,
                                                                                 hist=h, hist_out=h_out),
                            bump=not torch.cuda.is_current_stream_capturing())      # a captured pair swaps twice: the address is back
        self._carry_slot_momentum(0, 1)      # the carry's map reads no cursor: the same launch eagerly and in a captured pair, whose two
        Fn.cursor_add(q.m)                   # iterations put the live buffer back at its address, as the histories

    def fifo_capture(self, q: "FifoQueue", steady: bool, za: torch.Tensor, zb: torch.Tensor) -> "torch.cuda.CUDAGraph":
        """Two iterations of one phase of an open queue in one HIP graph, one chain on one stream: ramp za -> zb -> za, steady twice
        on (za, zb).  After a replay the latent is back in ``za`` and ``x0_hist`` at its address; the cursors have moved by two.  Every
        kernel of the phase must have run once before (the driver takes each phase's first iteration eagerly).  The graph is this
        queue's: it holds the seed, c0, the clip length, the hops and every address by value."""
        self._sync_weights()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            if steady:
                self.fifo_steady(q, za, zb)
                self.fifo_steady(q, za, zb)
            else:
                self.fifo_ramp(q, za, zb)
                self.fifo_ramp(q, zb, za)
        return g

    def eps_tokens(self) -> torch.Tensor:
        """ε̂ tokens left in the workspace by the last step (debug / parity only): cond / null [2B,Nt,D] after a CFG step; after a
        cond-only step the conditional prediction alone, [B,Nt,D] — that step computes no null rows, and whatever an earlier CFG
        step left behind them is not handed out.  Under ``run`` the last step is the schedule's last."""
        e = self.embed
        D = self.head.output_dims[self.target]
        n = 2 * e.B * e.Nt * D
        tail = self.workspace[self.workspace.numel() - ((n * 4 + 255) // 256) * 256:]
        if self._last_cond_only:
            return tail[: n * 2].view(torch.float32).view(e.B, e.Nt, D).clone()
        return tail[: n * 4].view(torch.float32).view(2 * e.B, e.Nt, D).clone()

    # ---- whole trajectory -------------------------------------------------------------------------------
    def begin(self, sched: torch.Tensor) -> None:
        """Upload a sampling schedule and put the device-side cursor at its start (no per-step H2D afterwards)."""
        dev, B = self.device, self.embed.B
        self._sched = sched.to(dev, torch.long).contiguous()
        self._cursor = torch.zeros(1, dtype=torch.int32, device=dev)
        self._tn = torch.empty(B, dtype=torch.long, device=dev)
        self._tp = torch.empty(B, dtype=torch.long, device=dev)
        self._tl = torch.empty(B, dtype=torch.long, device=dev)
        self._zero_apg_momentum()

    def rewind(self) -> None:
        """the cursor back to the schedule's start; an APG momentum buffer is carried as it is (``begin`` zeroes it)"""
        self._cursor.zero_()

    def advance(self, src: torch.Tensor, dst: torch.Tensor, cond_only: bool = False) -> None:
        """dst = one step from src at the cursor's (t_now, t_prev); the cursor moves on, all on the stream.  Solver "dpmpp_2m" also
        reads t_last off the cursor (-1 at the start of the schedule: every trajectory begins first order).  ``cond_only``: as
        ``step`` — the cursor's timesteps stay on the device, the caller names the kind of step."""
        multistep = self.solver == "dpmpp_2m"
        self._advance_cursor(multistep)
        self.step(src, self._tn, self._tp, out=dst, t_last=self._tl if multistep else None, cond_only=cond_only)

    def _advance_cursor(self, multistep: bool) -> None:
        """the cursor's pair into (_tn, _tp), with ``multistep`` the entry before it into _tl as well; the cursor moves on"""
        cursor = (self._sched.data_ptr(), self._sched.numel(), self._cursor.data_ptr())
        tail = (self._tn.data_ptr(), self._tp.data_ptr(), self.embed.B, L.stream_ptr(self.device))
        if multistep:
            L.check(L.lib().avd_sched_advance_ms(*cursor, self._tl.data_ptr(), *tail))
        else:
            L.check(L.lib().avd_sched_advance(*cursor, *tail))

    def capture_pair(self, za: torch.Tensor, zb: torch.Tensor, cond_only: bool = False) -> "_CapturedPair":
        """Capture two steps (za -> zb -> za) of one kind into one HIP graph; replaying it advances the trajectory by two."""
        if self.eta > 0 and self._key is None:
            raise NotImplementedError("graph replay with eta > 0 would replay the same noise (build the engine with noise_seed)")
        self._sync_weights()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self.advance(za, zb, cond_only)
            self.advance(zb, za, cond_only)
        return _CapturedPair(self, g)

    GRAPH_BELOW_ROWS = 6144      # 2B*N under which a step's ~60-95 launches are host-bound: replay them from a HIP graph

    def check_schedule(self, sched: torch.Tensor) -> None:
        """what ``run`` asks of a schedule before it steps (a caller that drives ``begin`` / ``advance`` itself asks the same).
        Solver "dpmpp_2m": strictly decreasing runs, joined at most by the up-jumps of a resampling schedule — a jump returns to a
        timestep the schedule has already passed (schedule_utils.resample_schedule emits nothing else; a climb to a new timestep is
        refused as a mis-ordered schedule, as before).  Any resampling schedule (schedule_utils.has_jumps: an up-jump back to a
        timestep already passed): ``noise_seed`` (the renoise key, also at eta == 0), no equal neighbours, and under a window
        consensus a renoise keyed by canvas position at the consensus hop.  Solver "ddim" takes any other schedule, as before."""
        sc = torch.as_tensor(sched).reshape(-1).to("cpu", torch.long)
        jumps = su.has_jumps(sc)
        if self.solver == "dpmpp_2m" and sc.numel() >= 2:
            s, seen, ok = sc.tolist(), set(), True
            for a, b in zip(s[:-1], s[1:]):
                seen.add(a)
                ok = ok and (b < a or (b > a and b in seen))
            if not ok:
                raise ValueError("solver 'dpmpp_2m' needs a strictly decreasing schedule (its history step must lie above t_now), or "
                                 "strictly decreasing runs joined by the up-jumps of schedule_utils.resample_schedule, which return to "
                                 "a timestep already passed")
        if not jumps:
            return
        su.step_segments(sc, None)                  # equal neighbours
        self._renoise_keying()

    # ---- RePaint resampling: the forward jump of a schedule with up-jumps ----
    def _renoise_hop(self) -> Optional[int]:
        """the hop of the canvas keying the renoise takes (the engine's canvas_hop or a canvas-keyed guide's; when both are set they
        agree: set_known checks it), None = keyed per sample"""
        if self.canvas_hop is not None:
            return self.canvas_hop
        return self._guide_hop if self._guide is not None else None

    def _renoise_keying(self) -> Optional[int]:
        """the checks every renoise makes (``check_schedule`` makes them before the first step); returns ``_renoise_hop()``"""
        if self._key is None:
            raise ValueError("a schedule with up-jumps (resampling) draws its renoise normals from the seeded stream: build the engine "
                             "with noise_seed (also at eta == 0)")
        hop = self._renoise_hop()
        if self._cons_hop is not None and hop != self._cons_hop:
            raise ValueError("window consensus needs the renoise of a resampling schedule keyed by canvas position at the consensus "
                             "hop: the mean of the windows' independent renoise draws would shrink their variance (build the engine "
                             "with noise_keying='canvas', canvas_hop=hop, or set a canvas-keyed guide with that hop)")
        if self._guide is not None and (self._guide_hop is None) != (hop is None):
            raise ValueError("a guide keyed per sample cannot end a canvas-keyed renoise: set_known(..., keying='canvas', hop=canvas_hop)")
        return hop

    def renoise(self, z: torch.Tensor, t_from: torch.Tensor, t_to: torch.Tensor, visit: int,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The forward jump t_from -> t_to of a resampling schedule (include/avdiff_hip.h, "renoise"): out = sqrt(rho) z + sqrt(1 - rho)
        n_r with rho = a(t_to) / a(t_from), n_r drawn from (noise_seed, sample_offset + b, visit) — or by canvas position when the
        engine has ``canvas_hop`` or a canvas-keyed guide; a ``set_known`` guide ends the launch in its blend at t_to, so a held region
        stays on its forward path.  One eager launch; ``out`` may be ``z`` (in place).  No consensus pass follows: on windows that
        agree, the jump is the same linear map with the same normals."""
        hop = self._renoise_keying()
        z = L.dev_f32(z, "z")
        if tuple(z.shape) != self.latent_shape:
            raise ValueError(f"latent shape {tuple(z.shape)} != engine shape {self.latent_shape}")
        return Fn.renoise(z, t_from, t_to, self.alpha_bar, self.noise_seed, visit, self.sample_offset, guide=self._guide,
                          canvas_hop=hop, out=out)

    def advance_renoise(self, z: torch.Tensor, visit: int) -> None:
        """``renoise`` in place at the cursor's pair (t_from, t_to) = (sched[i], sched[i + 1]); the cursor moves on, so the steps that
        follow — eager or replayed from a captured pair — read the right timesteps."""
        self._advance_cursor(False)
        self.renoise(z, self._tn, self._tp, visit, out=z)

    def run(self, z: torch.Tensor, sched: torch.Tensor, graph: Optional[bool] = None) -> torch.Tensor:
        """Apply len(sched)-1 steps.  ``graph=True`` replays a captured two-step HIP graph; ``None`` (default) does so when the
        batch is small enough for the step to be launch-bound (2B*N < 6,144 rows, eta == 0 or a seeded engine) — results are
        bit-identical either way (tests: test_chained_sampler_golden, test_gpu_seeded_noise).
        With a ``guidance_interval`` the schedule is read on the host and split into maximal segments of CFG and of cond-only steps
        (schedule_utils.guidance_segments); the device cursor runs on across them.  Each kind follows the rule above with its own
        row count (B*N for cond-only steps), takes its own warm-up step outside capture and keeps its own captured pair for the
        whole run; capturing one kind leaves the other's pair valid.
        A resampling schedule (schedule_utils.resample_schedule: RePaint resampling; recognised by schedule_utils.has_jumps, an
        up-jump back to a timestep already passed) is split the same way (schedule_utils.step_segments): a pair sched[i] <
        sched[i + 1] is a renoise — one eager launch, in place in the current
        latent buffer, visit = i, its timesteps read off the device cursor (``advance_renoise``) — so the captured pairs of the
        denoising kinds stay valid and aligned.  It needs ``noise_seed``, and under a window consensus the canvas keying
        (``check_schedule``).  Solver "dpmpp_2m" takes the first step after a jump first order (avd_sched_advance_ms leaves t_last = -1
        there) and overwrites x0_hist with it.  Limit: at eta > 0 the step noise stays keyed by (sample, t_now, element), so a
        revisited timestep repeats its step normals; only the renoise normals are fresh per visit.
        One loop runs every schedule (schedule_utils.trajectory_segments; a plain schedule is one CFG segment).  A captured pair steps
        cur -> other -> cur between the two latent buffers it was captured on, so it is replayed only while the trajectory sits in
        its source buffer; a single eager step puts it there.  A renoise pair works in place in ``cur`` and swaps nothing."""
        self._clip_refusal("run", "a clip guide is keyed by the clip positions of step_slots' slots; a trajectory is guided by set_known")
        self._clips_refusal("run")
        self._slot_cfg_refusal("run")
        self.check_schedule(sched)
        segs = su.trajectory_segments(sched, self.guidance_interval)
        graphable = self.eta == 0 or self._key is not None
        use_graph = {}
        for cfg in (True, False):
            rows = (2 if cfg else 1) * self.embed.B * self.N
            use_graph[cfg] = (graphable and rows < self.GRAPH_BELOW_ROWS) if graph is None else bool(graph)
        self.begin(sched)
        cur = L.dev_f32(z, "z").clone()
        other = torch.empty_like(cur)
        warmed, pairs = set(), {}                   # per kind: warm-up step taken; (captured pair, its source buffer)
        for start, stop, kind in segs:
            if kind == "renoise":
                for i in range(start, stop):
                    self.advance_renoise(cur, i)
                continue
            cfg = kind == "cfg"
            left, cond = stop - start, not cfg
            while left:
                replay = False
                if use_graph[cfg] and cfg in warmed and left >= 2:
                    if cfg not in pairs:
                        pairs[cfg] = (self.capture_pair(cur, other, cond), cur)      # capture enqueues nothing
                    replay = pairs[cfg][1] is cur
                if replay:
                    for _ in range(left // 2):
                        pairs[cfg][0].replay()
                    self._last_cond_only = cond
                    left %= 2
                else:                               # warm-up, a segment's odd step, or the step that realigns the buffers
                    self.advance(cur, other, cond)
                    cur, other = other, cur
                    warmed.add(cfg)
                    left -= 1
        return cur


def _scalar_like(v) -> bool:
    """a single number (not a sequence): the same guidance for every sample, the plain step's scalar"""
    return isinstance(v, (int, float, np.generic)) or (isinstance(v, (torch.Tensor, np.ndarray)) and v.ndim == 0)


def frame_mask(latent_shape, lo: int, hi: int) -> torch.Tensor:
    """A latent guide mask (DenoiseEngine.set_known, sample_one_direction ``mask``): float32 ones on latent frames [lo, hi) and zeros
    elsewhere — the T axis of a video latent ([C,T,H,W] or [B,C,T,H,W]), the F axis of an audio latent ([Ca,F] or [B,Ca,F]).
    "Keep the first frames and generate what follows" is frame_mask(shape, 0, k).  CPU tensor of ``latent_shape``."""
    shape = tuple(int(s) for s in latent_shape)
    if len(shape) in (4, 5):
        axis = len(shape) - 3
    elif len(shape) in (2, 3):
        axis = len(shape) - 1
    else:
        raise ValueError(f"latent_shape {shape} is neither a video ([B,]C,T,H,W) nor an audio ([B,]Ca,F) latent")
    n = shape[axis]
    if not 0 <= lo <= hi <= n:
        raise ValueError(f"frames [{lo}, {hi}) must lie within [0, {n}]")
    m = torch.zeros(shape, dtype=torch.float32)
    idx = [slice(None)] * len(shape)
    idx[axis] = slice(lo, hi)
    m[tuple(idx)] = 1.0
    return m


def canvas_frame_mask(canvas_shape, lo: int, hi: int) -> torch.Tensor:
    """``frame_mask`` on a latent canvas (stream_generate ``mask``): float32 ones on canvas positions [lo, hi) and zeros elsewhere — the P
    axis of a video canvas [C,P,H,W] or of an audio canvas [Ca,P].  "Keep the first positions of the long clip and generate what
    follows" is canvas_frame_mask(shape, 0, k).  CPU tensor of ``canvas_shape``."""
    shape = tuple(int(s) for s in canvas_shape)
    if len(shape) not in (2, 4):
        raise ValueError(f"canvas_shape {shape} is neither a video ([C,P,H,W]) nor an audio ([Ca,P]) latent canvas")
    return frame_mask(shape, lo, hi)


# ----------------------------------------------------------------------------------------------------------
# reference-signature entry point (B = 1, codec / VAE supplied by the caller)
# ----------------------------------------------------------------------------------------------------------

@torch.no_grad()
def sample_one_direction(*, cfg: Dict, vid_vae, aud_codec, adapt_v: LinearAdapter, adapt_a: LinearAdapter,
                         core: MMDiT, head: MultiModalNoiseHead, tstep_dim: int, prompt_modality: str,
                         prompt_video: Optional[np.ndarray], prompt_audio: Optional[np.ndarray],
                         device: torch.device, init_noise: Optional[torch.Tensor] = None,
                         noise_seed: Optional[int] = None, init_video: Optional[np.ndarray] = None,
                         init_audio: Optional[np.ndarray] = None, strength: float = 1.0, mask=None,
                         guide_seed: Optional[int] = None, guidance_interval=None, resample=None) -> Dict[str, np.ndarray]:
    """sample_clip.py:220-394 with the loop on the HIP engine.  The V->A branch uses the [1,3,T,H,W] layout the
    reference's comment intends (its own permute at :288 is a bug that crashes in conv3d).
    ``init_noise`` (extension; default None = draw it as the reference does, :297 / :304): the target's initial latent, so that a
    run can be repeated across devices — the reference's only RNG draw comes from the device generator.
    ``noise_seed`` (extension; default None = the reference's per-step ``randn_like``): with ``sampling.ddim_eta`` > 0 the per-step
    DDIM noise comes from the seeded stream (DenoiseEngine ``noise_seed``), so the whole trajectory repeats from (init_noise,
    noise_seed).
    ``sampling.solver`` (extension; default "ddim"): "dpmpp_2m" samples with DPM-Solver++(2M) (DenoiseEngine ``solver``) over the
    same ``sampler_steps`` schedule; with ``sampling.ddim_eta`` > 0 it runs the solver's SDE form, which needs ``noise_seed``.
    ``init_video`` (uint8 [T,H,W,3], audio->video) / ``init_audio`` (float waveform, video->audio), ``strength``, ``mask``,
    ``guide_seed`` (extensions; the defaults change nothing): start from, or hold on to, an existing clip of the target modality,
    encoded with the same ``vid_vae`` / ``aud_codec``.  ``strength`` < 1 runs the last part of the schedule from the encoded clip
    noised to that point (SDEdit, schedule_utils.truncate_schedule; 0 returns the decoded clip).  ``mask`` (latent-shaped for one
    sample, e.g. ``frame_mask``; 1 = keep) holds the trajectory to the clip there at every step (DenoiseEngine.set_known); without
    a mask the whole latent is free.  ``guide_seed`` keys the clip's forward noise (default ``noise_seed``, else 0).
    ``sampling.guidance_rescale`` (extension; a per-modality dict like ``guidance_scale``, default 0): CFG rescale phi of the target
    (DenoiseEngine ``guidance_rescale``); 0 runs the plain step.
    ``sampling.apg`` (extension; a per-modality dict like ``guidance_scale``, each entry a dict of norm_threshold / eta_parallel /
    momentum; default none): adaptive projected guidance for the target (DenoiseEngine ``apg``) in place of the CFG combine.
    ``guidance_interval`` (extension; default None) or ``sampling.guidance_interval`` (a per-modality dict of [t_lo, t_hi] like
    ``guidance_scale``; the argument wins): apply guidance only on steps with t_lo <= t_now <= t_hi, step on the conditional
    prediction alone elsewhere (DenoiseEngine ``guidance_interval``).
    ``resample`` (extension; default None) = (jump, resamples), or ``sampling.resample: {jump:, resamples:}`` (the argument wins):
    RePaint resampling of a masked init clip — after every ``jump`` steps the latent is sent back up the schedule by a seeded forward
    jump and the stretch is denoised again, ``resamples`` passes in all (schedule_utils.resample_schedule, applied after ``strength``
    has truncated the schedule; DenoiseEngine ``renoise``), so that the generated region harmonises with the held one.  It needs an
    init clip with a ``mask``, and ``noise_seed`` (the key of the renoise normals, also at ``ddim_eta`` == 0); resamples == 1 is
    today's run.  At ``ddim_eta`` > 0 a revisited timestep repeats its step normals; only the jumps draw fresh ones."""
    strength = P.check_init_args(prompt_modality, init_video, init_audio, strength, mask)
    init = P.init_clip_array(init_video, init_audio)
    pc = P.read_config(cfg, prompt_modality, guidance_interval=guidance_interval, resample=resample, has_init=init is not None,
                       has_mask=mask is not None, noise_seed=noise_seed)
    if pc.target == "audio":
        if prompt_video is None:
            raise ValueError("prompt_video frames required for prompt_modality=video")
        z_p = P.encode_video(vid_vae, prompt_video, device)                          # [1,3,T,H,W] -> [1,Cv,T',H',W']
        lat_shape = (1, pc.Ca, pc.Fa)
    else:
        if prompt_audio is None:
            raise ValueError("prompt_audio required for prompt_modality=audio")
        z_p = P.encode_audio(aud_codec, prompt_audio, device, as_float32=False)      # [1,Ca,Fa]
        T_in = prompt_video.shape[0] if prompt_video is not None else int(round(cfg["data"]["clip_seconds"] * pc.fps))
        lat_shape = (1, pc.Cv, max(1, T_in // pc.t_down), pc.H // pc.s_down, pc.W // pc.s_down)
    z = torch.randn(*lat_shape, device=device) if init_noise is None else init_noise.to(device).float()
    if tuple(z.shape) != lat_shape:
        raise ValueError(f"init_noise has shape {tuple(z.shape)}, expected {lat_shape}")
    eng = P.build_engine(pc, adapt_v=adapt_v, adapt_a=adapt_a, core=core, head=head, tstep_dim=tstep_dim, latent_shape=lat_shape,
                         n_prompt=P.prompt_tokens(pc, z_p.shape), noise_seed=noise_seed)
    eng.set_prompt(z_p.float())
    sched = pc.sched
    if init is not None:
        known = P.encode_video(vid_vae, init, device) if pc.target == "video" else P.encode_audio(aud_codec, init, device)
        if tuple(known.shape) != lat_shape:
            raise ValueError(f"the init clip encodes to a latent of shape {tuple(known.shape)}, the target's is {lat_shape}")
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, dtype=torch.float32)
            if m.dim() == len(lat_shape):
                m = m.squeeze(0)
            if tuple(m.shape) != lat_shape[1:]:
                raise ValueError(f"mask has shape {tuple(m.shape)}, expected one sample's latent shape {lat_shape[1:]}")
        z, sched = P.guided_start(eng, pc, known, m, z, strength, P.default_guide_seed(guide_seed, noise_seed))
    z = eng.run(z, sched)
    if pc.target == "audio":
        return {"audio": aud_codec.decode(z).squeeze(0).squeeze(0).detach().cpu().numpy(), "sr": pc.sr}
    x_hat = vid_vae.decode(z).clamp(0, 1)
    return {"video": (x_hat[0].permute(1, 2, 3, 0).detach().cpu().numpy() * 255.0).astype(np.uint8), "fps": pc.fps}
