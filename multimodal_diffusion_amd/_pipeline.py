"""The front end that ``sampler.sample_one_direction`` and ``stream_infer.stream_generate`` share: the device-free argument checks,
the config read-out, clip encoding, the prompt-token count, engine construction and the guided start.  Plain functions over one
record of config values; the two pipelines keep what is their own (windows, consensus, sharding, decode)."""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import schedule_utils as su


def tube_from_config(cfg: Dict) -> Tuple[int, int, int]:
    """tokenizer.video.tube as (t, h, w); a config without "w" has the reference's square tube (w = h)"""
    tube = cfg["tokenizer"]["video"]["tube"]
    return int(tube["t"]), int(tube["h"]), int(tube.get("w", tube["h"]))


# ---- argument checks that need no device ----
def check_init_args(prompt_modality: str, init_video, init_audio, strength, mask) -> float:
    """the latent guide's arguments of a pipeline call; returns ``strength`` as a float"""
    strength = float(strength)
    if not 0.0 <= strength <= 1.0:
        raise ValueError(f"strength must lie in [0, 1], got {strength}")
    if init_video is not None and init_audio is not None:
        raise ValueError("pass init_video or init_audio, not both")
    if init_video is None and init_audio is None and (mask is not None or strength < 1.0):
        raise ValueError("a mask or a strength < 1 needs an init clip (init_video for audio->video, init_audio for video->audio)")
    if init_video is not None and prompt_modality != "audio":
        raise ValueError("init_video is the target of the audio->video direction (prompt_modality='audio')")
    if init_audio is not None and prompt_modality != "video":
        raise ValueError("init_audio is the target of the video->audio direction (prompt_modality='video')")
    return strength


def init_clip_array(init_video, init_audio) -> Optional[np.ndarray]:
    """the init clip as an array once its form is checked (uint8 [T,H,W,3] frames / a 1-D floating waveform); None without one"""
    if init_video is not None:
        init = np.asarray(init_video)
        if init.ndim != 4 or init.shape[-1] != 3 or init.dtype != np.uint8:
            raise ValueError(f"init_video must be uint8 [T,H,W,3], got {init.dtype} {init.shape}")
        return init
    if init_audio is not None:
        init = np.asarray(init_audio)
        if init.ndim != 1 or not np.issubdtype(init.dtype, np.floating):
            raise ValueError(f"init_audio must be a float waveform [N], got {init.dtype} {init.shape}")
        return init
    return None


def check_resample_args(rs, has_init: bool, has_mask: bool, noise_seed) -> None:
    """what RePaint resampling asks of a pipeline call: ``rs`` None or (jump, resamples)"""
    if rs is None:
        return
    if not (has_init and has_mask):
        raise ValueError("resample (RePaint resampling) harmonises a generated region with a held one: it needs an init clip with a "
                         "mask (init_video / init_audio and mask)")
    if noise_seed is None:
        raise ValueError("resample draws its forward jumps from the seeded stream: it needs noise_seed (also at ddim_eta == 0)")


# ---- the config read-out ----
class PipelineConfig(NamedTuple):
    """what a pipeline call reads from its config; the last six are the target's"""
    target: str                       # the generated modality: "audio" for a video prompt, "video" for an audio prompt
    tube: Tuple[int, int, int]
    chunk: Tuple[int, int]            # (length, stride)
    Cv: int
    t_down: int
    s_down: int
    Ca: int
    Fa: int
    H: int
    W: int
    fps: int
    sr: int
    eta: float
    solver: str                       # "ddim" | "dpmpp_2m" (DenoiseEngine ``solver``)
    alpha_bar: torch.Tensor
    sched: torch.Tensor
    guidance: float
    rescale: float                    # sampling.guidance_rescale: per modality, like guidance_scale
    interval: Optional[Tuple[int, int]]
    resample: Optional[Tuple[int, int]]
    apg: Optional[Tuple[float, float, float]] = None      # sampling.apg: per modality; (norm_threshold, eta_parallel, momentum)


def read_config(cfg: Dict, prompt_modality: str, *, guidance_interval, resample, has_init: bool, has_mask: bool,
                noise_seed) -> PipelineConfig:
    """The config values of one pipeline call.  ``guidance_interval`` / ``resample`` are the call's arguments: they win over
    ``sampling.guidance_interval`` / ``sampling.resample``; the resample setting is checked against the call (``check_resample_args``)
    before anything else is read."""
    scfg = cfg["sampling"]
    rs = su.check_resample(resample) or su.resample_from_config(scfg)
    check_resample_args(rs, has_init, has_mask, noise_seed)
    if prompt_modality not in ("video", "audio"):
        raise ValueError("prompt_modality must be 'video' or 'audio'")
    target = "audio" if prompt_modality == "video" else "video"
    chunk = cfg["tokenizer"]["audio"]["chunk"]
    Cv, t_down, s_down = (int(cfg["video"]["latent"][k]) for k in ("channels", "t_down", "s_down"))
    c = cfg["diffusion"][target]
    betas = su.make_beta_schedule(int(c["steps"]), kind=c["schedule"], min_beta=c["min_beta"], max_beta=c["max_beta"])
    return PipelineConfig(
        target=target, tube=tube_from_config(cfg), chunk=(int(chunk["length"]), int(chunk["stride"])),
        Cv=Cv, t_down=t_down, s_down=s_down,
        Ca=int(cfg["audio"]["latent"]["channels"]), Fa=int(cfg["audio"]["latent"]["frames_per_clip"]),
        H=int(cfg["video"]["size"][0]), W=int(cfg["video"]["size"][1]), fps=int(cfg["video"]["fps"]), sr=int(cfg["audio"]["sr"]),
        eta=float(scfg.get("ddim_eta", 0.0)), solver=str(scfg.get("solver", "ddim")),
        alpha_bar=su.alphas_cumprod_from_betas(betas)[1], sched=su.make_sampling_schedule(int(c["steps"]), int(c["sampler_steps"])),
        guidance=float(scfg["guidance_scale"].get(target, 3.0)), rescale=float(scfg.get("guidance_rescale", {}).get(target, 0.0)),
        interval=su.check_guidance_interval(guidance_interval) or su.guidance_interval_from_config(scfg, target), resample=rs,
        apg=apg_from_config(scfg, target))


def apg_from_config(scfg: Dict, target: str) -> Optional[Tuple[float, float, float]]:
    """``sampling.apg``: a per-modality dict like ``guidance_scale``; the target's entry is a dict with any of norm_threshold /
    eta_parallel / momentum (functional.apg_params checks them).  None without an entry for the target."""
    from . import functional as Fn
    apg = scfg.get("apg")
    if apg is None:
        return None
    if not isinstance(apg, dict) or set(apg) - {"video", "audio"}:
        raise ValueError(f"sampling.apg must be a dict per modality ('video' / 'audio'), got {apg!r}")
    vals = Fn.apg_from_dict(apg.get(target))
    if vals is not None and float(scfg.get("guidance_rescale", {}).get(target, 0.0)) != 0.0:
        raise ValueError("sampling.apg cannot be combined with sampling.guidance_rescale != 0 for the same target")
    return vals


# ---- clips to latents ----
def encode_video(vid_vae, frames: np.ndarray, device: torch.device) -> torch.Tensor:
    """uint8 frames [T,H,W,3] (one clip) or [N,T,H,W,3] -> ``vid_vae.encode`` of [N,3,T,H,W] float in [0, 1]: [N,Cv,T',H',W']"""
    x = torch.from_numpy(np.ascontiguousarray(frames)).to(device).float() / 255.0
    if x.dim() == 4:
        x = x.unsqueeze(0)
    return vid_vae.encode(x.permute(0, 4, 1, 2, 3).contiguous())


def encode_audio(aud_codec, wav: np.ndarray, device: torch.device, as_float32: bool = True) -> torch.Tensor:
    """waveform [n] (one clip) or [N,n] -> ``aud_codec.encode`` of [N,1,n]: [N,Ca,Fa].  ``as_float32=False`` hands the samples over in
    their own dtype (``sample_one_direction``'s prompt, as the reference: the codec decides what it takes)."""
    x = torch.from_numpy(np.ascontiguousarray(wav, dtype=np.float32 if as_float32 else None)).to(device)
    if x.dim() == 1:
        x = x[None, :]
    return aud_codec.encode(x[:, None, :])


def prompt_tokens(pc: PipelineConfig, zp_shape) -> int:
    """the prompt rows of an encoded prompt [N,Cv,T',H',W'] (tubes) or [N,Ca,Fa] (chunks)"""
    if pc.target == "audio":
        t, h, w = pc.tube
        return (zp_shape[2] // t) * (zp_shape[3] // h) * (zp_shape[4] // w)
    length, stride = pc.chunk
    return (zp_shape[-1] - length) // stride + 1


def default_guide_seed(guide_seed: Optional[int], noise_seed: Optional[int]) -> int:
    """``guide_seed``, else ``noise_seed``, else 0"""
    return guide_seed if guide_seed is not None else (noise_seed if noise_seed is not None else 0)


# ---- the engine and its guided start ----
def build_engine(pc: PipelineConfig, *, adapt_v, adapt_a, core, head, tstep_dim: int, latent_shape, n_prompt: int, noise_seed,
                 **streaming):
    """the DenoiseEngine of ``pc``'s target; ``streaming``: the keywords only stream_generate sets (sample_offset, noise_keying,
    canvas_hop)"""
    from .sampler import DenoiseEngine      # sampler imports this module
    return DenoiseEngine(adapt_v=adapt_v, adapt_a=adapt_a, core=core, head=head, tstep_dim=tstep_dim, target=pc.target,
                         latent_shape=tuple(latent_shape), prompt_tokens=n_prompt, alpha_bar=pc.alpha_bar, guidance=pc.guidance,
                         eta=pc.eta, tube=pc.tube, chunk=pc.chunk, noise_seed=noise_seed, solver=pc.solver,
                         guidance_rescale=pc.rescale, guidance_interval=pc.interval,
                         apg=None if pc.apg is None else dict(zip(("norm_threshold", "eta_parallel", "momentum"), pc.apg)), **streaming)


def guided_start(eng, pc: PipelineConfig, known: torch.Tensor, mask, z: torch.Tensor, strength: float, guide_seed: int, **keying):
    """(z_start, schedule) of a trajectory guided by the encoded init clip ``known`` (DenoiseEngine.set_known / start_latent): the
    schedule is truncated by ``strength``, then expanded by ``pc.resample``.  ``mask`` None: SDEdit without a mask — the guide is
    cleared after the start, the whole latent is free and the plain step runs.  ``keying``: set_known's canvas keywords."""
    eng.set_known(known, torch.zeros(eng.latent_shape[1:]) if mask is None else mask, guide_seed=guide_seed, **keying)
    z, sched = eng.start_latent(z, pc.sched, strength)
    if mask is None:
        eng.clear_known()
    return z, (sched if pc.resample is None else su.resample_schedule(sched, *pc.resample))
