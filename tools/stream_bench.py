#!/usr/bin/env python3
"""One long audio -> video clip through stream_generate's three samplers on one GPU, end to end (split, encode, denoise, decode,
cross-fade): independent windows, windows under latent consensus, and the FIFO queue (sampler="fifo"), at the C3 geometry (256 x 256,
3 s windows every 1 s: 12 latent frames per window, hop 4; tube 2 x 4 x 4: S = 6; 8 layers) and one step count.  The three calls run
interleaved in one process after a warm-up call each; the median per sampler is printed, beside the time of the front end all three
share (the prompt windows' encode, and the decode + cross-fade of the windows' latents, timed on their own).
The FIFO figure includes the queue's ramp (steps - 1 model calls before the first slot finishes).  Quality is not measured: there are
no trained weights.  The record is profiles/stream_fifo_e2e.txt."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import multimodal_diffusion_amd as A                                   # noqa: E402
from multimodal_diffusion_amd import stream_infer as S                 # noqa: E402
import bench                                                           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--seconds", type=float, default=22.0, help="length of the prompt clip (3 s windows every 1 s)")
ap.add_argument("--steps", type=int, default=48, help="sampler steps of all three samplers (a multiple of S = 6)")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--matmul", default="bf16x3", help="matrix-pipe mode (default: bench.py's headline mode)")
args = ap.parse_args()

dev = torch.device("cuda:0")
(av, aa, core, head), tdim = bench.build_modules(dev)
core.matmul = head.matmul = args.matmul
torch.manual_seed(0)
vae = A.VideoVAE.from_config({"latent": {"channels": 8, "t_down": 4, "s_down": 8}}).eval().to(dev)
codec = A.AudioCodec.from_config({"sr": 16000, "latent": {"channels": 8, "frames_per_clip": 150}, "codec": {"hop_samples": 320}}).eval().to(dev)
cfg = {"tokenizer": {"width": 512, "video": {"tube": {"t": 2, "h": 4, "w": 4}}, "audio": {"chunk": {"length": 4, "stride": 4}}},
       "video": {"fps": 16, "size": [256, 256], "latent": {"channels": 8, "t_down": 4, "s_down": 8}},
       "audio": {"sr": 16000, "latent": {"channels": 8, "frames_per_clip": 150}},
       "data": {"clip_seconds": 3.0},
       "diffusion": {m: {"steps": 1000, "sampler_steps": args.steps, "schedule": "cosine", "min_beta": 1e-4, "max_beta": 0.02}
                     for m in ("video", "audio")},
       "sampling": {"guidance_scale": {"video": 3.5, "audio": 3.5}},
       "streaming": {"window_seconds": 3.0, "hop_seconds": 1.0, "crossfade_seconds": 0.25}}
wav = (0.1 * torch.randn(int(args.seconds * 16000), generator=torch.Generator().manual_seed(9))).numpy()
n_windows = S.split_audio_into_windows(wav, 16000, 3.0, 1.0)[0].shape[0]
geo = S.fifo_geometry(cfg, "audio", n_windows, args.steps)
kw = dict(cfg=cfg, vid_vae=vae, aud_codec=codec, adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tdim, device=dev,
          prompt_modality="audio", prompt_video=None, prompt_audio=wav, seed=1, max_windows_per_batch=32)
kinds = [("windows", {}), ("consensus", dict(consensus="uniform")), ("fifo", dict(sampler="fifo"))]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


frames = None
for name, extra in kinds:                                  # warm-up: every kernel's first launch, the allocator's pools
    frames = S.stream_generate(**dict(kw, **extra))["video"]
ts = {name: [] for name, _ in kinds}
for _ in range(args.rounds):
    for name, extra in kinds:
        ts[name].append(timed(lambda: S.stream_generate(**dict(kw, **extra)))[0])

# the front end all three share, on its own: the prompt windows' encode, and the decode + cross-fade of N windows of latents
from multimodal_diffusion_amd import _pipeline as P        # noqa: E402
chunks = S.split_audio_into_windows(wav, 16000, 3.0, 1.0)[0]
z = torch.randn(n_windows, 8, 12, 32, 32, device=dev)
pc = P.read_config(cfg, "audio", guidance_interval=None, resample=None, has_init=False, has_mask=False, noise_seed=None)
enc, dec = [], []
for _ in range(args.rounds + 1):
    enc.append(timed(lambda: P.encode_audio(codec, chunks, dev))[0])
    dec.append(timed(lambda: S._stitch(cfg, pc, S._decode_windows(cfg, pc, vae, codec, (8, 12, 32, 32), z, dev)))[0])
front = statistics.median(enc[1:]) + statistics.median(dec[1:])

print(f"stream_generate, audio -> video, one clip of {args.seconds:g} s = {n_windows} windows of 3 s every 1 s ({frames.shape[0]} frames of "
      f"256 x 256 out), {args.steps} steps, C3 geometry (latent window [8, 12, 32, 32], hop 4; 8 layers, {args.matmul}, DDIM eta 0, eager), "
      f"end to end (split, encode, denoise, decode, cross-fade), {args.rounds} interleaved rounds after one warm-up call each; milliseconds")
print(f"  the FIFO queue: B = {geo.B} samples of S = {geo.S} slots, canvas P = {geo.P} latent frames = {geo.n_slots} slots; its figure "
      f"includes the ramp ({args.steps - 1} model calls before the first of {geo.n_slots} steady iterations)")
for name, _ in kinds:
    v = ts[name]
    med = statistics.median(v)
    print(f"  {name:10s} " + " ".join(f"{t * 1e3:8.1f}" for t in v) + f"   median {med * 1e3:8.1f}   without encode, decode and cross-fade "
          f"({front * 1e3:.1f}) {1e3 * (med - front):8.1f}   per output second {1e3 * med / (frames.shape[0] / 16):.1f}")
w, c, f = (statistics.median(ts[name]) for name, _ in kinds)
print(f"  fifo against windows x {f / w:.3f}, against consensus x {f / c:.3f}")
print("  model calls: windows and consensus " + f"{args.steps} steps at batch {n_windows}; fifo {args.steps - 1} + {geo.n_slots} steps at batch {geo.B}")
print("  quality is not measured: there are no trained weights")
