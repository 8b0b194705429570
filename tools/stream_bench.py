#!/usr/bin/env python3
"""One long audio -> video clip through stream_generate's three samplers on one GPU, end to end (split, encode, denoise, decode,
cross-fade): independent windows, windows under latent consensus, and the FIFO queue (sampler="fifo"), at the C3 geometry (256 x 256,
3 s windows every 1 s: 12 latent frames per window, hop 4; tube 2 x 4 x 4: S = 6; 8 layers) and one step count.  The three calls run
interleaved in one process after a warm-up call each; the median per sampler is printed, beside the time of the front end all three
share (the prompt windows' encode, and the decode + cross-fade of the windows' latents, timed on their own).
The FIFO figure includes the queue's ramp (steps - 1 model calls before the first slot finishes).  Quality is not measured: there are
no trained weights.  The record is profiles/stream_fifo_e2e.txt.

--prompt-frac kernels | e2e times the fractional prompt hop (include/avdiff_hip.h, "fractional prompt hop") instead:
  kernels   functional.fifo_prompt_gather_frac in both modes beside the integer functional.fifo_prompt_gather at the two C3 prompt shapes
            (the audio prompt of a video target: canvas [8, P], windows of 148 frames, hop 25; the video prompt of an audio target:
            canvas [8, P, 32, 32], windows of 12 latent frames, hop 8 / 25), B = 8 and 32, off a device cursor: at den = 1, where it
            reads the integer gather's rows, and at a true fraction.  Device events around --launches back-to-back launches, the
            variants interleaved over --rounds rounds, all rounds printed.  On a checkout without the fractional gather the integer
            rows alone are timed, so the same command on the parent commit gives the figures to compare.
  e2e       one video -> audio clip through the windows sampler and through sampler="fifo" with prompt_interp "linear" and "nearest"
            (eager, and "linear" replayed from HIP graphs), --steps steps (74 = 2 x the S = 37 slots of an audio sample).
The records are profiles/fifo_prompt_frac_kernels.txt and profiles/fifo_prompt_frac_e2e.txt."""
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
ap.add_argument("--prompt-frac", choices=("kernels", "e2e"), default=None, help="time the fractional prompt hop instead (see above)")
ap.add_argument("--launches", type=int, default=200, help="--prompt-frac kernels: launches per timed window")
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
geo = S.fifo_geometry(cfg, "audio", n_windows, args.steps) if args.prompt_frac is None else None
kw = dict(cfg=cfg, vid_vae=vae, aud_codec=codec, adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tdim, device=dev,
          prompt_modality="audio", prompt_video=None, prompt_audio=wav, seed=1, max_windows_per_batch=32)
kinds = [("windows", {}), ("consensus", dict(consensus="uniform")), ("fifo", dict(sampler="fifo"))]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def prompt_frac_kernels():
    from multimodal_diffusion_amd import functional as Fn
    has_frac = hasattr(Fn, "fifo_prompt_gather_frac")
    g = torch.Generator().manual_seed(3)
    cursor = torch.tensor([1], dtype=torch.int32, device=dev)
    # name, canvas, S, prompt_len, the whole hop, the true fraction
    shapes = [("audio prompt [8, 6000], windows of 148 (inner 1: one element per lane)", torch.randn(8, 6000, generator=g).to(dev), 6, 148, 25, (51, 2)),
              ("video prompt [8, 1200, 32, 32], windows of 12 (inner 1024: 16-byte lanes)", torch.randn(8, 1200, 32, 32, generator=g).to(dev), 37, 12,
               1, (8, 25))]
    print(f"prompt gathers off a device cursor (m = 1), microseconds per launch: device events around {args.launches} back-to-back "
          f"launches (launch overhead included), {args.rounds} interleaved rounds after a warm-up, then the median; bytes = output written "
          "+ canvas rows read (twice in \"linear\" at a true fraction)")
    if not has_frac:
        print("  this checkout has no fractional gather: the integer gather alone")
    for name, canvas, S_, Lp, hop, (num, den) in shapes:
        for B in (8, 32):
            out = torch.empty((B, 8, Lp) + tuple(canvas.shape[2:]), device=dev)
            cases = [(f"integer, hop {hop}", 2, lambda: Fn.fifo_prompt_gather(canvas, cursor, B, S_, hop, Lp, out=out))]
            if has_frac:
                for mode in Fn.PROMPT_INTERPS:
                    cases.append((f"{mode}, hop {hop} / 1", 2,
                                  lambda mode=mode: Fn.fifo_prompt_gather_frac(canvas, cursor, B, 0, S_, hop, 1, mode, Lp, out=out)))
                for mode in Fn.PROMPT_INTERPS:
                    cases.append((f"{mode}, hop {num} / {den}", 3 if mode == "linear" else 2,
                                  lambda mode=mode: Fn.fifo_prompt_gather_frac(canvas, cursor, B, 0, S_, num, den, mode, Lp, out=out)))
            us = {c[0]: [] for c in cases}
            for rnd in range(args.rounds + 1):
                for label, _, fn in cases:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(args.launches):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    if rnd:
                        us[label].append(1e3 * e0.elapsed_time(e1) / args.launches)
            print(f"  {name}, B = {B}: out {out.numel() * 4 / 1e6:.2f} MB")
            for label, streams, _ in cases:
                v = us[label]
                med = statistics.median(v)
                print(f"    {label:22s} " + " ".join(f"{t:7.2f}" for t in v) + f"   median {med:7.2f}   "
                      f"{streams * out.numel() * 4 / med / 1e3:7.1f} GB/s")


def prompt_frac_e2e():
    cfg2 = dict(cfg, diffusion={m: dict(cfg["diffusion"][m], sampler_steps=args.steps) for m in ("video", "audio")})
    vid = torch.randint(0, 256, (int(args.seconds * 16), 256, 256, 3), generator=torch.Generator().manual_seed(11), dtype=torch.uint8).numpy()
    n_win = S.split_frames_into_windows(vid, 16, 3.0, 1.0)[0].shape[0]
    geo2 = S.fifo_geometry(cfg2, "video", n_win, args.steps, prompt_interp="linear")
    kw2 = dict(kw, cfg=cfg2, prompt_modality="video", prompt_video=vid, prompt_audio=None)
    runs = [("windows", {})] + [(f"fifo {mode}" + (", graph" if graph else ""),
                                 dict(sampler="fifo", fifo={"steps": args.steps, "prompt_interp": mode, "graph": graph}))
                                for mode, graph in (("linear", False), ("nearest", False), ("linear", True))]
    wavs = {name: S.stream_generate(**dict(kw2, **extra))["audio"] for name, extra in runs}      # the warm-up calls
    tt = {name: [] for name, _ in runs}
    for _ in range(args.rounds):
        for name, extra in runs:
            tt[name].append(timed(lambda: S.stream_generate(**dict(kw2, **extra)))[0])
    secs = wavs["windows"].shape[0] / 16000
    print(f"stream_generate, video -> audio, one clip of {args.seconds:g} s = {n_win} windows of 3 s every 1 s ({secs:g} s of audio out), "
          f"{args.steps} steps, C3 geometry (audio latent window [8, 150], hop 50, chunks of 4; video prompt 256 x 256: latent [8, 12, 32, 32] "
          f"per window; 8 layers, {args.matmul}, DDIM eta 0), end to end (split, encode, denoise, decode, cross-fade), {args.rounds} interleaved "
          "rounds after one warm-up call each; milliseconds")
    print(f"  the FIFO queue: B = {geo2.B} samples of S = {geo2.S} slots of {geo2.slot_len}, prompt hop {geo2.prompt_hop} / {geo2.prompt_den} "
          f"positions per slot, canvas P = {geo2.P} latent frames = {geo2.n_slots} slots; its figures include the ramp ({args.steps - 1} model "
          f"calls before the first of {geo2.n_slots} steady iterations)")
    for name, _ in runs:
        v = tt[name]
        med = statistics.median(v)
        print(f"  {name:20s} " + " ".join(f"{t * 1e3:8.1f}" for t in v) + f"   median {med * 1e3:8.1f}   per output second {1e3 * med / secs:.1f}"
              f"   x {med / statistics.median(tt['windows']):.3f} of windows")
    print(f"  model calls: windows {args.steps} steps at batch {n_win}; fifo {args.steps - 1} + {geo2.n_slots} steps at batch {geo2.B}")
    assert all(w.shape == wavs["windows"].shape for w in wavs.values())
    print("  quality is not measured: there are no trained weights, so neither sampler nor prompt_interp mode can be ranked by ear or metric")


if args.prompt_frac is not None:
    prompt_frac_kernels() if args.prompt_frac == "kernels" else prompt_frac_e2e()
    sys.exit(0)

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
