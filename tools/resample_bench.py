#!/usr/bin/env python3
"""RePaint resampling at C3 geometry on one GPU (the records profiles/resample_kernels.txt and profiles/resample_e2e.txt).

--kernels: per-launch time of avd_renoise_f32 / avd_renoise_canvas_f32 under a guide beside avd_latent_guide_f32 / _canvas_f32 on the
same tensors (latent [B, 8, 12, size/8, size/8], frame_mask over the first 6 of 12 latent frames shared by the batch), from the
library's own launch events (avd_prof_enable / avd_prof_report): one process, interleaved rounds, no tracer.
default: the A->V sampler loop, DDIM, a masked init latent, with resample=(JUMP, RESAMPLES) against the plain schedule, interleaved
in one process; prints the measured time ratio beside the counted ratio of denoising steps."""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import multimodal_diffusion_amd as A                                   # noqa: E402
from multimodal_diffusion_amd import _lib as L                         # noqa: E402
from multimodal_diffusion_amd import functional as Fn                  # noqa: E402
from multimodal_diffusion_amd import schedule_utils as su              # noqa: E402
import bench                                                           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--sampler-steps", type=int, default=50)
ap.add_argument("--resample", type=int, nargs=2, default=(10, 2), metavar=("JUMP", "RESAMPLES"))
ap.add_argument("--matmul", default="bf16x3")
ap.add_argument("--reps", type=int, default=3, help="interleaved rounds")
ap.add_argument("--launches", type=int, default=20, help="with --kernels: launches per entry and round")
ap.add_argument("--kernels", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
B, S, size = args.batch, args.sampler_steps, args.size
shape = (B, 8, 12, size // 8, size // 8)
abar = su.alphas_cumprod_from_betas(su.make_beta_schedule(1000, "cosine", 1e-4, 0.02))[1].to(dev)
g = torch.Generator().manual_seed(1)
z0 = torch.randn(shape, generator=g).to(dev)
known = torch.randn(shape, generator=g).to(dev)
mask = A.frame_mask(shape[1:], 0, 6).to(dev)

if args.kernels:
    hop, seed, gseed = 4, 1234, 99
    guide = Fn.latent_guide_desc(known, mask, gseed, 0)
    tf = torch.full((B,), 499, dtype=torch.long, device=dev)
    tt = torch.full((B,), 699, dtype=torch.long, device=dev)
    out = torch.empty_like(z0)
    entries = {
        "avd_latent_guide_f32": lambda: Fn.latent_guide(known, tt, abar, z=z0, mask=mask, seed=gseed),
        "avd_renoise_f32 (guide)": lambda: Fn.renoise(z0, tf, tt, abar, seed, 7, guide=guide, out=out),
        "avd_renoise_f32 (no guide)": lambda: Fn.renoise(z0, tf, tt, abar, seed, 7, out=out),
        "avd_latent_guide_canvas_f32": lambda: Fn.latent_guide(known, tt, abar, z=z0, mask=mask, seed=gseed, canvas_hop=hop),
        "avd_renoise_canvas_f32 (guide)": lambda: Fn.renoise(z0, tf, tt, abar, seed, 7, guide=guide, canvas_hop=hop, out=out),
        "avd_renoise_canvas_f32 (no guide)": lambda: Fn.renoise(z0, tf, tt, abar, seed, 7, canvas_hop=hop, out=out),
    }
    tags = {"avd_latent_guide_f32": "latent_guide_kernel", "avd_renoise_f32 (guide)": "renoise_kernel",
            "avd_renoise_f32 (no guide)": "renoise_kernel", "avd_latent_guide_canvas_f32": "canvas_latent_guide_kernel<4>",
            "avd_renoise_canvas_f32 (guide)": "canvas_renoise_kernel<4>", "avd_renoise_canvas_f32 (no guide)": "canvas_renoise_kernel<4>"}
    for fn in entries.values():                         # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    L.prof_enable(True)
    rounds = {name: [] for name in entries}
    for _ in range(args.reps):
        for name, fn in entries.items():
            before = L.prof_report().get(tags[name], (0, 0.0, 0.0))
            for _ in range(args.launches):
                fn()
            torch.cuda.synchronize()
            after = L.prof_report()[tags[name]]
            assert after[0] - before[0] == args.launches, (name, before, after)
            rounds[name].append(1e3 * (after[1] - before[1]) / args.launches)
    L.prof_enable(False)
    mb = 4 * z0.numel() / 1e6
    print(f"latent {list(shape)} ({mb:.1f} MB per tensor), {args.reps} interleaved rounds of {args.launches} launches, us per launch:")
    for name, r in rounds.items():
        print(f"  {name:36s} " + "  ".join(f"{v:7.2f}" for v in r) + f"   median {statistics.median(r):7.2f}", flush=True)
    sys.exit(0)

mods, tdim = bench.build_modules(dev)
av, aa, core, head = mods
za = torch.randn(B, 8, 150, generator=torch.Generator().manual_seed(2)).to(dev)
sched = su.make_sampling_schedule(1000, S)
jump, resamples = args.resample
sched_r = su.resample_schedule(sched, jump, resamples)
kinds = [k for a, b, k in su.step_segments(sched_r, None) for _ in range(b - a)]
n_steps, n_jumps = sum(k != "renoise" for k in kinds), kinds.count("renoise")
eng = A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tdim, target="video", latent_shape=shape, prompt_tokens=37,
                      alpha_bar=abar, guidance=3.5, matmul=args.matmul, noise_seed=1234)
eng.set_prompt(za)
eng.set_known(known, mask, guide_seed=99)
start, _ = eng.start_latent(z0, sched, 1.0)
variants = (("resample=None", sched), (f"resample=({jump}, {resamples})", sched_r))
eng.run(start, su.resample_schedule(sched[-7:], 2, 2))     # warm-up: steps and jumps
times = {name: [] for name, _ in variants}
for _ in range(args.reps):
    for name, sc in variants:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.run(start, sc)
        torch.cuda.synchronize()
        times[name].append(1e3 * (time.perf_counter() - t0))
base = statistics.median(times["resample=None"])
for name, sc in variants:
    med = statistics.median(times[name])
    print(f"[{args.matmul}] A->V ddim B={B} {size}x{size} guided {name:20s}: {med:8.2f} ms per trajectory (min {min(times[name]):8.2f}, "
          f"{args.reps} rounds; {sc.numel() - 1} pairs)   x{med / base:.4f} vs resample=None", flush=True)
print(f"counted: {n_steps} denoising steps + {n_jumps} jumps against {S} steps: x{n_steps / S:.4f} in steps")
