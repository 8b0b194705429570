#!/usr/bin/env python3
"""End-to-end audio->video generation for one batch on one GPU (GPU box): 50 DDIM + CFG steps at 256x256 (the bench.py
workload) followed by VideoVAE.decode of the whole batch — the part of sample_one_direction (sample_clip.py:220-394) that runs
on the device.  Prints the sampler / decode split for the matrix-pipe modes, then the other direction (video -> audio,
sample_clip.py:313-352): VideoVAE.encode of the batch of prompt clips, 50 steps on the audio latent, AudioCodec.decode."""
import argparse
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import multimodal_diffusion_amd as A                                   # noqa: E402
from multimodal_diffusion_amd import schedule_utils as su              # noqa: E402
import bench                                                           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--size", type=int, default=256)
ap.add_argument("--sampler-steps", type=int, default=50)
ap.add_argument("--solver", choices=("ddim", "dpmpp_2m"), default="ddim",
                help="sampler of the end-to-end runs (DenoiseEngine solver=): DDIM or DPM-Solver++(2M)")
ap.add_argument("--modes", default="f32,bf16x3,f16x2", help="comma-separated matrix-pipe modes of the end-to-end runs")
ap.add_argument("--eta", type=float, default=None,
                help="time only the sampler loop, both directions, at eta = 0 against eta = ETA (DDIM noise per step) instead of the "
                     "end-to-end runs; the variants run interleaved in one process")
ap.add_argument("--noise", choices=("both", "seeded", "unseeded"), default="both",
                help="with --eta: the eta > 0 noise source(s) to time — seeded (the in-kernel stream of DenoiseEngine(noise_seed=...)) "
                     "and / or unseeded (torch.randn_like per step)")
ap.add_argument("--matmul", default="bf16x3", help="with --eta: matrix-pipe mode (default: bench.py's headline mode)")
ap.add_argument("--reps", type=int, default=5, help="with --eta / --strength / --keep-frames / --guidance-rescale: interleaved rounds; the median per variant "
                                                   "is printed")
ap.add_argument("--strength", type=float, default=None,
                help="time only the A->V sampler loop with a latent guide (DenoiseEngine.set_known / start_latent) at this SDEdit strength "
                     "beside the unguided loop, interleaved in one process")
ap.add_argument("--keep-frames", type=int, default=None,
                help="with or without --strength: hold the first K latent frames to the known clip (frame_mask) at every step")
ap.add_argument("--guidance-rescale", type=float, default=None,
                help="time only the sampler loop, both directions, plain CFG against DenoiseEngine(guidance_rescale=PHI) (statistics "
                     "pass + controlled fused step), interleaved in one process")
ap.add_argument("--apg", action="store_true",
                help="with --guidance-rescale: also time DenoiseEngine(apg=...) (adaptive projected guidance: statistics pass + APG fused "
                     "step) without and with momentum, in the same interleaved rounds")
ap.add_argument("--guidance-interval", type=int, nargs=2, default=None, metavar=("LO", "HI"),
                help="time only the sampler loop, both directions, the plain trajectory against DenoiseEngine(guidance_interval=(LO, HI)) "
                     "(cond-only steps outside the interval), interleaved in one process")
ap.add_argument("--consensus-hop", type=int, default=None, metavar="HOP",
                help="time only the sampler loop, the plain trajectory against DenoiseEngine.set_window_consensus(HOP) (the batch as "
                     "consecutive windows of one latent canvas, HOP latent frames apart; the audio direction takes HOP * 150 / 12 "
                     "latent frames), interleaved in one process")
args = ap.parse_args()
dev = torch.device("cuda:0")
B, S, size = args.batch, args.sampler_steps, args.size
mods, tdim = bench.build_modules(dev)
av, aa, core, head = mods
torch.manual_seed(0)
vae = A.VideoVAE.from_config({"latent": {"channels": 8, "t_down": 4, "s_down": 8}}).eval().to(dev)
abar = su.alphas_cumprod_from_betas(su.make_beta_schedule(1000, "cosine", 1e-4, 0.02))[1]
sched = su.make_sampling_schedule(1000, S)
z0 = torch.randn(B, 8, 12, size // 8, size // 8, generator=torch.Generator().manual_seed(1)).to(dev)
za = torch.randn(B, 8, 150, generator=torch.Generator().manual_seed(2)).to(dev)

if args.eta is not None:
    # eta > 0 cost: the same trajectory at eta = 0, at eta = ETA with torch.randn_like noise per step (eager: a captured graph would
    # replay one draw) and at eta = ETA with the seeded in-kernel stream (graph replay where run() takes it, as at eta = 0)
    import statistics
    variants = [("eta=0", 0.0, None)]
    if args.noise in ("both", "unseeded"):
        variants.append((f"eta={args.eta:g} unseeded", args.eta, None))
    if args.noise in ("both", "seeded"):
        variants.append((f"eta={args.eta:g} seeded", args.eta, 1234))
    zv_prompt = torch.randn(B, 8, 12, size // 8, size // 8, generator=torch.Generator().manual_seed(3)).to(dev)
    for target, z_init, prompt, n_prompt in (("video", z0, za, 37), ("audio", za, zv_prompt, (12 // 2) * (size // 8 // 4) ** 2)):
        engs = []
        for name, eta, seed in variants:
            eng = A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tdim, target=target,
                                  latent_shape=tuple(z_init.shape), prompt_tokens=n_prompt, alpha_bar=abar, guidance=3.5, eta=eta,
                                  matmul=args.matmul, noise_seed=seed)
            eng.set_prompt(prompt)
            eng.run(z_init, sched[:4])                  # warm-up (a graph-replaying variant captures here too)
            engs.append(eng)
        times = {name: [] for name, _, _ in variants}
        for _ in range(args.reps):
            for (name, _, _), eng in zip(variants, engs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.run(z_init, sched)
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0) / S)
        base = statistics.median(times["eta=0"])
        direction = "A->V" if target == "video" else "V->A"
        rows = 2 * B * (engs[0].N)
        for (name, _, _), eng in zip(variants, engs):
            med = statistics.median(times[name])
            graph = (eng.eta == 0 or eng.noise_seed is not None) and rows < eng.GRAPH_BELOW_ROWS
            print(f"[{args.matmul}] {direction} B={B} {size}x{size} {name:18s}: {med:7.3f} ms/step (min {min(times[name]):7.3f}, "
                  f"{args.reps} rounds of {S} steps, {'graph' if graph else 'eager'})  {100 * (med / base - 1):+6.2f} % vs eta=0", flush=True)
    sys.exit(0)

if args.guidance_interval is not None:
    # guidance interval: the plain engine against one whose steps outside [LO, HI] are cond-only, interleaved; ms/step and clips/s medians
    import statistics
    zv_prompt = torch.randn(B, 8, 12, size // 8, size // 8, generator=torch.Generator().manual_seed(3)).to(dev)
    lo, hi = args.guidance_interval
    variants = (("plain", None), (f"interval=[{lo},{hi}]", (lo, hi)))
    for target, z_init, prompt, n_prompt in (("video", z0, za, 37), ("audio", za, zv_prompt, (12 // 2) * (size // 8 // 4) ** 2)):
        engs = []
        for name, iv in variants:
            eng = A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tdim, target=target,
                                  latent_shape=tuple(z_init.shape), prompt_tokens=n_prompt, alpha_bar=abar, guidance=3.5,
                                  guidance_interval=iv, matmul=args.matmul, solver=args.solver)
            eng.set_prompt(prompt)
            eng.run(z_init, sched)                      # warm-up: both kinds of step (and their graphs where run() captures)
            engs.append(eng)
        n_cfg = sum(b - a for a, b, c in su.guidance_segments(sched, (lo, hi)) if c)
        times = {name: [] for name, _ in variants}
        for _ in range(args.reps):
            for (name, _), eng in zip(variants, engs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.run(z_init, sched)
                torch.cuda.synchronize()
                times[name].append(time.perf_counter() - t0)
        base = statistics.median(times["plain"])
        direction = "A->V" if target == "video" else "V->A"
        for name, iv in variants:
            med = statistics.median(times[name])
            print(f"[{args.matmul}] {direction} {args.solver} B={B} {size}x{size} {name:22s}: {1e3 * med / S:7.3f} ms/step (min "
                  f"{1e3 * min(times[name]) / S:7.3f}, max {1e3 * max(times[name]) / S:7.3f}), {B / med:8.2f} clips/s, {args.reps} rounds of {S} "
                  f"steps ({n_cfg if iv else S} CFG)  {100 * (med / base - 1):+6.2f} % vs plain", flush=True)
    sys.exit(0)

if args.guidance_rescale is not None:
    # CFG rescale cost: the plain engine against one with guidance_rescale = PHI, interleaved; ms/step medians
    import statistics
    zv_prompt = torch.randn(B, 8, 12, size // 8, size // 8, generator=torch.Generator().manual_seed(3)).to(dev)
    variants = (("plain", {}), (f"rescale={args.guidance_rescale:g}", dict(guidance_rescale=args.guidance_rescale)))
    if args.apg:
        apg = dict(norm_threshold=15.0, eta_parallel=0.0)
        variants += (("apg", dict(apg=dict(apg, momentum=0.0))), ("apg momentum", dict(apg=dict(apg, momentum=-0.5))))
    for target, z_init, prompt, n_prompt in (("video", z0, za, 37), ("audio", za, zv_prompt, (12 // 2) * (size // 8 // 4) ** 2)):
        engs = []
        for name, ctl in variants:
            eng = A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tdim, target=target,
                                  latent_shape=tuple(z_init.shape), prompt_tokens=n_prompt, alpha_bar=abar, guidance=3.5,
                                  matmul=args.matmul, solver=args.solver, **ctl)
            eng.set_prompt(prompt)
            eng.run(z_init, sched[:4])                  # warm-up
            engs.append(eng)
        times = {name: [] for name, _ in variants}
        for _ in range(args.reps):
            for (name, _), eng in zip(variants, engs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.run(z_init, sched)
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0) / S)
        base = statistics.median(times["plain"])
        direction = "A->V" if target == "video" else "V->A"
        for name, _ in variants:
            med = statistics.median(times[name])
            print(f"[{args.matmul}] {direction} {args.solver} B={B} {size}x{size} {name:14s}: {med:7.3f} ms/step (min {min(times[name]):7.3f}, "
                  f"{args.reps} rounds of {S} steps)  {100 * (med / base - 1):+6.2f} % vs plain", flush=True)
    sys.exit(0)

if args.consensus_hop is not None:
    # window consensus cost: the plain engine against one whose every step ends with the consensus pass over its output, interleaved
    import statistics
    zv_prompt = torch.randn(B, 8, 12, size // 8, size // 8, generator=torch.Generator().manual_seed(3)).to(dev)
    for target, z_init, prompt, n_prompt, hop in (("video", z0, za, 37, args.consensus_hop),
                                                  ("audio", za, zv_prompt, (12 // 2) * (size // 8 // 4) ** 2, args.consensus_hop * 150 // 12)):
        engs = {}
        for name in ("plain", f"consensus hop={hop}"):
            eng = A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tdim, target=target,
                                  latent_shape=tuple(z_init.shape), prompt_tokens=n_prompt, alpha_bar=abar, guidance=3.5,
                                  matmul=args.matmul, solver=args.solver)
            eng.set_prompt(prompt)
            if name != "plain":
                eng.set_window_consensus(hop)
            eng.run(z_init, sched[:4])                  # warm-up (a graph-replaying variant captures here too)
            engs[name] = eng
        times = {name: [] for name in engs}
        for _ in range(args.reps):
            for name, eng in engs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                eng.run(z_init, sched)
                torch.cuda.synchronize()
                times[name].append(1e3 * (time.perf_counter() - t0) / S)
        base = statistics.median(times["plain"])
        for name in engs:
            med = statistics.median(times[name])
            print(f"[{args.matmul}] {'A->V' if target == 'video' else 'V->A'} {args.solver} B={B} {size}x{size} {name:18s}: {med:7.3f} ms/step "
                  f"(min {min(times[name]):7.3f}, {args.reps} rounds of {S} steps)  {100 * (med / base - 1):+6.2f} % vs plain", flush=True)
    sys.exit(0)

if args.strength is not None or args.keep_frames is not None:
    # latent guide cost: the unguided trajectory against the guided one (start_latent at --strength, a frame_mask of --keep-frames
    # held at every step through the fused guided step); ms/step over the steps each variant runs
    import statistics
    strength = 1.0 if args.strength is None else args.strength
    K = args.keep_frames or 0
    known = torch.randn(z0.shape, generator=torch.Generator().manual_seed(4)).to(dev)
    engs = {}
    for name in ("unguided", "guided"):
        eng = A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tdim, target="video", latent_shape=tuple(z0.shape),
                              prompt_tokens=37, alpha_bar=abar, guidance=3.5, matmul=args.matmul, solver=args.solver)
        eng.set_prompt(za)
        if name == "guided":
            eng.set_known(known, A.frame_mask(tuple(z0.shape[1:]), 0, K), guide_seed=5)
        eng.run(z0, sched[:4])                          # warm-up
        engs[name] = eng
    times = {name: [] for name in engs}
    n_run = {}
    for _ in range(args.reps):
        for name, eng in engs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if name == "guided":
                z, sk = eng.start_latent(z0, sched, strength)
                if K == 0:
                    eng.clear_known()                   # SDEdit without a mask: the plain step
                eng.run(z, sk)
                if K == 0:
                    eng.set_known(known, None, guide_seed=5)
            else:
                sk = sched
                eng.run(z0, sched)
            torch.cuda.synchronize()
            n_run[name] = sk.numel() - 1
            times[name].append(1e3 * (time.perf_counter() - t0) / max(n_run[name], 1))
    base = statistics.median(times["unguided"])
    for name in engs:
        med = statistics.median(times[name])
        print(f"[{args.matmul}] A->V {args.solver} B={B} {size}x{size} {name:8s} strength={strength if name == 'guided' else 1.0:g} "
              f"keep_frames={K if name == 'guided' else 0}: {med:7.3f} ms/step (min {min(times[name]):7.3f}, {args.reps} rounds of "
              f"{n_run[name]} steps)  {100 * (med / base - 1):+6.2f} % vs unguided", flush=True)
    sys.exit(0)

MODES = args.modes.split(",")
for mode in MODES:
    vae.matmul = mode
    eng = A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tdim, target="video", latent_shape=tuple(z0.shape),
                          prompt_tokens=37, alpha_bar=abar, guidance=3.5, matmul=mode, solver=args.solver)
    eng.set_prompt(za)
    z = eng.run(z0, sched[:3])                      # warm-up
    x = vae.decode(torch.randn_like(z))             # full-batch warm-up: the decoder's workspace (tens of GB) is allocated here
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    z = eng.run(z0, sched)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    # the random-weight trajectory explodes numerically (|z| ~ 1e5); decode a unit-scale latent of the same shape
    x = vae.decode(torch.randn_like(z))
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"[{mode:6s}] {args.solver} B={B} {size}x{size}: sampler {S} steps {1e3 * (t1 - t0):7.1f} ms ({1e3 * (t1 - t0) / S:.2f} ms/step)  "
          f"VAE decode {1e3 * (t2 - t1):7.1f} ms ({1e3 * (t2 - t1) / B:.2f} ms/sample)  total {1e3 * (t2 - t0):7.1f} ms  "
          f"= {B / (t2 - t0):.1f} clips/s   out {tuple(x.shape)}", flush=True)

# ---- video -> audio: encode the prompt clips, 50 steps on [B, 8, 150] with 384 prompt tokens, codec decode
codec = A.AudioCodec.from_config({"sr": 16000, "latent": {"channels": 8}, "codec": {"hop_samples": 320}}).eval().to(dev)
xv = (torch.rand(B, 3, 48, size, size, generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
for mode in MODES:
    vae.matmul = mode
    eng = A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tdim, target="audio", latent_shape=tuple(za.shape),
                          prompt_tokens=(12 // 2) * (size // 8 // 4) ** 2, alpha_bar=abar, guidance=3.5, matmul=mode,
                          solver=args.solver)      # tube patches 2 x 4 x 4
    zp = vae.encode(xv)                              # warm-up (workspace)
    eng.set_prompt(zp)
    eng.run(za, sched[:3])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    zp = vae.encode(xv)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    eng.set_prompt(zp)
    z = eng.run(za, sched)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    t3 = t2
    if codec is not None:
        wav = codec.decode(torch.randn_like(z))
        torch.cuda.synchronize()
        t3 = time.perf_counter()
    print(f"[{mode:6s}] {args.solver} V->A B={B} {size}x{size}: VAE encode {1e3 * (t1 - t0):7.1f} ms ({1e3 * (t1 - t0) / B:.2f} ms/sample)  sampler {S} steps "
          f"{1e3 * (t2 - t1):7.1f} ms ({1e3 * (t2 - t1) / S:.2f} ms/step)  codec decode {1e3 * (t3 - t2):6.1f} ms  total {1e3 * (t3 - t0):7.1f} ms  "
          f"= {B / (t3 - t0):.1f} clips/s", flush=True)
