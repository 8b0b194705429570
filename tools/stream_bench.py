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
The records are profiles/fifo_prompt_frac_kernels.txt and profiles/fifo_prompt_frac_e2e.txt.

--slot-momentum kernels | e2e times the slot APG momentum (include/avdiff_hip.h, "slot APG momentum") instead:
  kernels   at the C3 latent [B, 8, 12, 32, 32] (S = 6), B = 32 and 8, through the C entries of the fused slot update alone: the plain
            slot update, the slot APG update at beta = 0 and with a momentum buffer, with their statistics launches, for DDIM and
            DPM-Solver++(2M) at eta 0; the plain queue shift and the carry launch.  Kernel time under the library's launch events,
            --launches launches per window, the variants interleaved over --rounds rounds, all rounds printed.  On a checkout without
            the momentum the unchanged entries alone are timed (the plain update, the beta = 0 slot APG, the plain shift), so the
            same command on the parent commit gives the figures to compare.
  e2e       fifo_denoise under the slot APG with and without apg_momentum, DDIM at n = 48 and DPM-Solver++(2M) at n = 18 (8 layers),
            --slots-out and twice as many finished slots: the time per finished slot is the difference.
The records are profiles/slot_momentum_kernels.txt, profiles/slot_momentum_e2e.txt and profiles/slot_momentum_parent.txt.

--clips kernels | e2e times the FIFO clip batch (include/avdiff_hip.h, "FIFO clip batch") instead:
  kernels   at the C3 latent [K * B_q, 8, 12, 32, 32] (S = 6), K = 2, 4, 8 queues of B_q = 3 and K = 2, 4 of B_q = 8, without and with
            the history rider: the one multi-queue launch (functional.fifo_shift_clips) against what it replaces, K one-queue shifts
            on slices plus K copies of the popped heads into the canvases; beside them the unchanged one-queue plain and history shift
            at B = 3, 8 and 32, each timed twice per round.  Device events around --launches back-to-back iterations (launch overhead
            included: the two sides differ in their number of launches), the variants interleaved over --rounds rounds, all rounds
            printed.  On a checkout without the clip batch the unchanged shifts alone are timed, so the same command on the parent
            commit gives the figures to compare.
  e2e       fifo_denoise_clips (8 layers), DPM-Solver++(2M) at n = 18 with K = 1, 2, 4, 8, 10 clips and DDIM at n = 48 with K = 1, 2, 4:
            --slots-out and twice as many finished slots per clip, the time per finished slot per clip is the difference over K; one
            fifo_denoise line per solver beside them (the only line on a checkout without the clip batch).
The records are profiles/fifo_clips_kernels.txt, profiles/fifo_clips_e2e.txt and profiles/fifo_clips_parent.txt.

--clips keyed-kernels | keyed-e2e times the clip batch keying (include/avdiff_hip.h, "clip batch keying"):
  keyed-kernels  at the C3 latent [B, 8, 12, 32, 32] (S = 6), B = 30 as K = 10 queues of 3 and B = 32 as K = 4 queues of 8, the fused DDIM
                 and DPM-Solver++(2M) slot updates through their C entries at eta 0.5: with per-clip keys, with the per-clip guide, with
                 both, each beside the existing single-key and single-guide entry at the same B; the plain slot update and the existing
                 seeded update timed twice per round (their run-to-run spread), avd_fifo_shift_clips_f32, and the K-tail guide pass
                 against K single passes.  Kernel time under the library's launch events; device events where the sides differ in
                 their number of launches.  On a checkout without the keying the unchanged entries alone are timed, so the same
                 command on the parent commit gives the figures to compare.
  keyed-e2e      fifo_denoise_clips per finished slot per clip: DPM-Solver++(2M) at n = 18 with eta 0.5 at K = 1, 4, 10 and DDIM at n =
                 48 at K = 4, each beside the eta = 0 clip batch of the same build and beside fifo_denoise at eta 0.5 alone; the same
                 for a guided run (init_canvases against init_canvas).
The records are profiles/fifo_clips_keyed_kernels.txt, profiles/fifo_clips_keyed_parent.txt and profiles/fifo_clips_keyed_e2e.txt."""
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
ap.add_argument("--launches", type=int, default=200, help="--prompt-frac / --slot-momentum kernels: launches per timed window")
ap.add_argument("--slot-momentum", choices=("kernels", "e2e"), default=None, help="time the slot APG momentum instead (see above)")
ap.add_argument("--slots-out", type=int, default=12, help="--slot-momentum / --clips e2e: finished slots per timed fifo_denoise call")
ap.add_argument("--clips", choices=("kernels", "e2e", "keyed-kernels", "keyed-e2e"), default=None,
                help="time the FIFO clip batch, or its per-clip keying, instead (see above)")
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
geo = S.fifo_geometry(cfg, "audio", n_windows, args.steps) if args.prompt_frac is None and args.slot_momentum is None and args.clips is None else None
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


def slot_momentum_kernels():
    import ctypes as C
    from multimodal_diffusion_amd import _lib as L, functional as Fn, schedule_utils as su
    from oracle import ref_cpu as R
    lib = L.lib()
    has_mom = hasattr(Fn, "fifo_carry")
    abar = R.alpha_bar_table(R.beta_table(1000)).to(dev)
    S_, sl, T_ = 6, 2, 1000
    g = torch.Generator().manual_seed(0)
    PLAIN, CTL, MOM = "cfg_unpatch_ddim_kernel", "cfg_unpatch_ddim_kernel<slot cfg>", "cfg_unpatch_ddim_kernel<slot momentum>"
    STATS, STATS_M = "slot_cfg_stats_kernel", "slot_cfg_stats_kernel<momentum>"
    rows = []
    for B in (32, 8):
        shape = (B, 8, 12, 32, 32)
        z, hist, mom, out = (torch.randn(shape, generator=g).to(dev) for _ in range(4))
        eps2 = torch.randn(2 * B, 6 * 8 * 8, 256, generator=g).to(dev)
        nb = lib.avd_slot_cfg_stats_bytes(B, S_, 8 * sl * 32 * 32)
        stats = torch.empty(nb, dtype=torch.uint8, device=dev)
        key = L.SlotKey(0, 0, 1, None)
        for solver, n in (("ddim", 48), ("dpmpp_2m", 18)):
            dpm = solver == "dpmpp_2m"
            sched = su.make_sampling_schedule(T_, n)
            i = (torch.arange(B * S_) % (n - 2)).view(B, S_) + 1      # the diagonal: none held, none final
            tl, tn, tp = (sched[i + d].to(dev).contiguous() for d in (-1, 0, 1))
            head = (eps2.data_ptr(), z.data_ptr(), tl.data_ptr() if dpm else None, tn.data_ptr(), tp.data_ptr(), abar.data_ptr(), T_, 3.5, 0.0)
            tail = (S_, hist.data_ptr() if dpm else None, out.data_ptr(), *shape, 2, 4, 4)

            def plain(head=head, tail=tail):
                L.check(lib.avd_cfg_unpatch_ddim_slots_seeded_f32(*head, C.byref(key), *tail, L.stream_ptr(dev)))

            def ctl(beta, head=head, tail=tail):
                cfg_ = L.SlotCfg(None, None, 1, 20.0, 0.5, stats.data_ptr(), nb)
                if beta:      # the control with its two trailing fields
                    cfg_ = L.SlotCfgMomentum(None, None, L.SLOT_APG_MOMENTUM, 20.0, 0.5, stats.data_ptr(), nb, beta, mom.data_ptr())
                return lambda: L.check(lib.avd_cfg_unpatch_ddim_slots_cfg_f32(*head, None, None, *tail, C.byref(cfg_), L.stream_ptr(dev)))

            name = f"B={B} {solver}"
            rows += [(f"{name}: plain slot update (a)", PLAIN, plain), (f"{name}: slot APG beta = 0, update", CTL, ctl(0.0)),
                     (f"{name}: slot APG beta = 0, statistics", STATS, ctl(0.0))]
            if has_mom:
                rows += [(f"{name}: slot APG momentum, update", MOM, ctl(-0.5)), (f"{name}: slot APG momentum, statistics", STATS_M, ctl(-0.5))]
            rows += [(f"{name}: plain slot update (b)", PLAIN, plain)]
        shift = lambda z=z, B=B: Fn.fifo_shift(z, B * S_, 7, 999, sl)      # noqa: E731
        rows += [(f"B={B}: plain shift (a)", "fifo_shift_kernel<4>", shift)]
        if has_mom:
            rows += [(f"B={B}: carry", "fifo_carry_kernel<4>", lambda mom=mom, out=out: Fn.fifo_carry(mom, S_, sl, out=out))]
        rows += [(f"B={B}: plain shift (b)", "fifo_shift_kernel<4>", shift)]

    def per_launch_us(tag, fn):
        L.prof_enable(True)
        try:
            for _ in range(args.launches):
                fn()
            torch.cuda.synchronize()
        finally:
            L.prof_enable(False)
        n, ms, _ = L.prof_report()[tag]
        assert n == args.launches, (tag, n)
        return 1e3 * ms / n

    for _, _, fn in rows:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _, _ in rows}
    for _ in range(args.rounds):
        for name, tag, fn in rows:
            res[name].append(per_launch_us(tag, fn))
    print(f"C3 latent [B, 8, 12, 32, 32] (S = {S_} slots of 16384 elements: 16 chunks per slot), the fused CFG + un-patch + solver slot "
          f"update through its C entries (random eps tokens, the diagonal's tables: no slot held), eta 0: plain, under the slot APG at beta "
          f"= 0 and with a momentum buffer (beta -0.5), with the statistics launch of each; the plain queue shift and the carry launch.  "
          f"{args.rounds} interleaved rounds of {args.launches} launches, microseconds per launch (launch events)")
    if not has_mom:
        print("  this checkout has no slot momentum: the unchanged entries alone")
    for name, _, _ in rows:
        v = res[name]
        print(f"  {name:46s} " + " ".join(f"{x:8.2f}" for x in v) + f"   median {statistics.median(v):8.2f}")
    for B in (32, 8):                                      # the spread of the entries timed twice: what a difference has to exceed
        for what in ("ddim: plain slot update", "dpmpp_2m: plain slot update", "plain shift"):
            sep = " " if "shift" not in what else ": "
            v = res[f"B={B}{sep}{what} (a)"] + res[f"B={B}{sep}{what} (b)"]
            print(f"  B={B} {what}: run-to-run spread {min(v):.2f} .. {max(v):.2f}")


def slot_momentum_e2e():
    from multimodal_diffusion_amd import schedule_utils as su
    from oracle import ref_cpu as R
    abar = R.alpha_bar_table(R.beta_table(1000))
    S_, K = 6, args.slots_out
    g = torch.Generator().manual_seed(1)
    apg = {"norm_threshold": 20.0, "eta_parallel": 0.5}
    has_mom = "apg_momentum" in __import__("inspect").signature(A.fifo_denoise).parameters
    print(f"fifo_denoise under the slot APG without and with apg_momentum = -0.5 (one carry launch behind every shift), S = {S_} (C3 latent, "
          f"8 layers, {args.matmul}, eager), {args.rounds} rounds, the calls interleaved, {K} and {2 * K} slots out; milliseconds")
    for solver, n in (("ddim", 48), ("dpmpp_2m", 18)):
        sched = su.make_sampling_schedule(1000, n)
        canvas_p = torch.randn(8, 25 * (n + 2 * K) + 148, generator=g).to(dev)
        eng = A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tdim, target="video",
                              latent_shape=(n // S_, 8, 12, 32, 32), prompt_tokens=37, alpha_bar=abar, guidance=3.5, matmul=args.matmul,
                              solver=solver)
        kinds = [("apg", dict(apg=apg))] + ([("momentum", dict(apg=apg, apg_momentum=-0.5))] if has_mom else [])
        for _, kw_ in kinds:
            A.fifo_denoise(eng, canvas_p, 25, sched, 4, 5, **kw_)      # warm-up
        ts_ = {(name, K_): [] for name, _ in kinds for K_ in (K, 2 * K)}
        for _ in range(args.rounds):
            for K_ in (K, 2 * K):
                for name, kw_ in kinds:
                    ts_[name, K_].append(timed(lambda: A.fifo_denoise(eng, canvas_p, 25, sched, K_, 5, **kw_))[0])
        per = {}
        for name, _ in kinds:
            whole = {K_: statistics.median(ts_[name, K_]) for K_ in (K, 2 * K)}
            per[name] = (whole[2 * K] - whole[K]) / K
            print(f"  {solver:8s} n = {n}, B = {n // S_}, {name:8s}: " +
                  "; ".join(f"{K_} out " + " ".join(f"{t * 1e3:7.1f}" for t in ts_[name, K_]) for K_ in (K, 2 * K)) +
                  f"; per finished slot {per[name] * 1e3:.3f}")
        if has_mom:
            print(f"  {'':8s} per finished slot, momentum against none: {(per['momentum'] - per['apg']) * 1e3:+.3f} ms "
                  f"(x {per['momentum'] / per['apg']:.3f})")
    print("  quality is not measured: there are no trained weights")


def clips_kernels():
    from multimodal_diffusion_amd import _lib as L, functional as Fn
    has_clips = hasattr(Fn, "fifo_shift_clips")
    S_, sl, n_clip, c, t = 6, 2, 64, 48, 999
    g = torch.Generator().manual_seed(0)
    rows, pairs = [], []      # (name, fn, launches per iteration, bytes moved, the kernel's prof tag); (clip batch, its row of parts)
    slot = 8 * sl * 32 * 32 * 4

    def single(z, hist, hout):
        if hist is None:
            return lambda: Fn.fifo_shift(z, c, 7, t, sl)
        return lambda: Fn.fifo_shift(z, c, 7, t, sl, hist=hist, hist_out=hout)

    def measure(rows):
        """{name: [us per iteration of every round]} by device events, and {name: kernel us} under the library's launch events"""
        for _, fn, _, _, _ in rows:
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        us = {r[0]: [] for r in rows}
        for _ in range(args.rounds):
            for name, fn, _, _, _ in rows:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                us[name].append(1e3 * e0.elapsed_time(e1) / args.launches)
        kern = {}
        for name, fn, _, _, tag in rows:
            if tag is None:
                continue
            L.prof_enable(True)
            try:
                for _ in range(args.launches):
                    fn()
                torch.cuda.synchronize()
            finally:
                L.prof_enable(False)
            n, ms, _ = L.prof_report()[tag]
            assert n == args.launches, (tag, n)
            kern[name] = 1e3 * ms / n
        return us, kern

    def report(rows, us, kern):
        for name, _, launches, moved, _ in rows:
            v = us[name]
            med = statistics.median(v)
            k = f"   kernel alone {kern[name]:6.2f} = {moved / kern[name] / 1e3:7.1f} GB/s" if name in kern else ""
            print(f"  {name:44s} " + " ".join(f"{x:8.2f}" for x in v) + f"   median {med:8.2f}   {launches:2d} launch(es){k}")
        for B in (3, 8, 32):                               # the spread of the entries timed twice: what a difference has to exceed
            for what in ("plain shift", "history shift"):
                v = us[f"B={B}: {what} (a)"] + us[f"B={B}: {what} (b)"]
                print(f"  B={B} {what}: run-to-run spread {min(v):.2f} .. {max(v):.2f}")

    for B in (3, 8, 32):                                   # the unchanged one-queue entries, each twice per round
        z, hist, hout = (torch.randn((B, 8, 12, 32, 32), generator=g).to(dev) for _ in range(3))
        for tag in ("(a)", "(b)"):
            rows.append((f"B={B}: plain shift {tag}", single(z, None, None), 1, 2 * z.numel() * 4 + slot, "fifo_shift_kernel<4>"))
            rows.append((f"B={B}: history shift {tag}", single(z, hist, hout), 1, 4 * z.numel() * 4 + slot, "fifo_shift_kernel<4, HistShift>"))
    print(f"FIFO queue shifts at the C3 latent [B, 8, 12, 32, 32] (S = {S_} slots of {sl} frames, 16-byte lanes), through functional.* "
          f"(every call allocates its outputs, as the drivers' calls do): microseconds per iteration, device events around {args.launches} "
          f"back-to-back iterations (the host's launch work included: at these sizes it is what the loop waits for), {args.rounds} "
          f"interleaved rounds after a warm-up, then the median; kernel alone = the library's launch events around {args.launches} launches "
          "in a pass of their own, and the bytes the launch has to move over that time")
    print(" the unchanged one-queue shifts alone, before anything of the clip batch is allocated (the same pass on any checkout):")
    report(rows, *measure(rows))
    if not has_clips:
        print("  this checkout has no clip batch: nothing else to time")
        return
    for Bq, Ks in ((3, (2, 4, 8)), (8, (2, 4))):
        for K in Ks:
            z, hist, hout = (torch.randn((K * Bq, 8, 12, 32, 32), generator=g).to(dev) for _ in range(3))
            clips = torch.zeros(K, 8, n_clip * sl, 32, 32, device=dev)
            seeds = Fn.clip_seeds(list(range(1, K + 1)), K, dev)
            for rider in (False, True):
                moved = (4 if rider else 2) * z.numel() * 4 + K * slot

                def multi(z=z, hist=hist, hout=hout, clips=clips, seeds=seeds, K=K, rider=rider):
                    Fn.fifo_shift_clips(z, K, c, seeds, t, sl, clips, 5, hist=hist if rider else None, hist_out=hout if rider else None)

                def parts(z=z, hist=hist, hout=hout, clips=clips, K=K, Bq=Bq, rider=rider):
                    for k in range(K):
                        q = slice(k * Bq, (k + 1) * Bq)
                        res = Fn.fifo_shift(z[q], c, k + 1, t, sl, hist=hist[q] if rider else None, hist_out=hout[q] if rider else None)
                        clips[k, :, 5 * sl:6 * sl] = res[1]

                name = f"K={K} x B_q={Bq}{', history' if rider else ''}"
                rows += [(f"{name}: one launch", multi, 1, moved, f"fifo_shift_clips_kernel<4, {1 if rider else 0}>"),
                         (f"{name}: {K} shifts + {K} copies", parts, 2 * K, moved + K * slot, None)]
                pairs.append((name, rows[-1][0]))
    print(" every variant interleaved: the clip batch's one launch against the K one-queue shifts + K copies it replaces:")
    us, kern = measure(rows)
    report(rows, us, kern)
    for name, parts_name in pairs:
        a, b = statistics.median(us[f"{name}: one launch"]), statistics.median(us[parts_name])
        print(f"  {name:28s} one launch {a:8.2f} against {b:8.2f}: x {b / a:.2f}")


def clips_e2e():
    from multimodal_diffusion_amd import schedule_utils as su
    from oracle import ref_cpu as R
    abar = R.alpha_bar_table(R.beta_table(1000))
    S_, N = 6, args.slots_out
    has_clips = hasattr(A, "fifo_denoise_clips")
    g = torch.Generator().manual_seed(1)
    print(f"fifo_denoise_clips: K clips as K queues in one engine of batch K * B_q, S = {S_} (C3 latent [8, 12, 32, 32] per sample, 384 + 37 "
          f"tokens, 8 layers, {args.matmul}, eager, eta 0), audio prompt canvases with 25 latent frames per target slot; host clock around "
          f"calls that end in a device synchronise, {args.rounds} rounds, the calls interleaved, {N} and {2 * N} slots out per clip; "
          "milliseconds.  Per finished slot = the difference of the two clip lengths over the slots; per clip = that over K")
    if not has_clips:
        print("  this checkout has no clip batch: the fifo_denoise lines alone")
    for solver, n, Ks in (("dpmpp_2m", 18, (1, 2, 4, 8, 10)), ("ddim", 48, (1, 2, 4))):
        sched = su.make_sampling_schedule(1000, n)
        Bq = n // S_
        pcs = [torch.randn(8, 25 * (n + 2 * N) + 148, generator=g).to(dev) for _ in range(max(Ks))]

        def eng(B):
            return A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tdim, target="video",
                                   latent_shape=(B, 8, 12, 32, 32), prompt_tokens=37, alpha_bar=abar, guidance=3.5, matmul=args.matmul,
                                   solver=solver)

        e1 = eng(Bq)
        runs = [("fifo_denoise", 1, lambda n_out, e1=e1: A.fifo_denoise(e1, pcs[0], 25, sched, n_out, 5))]
        if has_clips:
            for K in Ks:
                eK = e1 if K == 1 else eng(K * Bq)
                runs.append((f"clips K = {K}", K, lambda n_out, eK=eK, K=K: A.fifo_denoise_clips(eK, pcs[:K], 25, sched, n_out,
                                                                                               list(range(5, 5 + K)))))
        for _, _, fn in runs:
            fn(4)                                          # warm-up
        ts_ = {(name, n_out): [] for name, _, _ in runs for n_out in (N, 2 * N)}
        for _ in range(args.rounds):
            for n_out in (N, 2 * N):
                for name, _, fn in runs:
                    ts_[name, n_out].append(timed(lambda: fn(n_out))[0])
        per1 = None
        for name, K, _ in runs:
            whole = {n_out: statistics.median(ts_[name, n_out]) for n_out in (N, 2 * N)}
            per = (whole[2 * N] - whole[N]) / N
            if name == "clips K = 1":
                per1 = per
            ratio = f"   x {per1 / (per / K):.2f} per clip against K = 1" if per1 is not None and K > 1 else ""
            print(f"  {solver:8s} n = {n}, B = {K * Bq:2d}, {name:13s}: " +
                  "; ".join(f"{n_out} out " + " ".join(f"{x * 1e3:7.1f}" for x in ts_[name, n_out]) for n_out in (N, 2 * N)) +
                  f"; per finished slot {per * 1e3:.3f}, per clip {per / K * 1e3:.3f}; ramp and start {(whole[N] - N * per) * 1e3:.1f}{ratio}")
    print("  quality is not measured: there are no trained weights")


def keyed_kernels():
    import ctypes as C
    from multimodal_diffusion_amd import _lib as L, functional as Fn, schedule_utils as su
    from oracle import ref_cpu as R
    lib = L.lib()
    has_keyed = hasattr(Fn, "slot_noise_clips")
    abar = R.alpha_bar_table(R.beta_table(1000)).to(dev)
    S_, sl, T_, P_ = 6, 2, 1000, 480      # every position of either walk inside the canvases
    g = torch.Generator().manual_seed(0)
    PLAIN, GUIDE, QUEUES = "cfg_unpatch_ddim_kernel", "cfg_unpatch_ddim_kernel<clip guide>", "cfg_unpatch_ddim_kernel<clip queues>"
    rows, passes, keep = [], [], []      # (name, prof tag, fn); (name, fn, launches) timed by device events; what the raw addresses need
    for B, K in ((30, 10), (32, 4)):
        shape = (B, 8, 12, 32, 32)
        z, hist, out = (torch.randn(shape, generator=g).to(dev) for _ in range(3))
        eps2 = torch.randn(2 * B, 6 * 8 * 8, 256, generator=g).to(dev)
        known = torch.randn(K, 8, P_, 32, 32, generator=g).to(dev)
        masks = (torch.rand(K, 8, P_, 32, 32, generator=g) < 0.5).float().to(dev)
        seeds = Fn.clip_seeds(list(range(1, K + 1)), K, dev)
        key = L.SlotKey(7, 40, S_, None)
        guide1 = L.ClipGuide(known.data_ptr(), masks.data_ptr(), P_, 9, 40, S_, None)      # K canvases: the single guide reads the first
        cq = L.ClipQueues(K, seeds.data_ptr(), seeds.data_ptr()) if has_keyed else None
        keep += [z, hist, out, eps2, known, masks, seeds]
        for solver, n in (("ddim", 48), ("dpmpp_2m", 18)):
            dpm = solver == "dpmpp_2m"
            sched = su.make_sampling_schedule(T_, n)
            i = (torch.arange(B * S_) % (n - 2)).view(B, S_) + 1      # the diagonal: none held, none final
            tl, tn, tp = (sched[i + d].to(dev).contiguous() for d in (-1, 0, 1))
            tail = (S_, hist.data_ptr() if dpm else None, out.data_ptr(), *shape, 2, 4, 4)

            keep += [tl, tn, tp]      # the closures below hold raw addresses: every tensor and struct of this pass stays alive, and
            #                           every name is bound here, not when the closure runs (the loop rebinds them all)
            head = {eta: (eps2.data_ptr(), z.data_ptr(), tl.data_ptr() if dpm else None, tn.data_ptr(), tp.data_ptr(), abar.data_ptr(), T_,
                          3.5, eta) for eta in (0.0, 0.5)}

            def seeded(eta, head=head, tail=tail, key=key):
                return lambda: L.check(lib.avd_cfg_unpatch_ddim_slots_seeded_f32(*head[eta], C.byref(key), *tail, L.stream_ptr(dev)))

            def guided(eta, head=head, tail=tail, key=key, guide1=guide1):
                return lambda: L.check(lib.avd_cfg_unpatch_ddim_slots_guided_f32(*head[eta], C.byref(key), C.byref(guide1), *tail,
                                                                                 L.stream_ptr(dev)))

            def clips(eta, with_guide, head=head, tail=tail, key=key, guide1=guide1, cq=cq):
                return lambda: L.check(lib.avd_cfg_unpatch_ddim_slots_clips_f32(*head[eta], C.byref(key), C.byref(guide1) if with_guide else None,
                                                                                C.byref(cq), *tail, None, L.stream_ptr(dev)))

            name = f"B={B} K={K} {solver}"
            rows += [(f"{name}: plain slot update, eta 0 (a)", PLAIN, seeded(0.0)), (f"{name}: single key, eta 0.5 (a)", PLAIN, seeded(0.5))]
            if has_keyed:
                rows += [(f"{name}: per-clip keys, eta 0.5", QUEUES, clips(0.5, False))]
            rows += [(f"{name}: single guide, eta 0", GUIDE, guided(0.0))]
            if has_keyed:
                rows += [(f"{name}: per-clip guide, eta 0", QUEUES, clips(0.0, True))]
            rows += [(f"{name}: single key + guide, eta 0.5", GUIDE, guided(0.5))]
            if has_keyed:
                rows += [(f"{name}: per-clip keys + guide, eta 0.5", QUEUES, clips(0.5, True))]
            rows += [(f"{name}: plain slot update, eta 0 (b)", PLAIN, seeded(0.0)), (f"{name}: single key, eta 0.5 (b)", PLAIN, seeded(0.5))]
        canv = torch.zeros(K, 8, 64 * sl, 32, 32, device=dev)
        rows += [(f"B={B} K={K}: fifo_shift_clips ({tag})", "fifo_shift_clips_kernel<4, 0>",
                  lambda z=z, K=K, canv=canv, seeds=seeds: Fn.fifo_shift_clips(z, K, 48, seeds, 999, sl, canv, 5)) for tag in ("a", "b")]
        # the K entering tails: one launch of the clip batch's pass against K one-queue passes on slices, in place
        Bq = B // K
        tails = torch.full((B, S_), Fn.SLOT_LEAVE, dtype=torch.long, device=dev)
        tails[Bq - 1::Bq, S_ - 1] = 999

        def single_passes(z=z, K=K, Bq=Bq, known=known, masks=masks, tails=tails):
            for k in range(K):
                q = slice(k * Bq, (k + 1) * Bq)
                Fn.clip_guide_slots(known[k], tails[q], abar, z[q], masks[k], slot_len=sl, seed=k + 1, first=40, out=z[q])

        passes.append((f"B={B} K={K}: {K} single tail passes", single_passes, K))
        if has_keyed:
            passes.append((f"B={B} K={K}: one K-tail pass", lambda z=z, known=known, masks=masks, tails=tails, seeds=seeds:
                           Fn.clip_guide_slots_clips(known, tails, abar, z, masks, slot_len=sl, seeds=seeds, first=40, out=z), 1))

    def per_launch_us(tag, fn):
        L.prof_enable(True)
        try:
            for _ in range(args.launches):
                fn()
            torch.cuda.synchronize()
        finally:
            L.prof_enable(False)
        n, ms, _ = L.prof_report()[tag]
        assert n == args.launches, (tag, n)
        return 1e3 * ms / n

    for _, _, fn in rows:
        for _ in range(3):
            fn()
    for _, fn, _ in passes:
        fn()
    torch.cuda.synchronize()
    res = {name: [] for name, _, _ in rows}
    ev = {name: [] for name, _, _ in passes}
    for _ in range(args.rounds):
        for name, tag, fn in rows:
            res[name].append(per_launch_us(tag, fn))
        for name, fn, _ in passes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ev[name].append(1e3 * e0.elapsed_time(e1) / args.launches)
    print(f"C3 latent [B, 8, 12, 32, 32] (S = {S_} slots of {sl} frames), the fused CFG + un-patch + solver slot update through its C entries "
          f"(random eps tokens, the diagonal's tables: no slot held), the rows form: one key / one guide for the batch (the existing entries) "
          f"against one per queue (avd_cfg_unpatch_ddim_slots_clips_f32), canvases of P = {P_} positions with a half-open mask; and "
          f"avd_fifo_shift_clips_f32.  {args.rounds} interleaved rounds of {args.launches} launches, microseconds per launch (launch events)")
    if not has_keyed:
        print("  this checkout has no clip batch keying: the unchanged entries alone")
    for name, _, _ in rows:
        v = res[name]
        print(f"  {name:52s} " + " ".join(f"{x:8.2f}" for x in v) + f"   median {statistics.median(v):8.2f}")
    for name in sorted({n[:-4] for n in res if n.endswith("(a)")}):      # the spread of the entries timed twice: what a difference has to exceed
        v = res[name + " (a)"] + res[name + " (b)"]
        print(f"  {name}: run-to-run spread {min(v):.2f} .. {max(v):.2f}")
    print(f" the entering tails' guide pass, in place, through functional.* (device events around {args.launches} back-to-back iterations, "
          "the host's launch work included), microseconds per iteration:")
    for name, _, launches in passes:
        v = ev[name]
        print(f"  {name:52s} " + " ".join(f"{x:8.2f}" for x in v) + f"   median {statistics.median(v):8.2f}   {launches:2d} launch(es)")


def keyed_e2e():
    from multimodal_diffusion_amd import schedule_utils as su
    from oracle import ref_cpu as R
    abar = R.alpha_bar_table(R.beta_table(1000))
    S_, N = 6, args.slots_out
    g = torch.Generator().manual_seed(1)
    print(f"fifo_denoise_clips with per-clip step seeds (eta 0.5) and per-clip init canvases, S = {S_} (C3 latent [8, 12, 32, 32] per sample, "
          f"8 layers, {args.matmul}, eager), beside the eta = 0 clip batch of the same build and fifo_denoise alone; host clock around calls "
          f"that end in a device synchronise, {args.rounds} rounds, the calls interleaved, {N} and {2 * N} slots out per clip; milliseconds.  "
          "Per finished slot = the difference of the two clip lengths over the slots; per clip = that over K")
    for solver, n, Ks in (("dpmpp_2m", 18, (1, 4, 10)), ("ddim", 48, (4,))):
        sched = su.make_sampling_schedule(1000, n)
        Bq = n // S_
        pcs = [torch.randn(8, 25 * (n + 2 * N) + 148, generator=g).to(dev) for _ in range(max(Ks))]
        canv = [torch.randn(8, 2 * (n + 2 * N), 32, 32, generator=g).to(dev) for _ in range(max(Ks))]
        mask = torch.zeros(8, 2 * (n + 2 * N), 32, 32, device=dev)
        mask[:, ::4] = 1.0

        def eng(B, eta):
            return A.DenoiseEngine(adapt_v=av, adapt_a=aa, core=core, head=head, tstep_dim=tdim, target="video",
                                   latent_shape=(B, 8, 12, 32, 32), prompt_tokens=37, alpha_bar=abar, guidance=3.5, matmul=args.matmul,
                                   solver=solver, eta=eta, noise_seed=3)

        e1 = eng(Bq, 0.5)
        runs = [("fifo_denoise eta .5", 1, lambda n_out, e1=e1: A.fifo_denoise(e1, pcs[0], 25, sched, n_out, 5)),
                ("fifo_denoise guided", 1, lambda n_out, e1=e1: A.fifo_denoise(e1, pcs[0], 25, sched, n_out, 5, init_canvas=canv[0], mask=mask))]
        for K in Ks:
            e0, eK = eng(K * Bq, 0.0), (e1 if K == 1 else eng(K * Bq, 0.5))
            seeds = list(range(5, 5 + K))
            runs += [(f"K = {K:2d} eta 0", K, lambda n_out, e0=e0, K=K, seeds=seeds: A.fifo_denoise_clips(e0, pcs[:K], 25, sched, n_out, seeds)),
                     (f"K = {K:2d} eta .5 keyed", K, lambda n_out, eK=eK, K=K, seeds=seeds:
                      A.fifo_denoise_clips(eK, pcs[:K], 25, sched, n_out, seeds, step_seeds=seeds)),
                     (f"K = {K:2d} eta .5 guided", K, lambda n_out, eK=eK, K=K, seeds=seeds:
                      A.fifo_denoise_clips(eK, pcs[:K], 25, sched, n_out, seeds, step_seeds=seeds, init_canvases=canv[:K], masks=[mask] * K))]
        for _, _, fn in runs:
            fn(4)                                          # warm-up
        ts_ = {(name, n_out): [] for name, _, _ in runs for n_out in (N, 2 * N)}
        for _ in range(args.rounds):
            for n_out in (N, 2 * N):
                for name, _, fn in runs:
                    ts_[name, n_out].append(timed(lambda: fn(n_out))[0])
        for name, K, _ in runs:
            whole = {n_out: statistics.median(ts_[name, n_out]) for n_out in (N, 2 * N)}
            per = (whole[2 * N] - whole[N]) / N
            print(f"  {solver:8s} n = {n}, B = {K * Bq:2d}, {name:20s}: " +
                  "; ".join(f"{n_out} out " + " ".join(f"{x * 1e3:7.1f}" for x in ts_[name, n_out]) for n_out in (N, 2 * N)) +
                  f"; per finished slot {per * 1e3:.3f}, per clip {per / K * 1e3:.3f}")
    print("  quality is not measured: there are no trained weights")


if args.clips is not None:
    {"kernels": clips_kernels, "e2e": clips_e2e, "keyed-kernels": keyed_kernels, "keyed-e2e": keyed_e2e}[args.clips]()
    sys.exit(0)
if args.prompt_frac is not None:
    prompt_frac_kernels() if args.prompt_frac == "kernels" else prompt_frac_e2e()
    sys.exit(0)
if args.slot_momentum is not None:
    slot_momentum_kernels() if args.slot_momentum == "kernels" else slot_momentum_e2e()
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
